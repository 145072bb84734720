// Score calibration and fusion (include/svk.h "calibration"): the statistics a prior-weighted logistic regression needs from
// a development trial list -- objective, gradient, Hessian at given weights -- in ONE streaming pass per Newton iteration, and
// the affine map llr = sum_d w_d s_d + b applied to a score list.  The reference has neither (its scores are raw cosines); on a
// framework this is a dozen float64 element-wise passes and reductions per iteration over 1.8e8 trials.
//
// svk_calibration_stats is a reduce-then-scan like roc.hip: stats_kernel gives every workgroup a contiguous span of QUADS (four
// consecutive trials), each thread adds its quads' terms to float64 accumulators in registers, a wave butterfly and an in-order
// sum over the four waves leave one row of partials per workgroup in the workspace, and finish_kernel, ONE workgroup, adds the
// rows in index order.  No floating-point atomics, no workgroup waits on another, and the geometry (stats_geometry) is a
// function of n alone -- not of the device's CU count -- so the order of additions is the one svk.h states and runs are
// bit-identical.  Instantiated per n_sys (1 .. 8): n_sys = 1 carries 2 + 2 + 3 accumulators, n_sys = 8 carries 2 + 9 + 45.
#include "svk_internal.h"

namespace {

constexpr int RT = 256;                  // threads per workgroup
constexpr int WAVES = RT / 64;
constexpr int MAX_SYS = 8;
constexpr unsigned GMAX = 2048;          // workgroups of stats_kernel at most (8 per CU on 256 CUs)

constexpr int n_out(int ns) { return 2 + (ns + 1) + (ns + 1) * (ns + 2) / 2; }   // L_tar, L_non, G, packed upper H

struct Weights {
  double w[MAX_SYS + 1];   // [n_sys] = the offset
  double tau, c_tar, c_non;
};

// Workgroup g of G owns the quads [g * span, min(quads, (g + 1) * span)), span a multiple of RT: a function of n alone.
struct Geometry {
  size_t quads, span;
  unsigned grid, steps;   // steps = span / RT: the quads a thread adds at most
};
Geometry stats_geometry(size_t n) {
  Geometry g;
  g.quads = (n + 3) / 4;
  const size_t units = (g.quads + RT - 1) / RT;
  g.steps = (unsigned)((units + GMAX - 1) / GMAX);
  g.span = (size_t)g.steps * RT;
  g.grid = (unsigned)((g.quads + g.span - 1) / g.span);
  return g;
}

// Workspace: double part[grid][n_out(n_sys)], then u64 cnt[grid][3], then the results: double fin[n_out], u64 fcnt[3].
struct Layout {
  size_t part, cnt, fin, fcnt, total;
};
Layout stats_layout(const Geometry& g, int ns) {
  Layout l;
  const size_t no = (size_t)n_out(ns);
  l.part = 0;
  l.cnt = l.part + (size_t)g.grid * no * 8;
  l.fin = l.cnt + (size_t)g.grid * 3 * 8;
  l.fcnt = l.fin + no * 8;
  l.total = (l.fcnt + 3 * 8 + 255) & ~(size_t)255;
  return l;
}

__device__ __forceinline__ bool finite_f32(float s) { return (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u; }

// sum_d w_d (double) s_d in the order d = 0, 1, ..., then the offset: every product and every sum rounded on its own
template <int NS>
__device__ __forceinline__ double affine(const double (&w)[MAX_SYS + 1], const float (&s)[NS]) {
#pragma clang fp contract(off)
  double z = w[0] * (double)s[0];
#pragma unroll
  for (int d = 1; d < NS; ++d) z = z + w[d] * (double)s[d];
  return z + w[NS];
}

// One trial's terms into acc: [0] L_tar, [1] L_non, [2 ..] G, then H's upper triangle row by row.  `on` is false for the padding
// of the last quad and for a trial with a non-finite score: its terms are +0.0, which change no bit of a sum.
template <int NS, bool VALUE_ONLY>
__device__ __forceinline__ void add_trial(const Weights& wt, const float (&s)[NS], bool target, bool on,
                                          double (&acc)[VALUE_ONLY ? 2 : n_out(NS)]) {
  constexpr int D = NS + 1;
  float x[NS];
#pragma unroll
  for (int d = 0; d < NS; ++d) x[d] = on ? s[d] : 0.0f;
  double z;
  {
#pragma clang fp contract(off)
    z = affine<NS>(wt.w, x) + wt.tau;
  }
  const double e = exp(-fabs(z));            // in (0, 1]; 0 once |z| > 745: the limits below are then exact
  const double lp = log1p(e);
  const double q = 1.0 / (1.0 + e);          // sigma(|z|); sigma(-|z|) = e q
  const bool pos = z >= 0.0;
  // target: softplus(-z), r = -sigma(-z); non-target: softplus(z), r = sigma(z)
  const double big = target ? fmax(-z, 0.0) : fmax(z, 0.0);
  const double sp = big + lp;
  acc[0] += (on && target) ? sp : 0.0;
  acc[1] += (on && !target) ? sp : 0.0;
  if (!VALUE_ONLY) {
    const double eq = e * q;
    const double r = target ? -(pos ? eq : q) : (pos ? q : eq);
    const double c = on ? (target ? wt.c_tar : wt.c_non) : 0.0;
    const double g = c * r, h = c * (eq * q);
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[2 + i] += g * (double)x[i];
    acc[2 + NS] += g;
    int k = 2 + D;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const double hx = h * (double)x[i];
#pragma unroll
      for (int j = i; j < NS; ++j) acc[k++] += hx * (double)x[j];
      acc[k++] += hx;
    }
    acc[k] += h;
  }
}

// VEC: one 16-byte load per system and one 4-byte label load per whole quad (base pointers and plane_stride allow it); else
// 4-byte and 1-byte loads.  The quad reaching past n always takes the checked loads.  Same values, same order, same bits.
template <int NS, bool VEC, bool VALUE_ONLY>
__global__ __launch_bounds__(RT) void stats_kernel(const float* __restrict__ sc, size_t plane_stride, const uint8_t* __restrict__ lab,
                                                   size_t n, size_t quads, size_t span, const Weights wt, int row_len,
                                                   double* __restrict__ part, unsigned long long* __restrict__ cnt) {
  constexpr int NA = VALUE_ONLY ? 2 : n_out(NS);
  double acc[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) acc[k] = 0.0;
  unsigned n_tar = 0, n_non = 0, n_skip = 0;   // per thread: at most 4 * steps
  const size_t lo = (size_t)blockIdx.x * span, hi = std::min(quads, lo + span);
  for (size_t qd = lo + threadIdx.x; qd < hi; qd += RT) {
    const size_t i0 = 4 * qd;
    float s[4][NS];
    bool tgt[4], in[4];
    if (VEC && i0 + 4 <= n) {
#pragma unroll
      for (int d = 0; d < NS; ++d) {
        const float4 v = *reinterpret_cast<const float4*>(sc + (size_t)d * plane_stride + i0);
        s[0][d] = v.x, s[1][d] = v.y, s[2][d] = v.z, s[3][d] = v.w;
      }
      const uchar4 u = *reinterpret_cast<const uchar4*>(lab + i0);
      tgt[0] = u.x != 0, tgt[1] = u.y != 0, tgt[2] = u.z != 0, tgt[3] = u.w != 0;
      in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        in[e] = i0 + e < n;
        tgt[e] = in[e] ? lab[i0 + e] != 0 : false;
#pragma unroll
        for (int d = 0; d < NS; ++d) s[e][d] = in[e] ? sc[(size_t)d * plane_stride + i0 + e] : 0.0f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool fin = true;
#pragma unroll
      for (int d = 0; d < NS; ++d) fin = fin && finite_f32(s[e][d]);
      const bool on = in[e] && fin;
      n_tar += on && tgt[e];
      n_non += on && !tgt[e];
      n_skip += in[e] && !fin;
      add_trial<NS, VALUE_ONLY>(wt, s[e], tgt[e], on, acc);
    }
  }
  __shared__ double red[WAVES][NA];
  __shared__ long long redc[WAVES][3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NA; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[w][k] = v;
  }
  const long long ct = wave_sum((long long)n_tar), cn = wave_sum((long long)n_non), cs = wave_sum((long long)n_skip);
  if (lane == 0) {
    redc[w][0] = ct;
    redc[w][1] = cn;
    redc[w][2] = cs;
  }
  __syncthreads();
  if ((int)threadIdx.x < NA) {
    double v = 0.0;
    for (int i = 0; i < WAVES; ++i) v += red[i][threadIdx.x];
    part[(size_t)blockIdx.x * row_len + threadIdx.x] = v;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 67) {
    const int k = threadIdx.x - 64;
    long long v = 0;
    for (int i = 0; i < WAVES; ++i) v += redc[i][k];
    cnt[(size_t)blockIdx.x * 3 + k] = (unsigned long long)v;
  }
}

// ONE workgroup of FIN_GROUPS waves adds the rows in index order: wave j the rows [j * per, min(grid, (j + 1) * per)), per =
// ceil(grid / FIN_GROUPS), one after another from 0.0 (lane k the value k, lanes 60 .. 62 the counts); then the FIN_GROUPS sums
// are added in the order j = 0, 1, ...
constexpr int FIN_GROUPS = 16;
__global__ __launch_bounds__(64 * FIN_GROUPS) void finish_kernel(const double* __restrict__ part,
                                                                 const unsigned long long* __restrict__ cnt, unsigned grid,
                                                                 int row_len, int n_val, double* __restrict__ fin,
                                                                 unsigned long long* __restrict__ fcnt) {
  __shared__ double red[FIN_GROUPS][64];
  __shared__ unsigned long long redc[FIN_GROUPS][3];
  const int k = threadIdx.x & 63, j = threadIdx.x >> 6;
  const unsigned per = (grid + FIN_GROUPS - 1) / FIN_GROUPS;
  const unsigned lo = std::min(grid, j * per), hi = std::min(grid, lo + per);
  if (k < n_val) {
    double v = 0.0;
#pragma unroll 8
    for (unsigned g = lo; g < hi; ++g) v += part[(size_t)g * row_len + k];
    red[j][k] = v;
  } else if (k >= 60 && k < 63) {
    unsigned long long v = 0;
#pragma unroll 8
    for (unsigned g = lo; g < hi; ++g) v += cnt[(size_t)g * 3 + (k - 60)];
    redc[j][k - 60] = v;
  }
  __syncthreads();
  if (j == 0 && k < n_val) {
    double v = 0.0;
    for (int i = 0; i < FIN_GROUPS; ++i) v += red[i][k];
    fin[k] = v;
  } else if (j == 0 && k >= 60 && k < 63) {
    unsigned long long v = 0;
    for (int i = 0; i < FIN_GROUPS; ++i) v += redc[i][k - 60];
    fcnt[k - 60] = v;
  }
}
static_assert(n_out(MAX_SYS) <= 60, "finish_kernel: the value lanes run into the count lanes");

using StatsKernel = void (*)(const float*, size_t, const uint8_t*, size_t, size_t, size_t, const Weights, int, double*,
                             unsigned long long*);
template <int NS>
StatsKernel pick_stats(bool vec, bool value_only) {
  return vec ? (value_only ? stats_kernel<NS, true, true> : stats_kernel<NS, true, false>)
             : (value_only ? stats_kernel<NS, false, true> : stats_kernel<NS, false, false>);
}
StatsKernel stats_instance(int ns, bool vec, bool value_only) {
  switch (ns) {
    case 1: return pick_stats<1>(vec, value_only);
    case 2: return pick_stats<2>(vec, value_only);
    case 3: return pick_stats<3>(vec, value_only);
    case 4: return pick_stats<4>(vec, value_only);
    case 5: return pick_stats<5>(vec, value_only);
    case 6: return pick_stats<6>(vec, value_only);
    case 7: return pick_stats<7>(vec, value_only);
    default: return pick_stats<8>(vec, value_only);
  }
}

// d_out[p] = f32(affine(w, s_p)); four consecutive trials per thread.  Every load of a thread precedes its stores, and no other
// thread touches its trials: d_out may be the scores themselves (n_sys == 1).
template <int NS, bool VEC>
__global__ __launch_bounds__(RT) void apply_kernel(const float* sc, size_t plane_stride, size_t n, const Weights wt, float* out) {
  const size_t i0 = 4 * ((size_t)blockIdx.x * RT + threadIdx.x);
  if (i0 >= n) return;
  float s[4][NS], r[4];
  if (VEC && i0 + 4 <= n) {
#pragma unroll
    for (int d = 0; d < NS; ++d) {
      const float4 v = *reinterpret_cast<const float4*>(sc + (size_t)d * plane_stride + i0);
      s[0][d] = v.x, s[1][d] = v.y, s[2][d] = v.z, s[3][d] = v.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)affine<NS>(wt.w, s[e]);
    *reinterpret_cast<float4*>(out + i0) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int d = 0; d < NS; ++d) s[e][d] = i0 + e < n ? sc[(size_t)d * plane_stride + i0 + e] : 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < n) out[i0 + e] = (float)affine<NS>(wt.w, s[e]);
  }
}

using ApplyKernel = void (*)(const float*, size_t, size_t, const Weights, float*);
template <int NS>
ApplyKernel pick_apply(bool vec) { return vec ? apply_kernel<NS, true> : apply_kernel<NS, false>; }
ApplyKernel apply_instance(int ns, bool vec) {
  switch (ns) {
    case 1: return pick_apply<1>(vec);
    case 2: return pick_apply<2>(vec);
    case 3: return pick_apply<3>(vec);
    case 4: return pick_apply<4>(vec);
    case 5: return pick_apply<5>(vec);
    case 6: return pick_apply<6>(vec);
    case 7: return pick_apply<7>(vec);
    default: return pick_apply<8>(vec);
  }
}

bool finite_f64(double v) { return v - v == 0.0; }

// 16-byte loads of every plane: the base and, beyond one plane, the distance between planes
bool planes_vec(const float* d_scores, int n_sys, int64_t plane_stride) {
  return (reinterpret_cast<uintptr_t>(d_scores) & 15) == 0 && (n_sys == 1 || plane_stride % 4 == 0);
}

}  // namespace

extern "C" {

size_t svk_calibration_stats_workspace_bytes(int64_t n, int32_t n_sys) {
  if (n <= 0 || n_sys < 1 || n_sys > MAX_SYS) return 0;
  return stats_layout(stats_geometry((size_t)n), n_sys).total;
}

int svk_calibration_stats(svk_ctx* ctx, const float* d_scores, int32_t n_sys, int64_t plane_stride, const uint8_t* d_labels,
                          int64_t n, const double* h_weights, double tau, const double* h_class_weight, int32_t flags,
                          void* d_workspace, size_t workspace_bytes, double* h_out, int64_t* h_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, h_out && h_count && h_weights && h_class_weight, "NULL host buffer");
  SVK_REQUIRE(ctx, n >= 0, "negative size");
  SVK_REQUIRE(ctx, n_sys >= 1 && n_sys <= MAX_SYS, "1 to 8 systems");
  SVK_REQUIRE(ctx, plane_stride >= n, "plane_stride below n");
  SVK_REQUIRE(ctx, (flags & ~1) == 0, "undefined flag bits");
  Weights wt;
  for (int d = 0; d <= MAX_SYS; ++d) wt.w[d] = d <= n_sys ? h_weights[d] : 0.0;
  wt.tau = tau;
  wt.c_tar = h_class_weight[0];
  wt.c_non = h_class_weight[1];
  for (int d = 0; d <= n_sys; ++d) SVK_REQUIRE(ctx, finite_f64(wt.w[d]), "non-finite weight");
  SVK_REQUIRE(ctx, finite_f64(tau) && finite_f64(wt.c_tar) && finite_f64(wt.c_non), "non-finite tau or class weight");
  const bool value_only = flags & 1;
  const int n_val = value_only ? 2 : n_out(n_sys);
  for (int k = 0; k < n_val; ++k) h_out[k] = 0.0;
  h_count[0] = h_count[1] = h_count[2] = 0;
  if (n == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_scores && d_labels && d_workspace, "NULL buffer");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_scores) & 3) == 0, "scores must be 4-byte aligned");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const Geometry g = stats_geometry((size_t)n);
  const Layout l = stats_layout(g, n_sys);
  SVK_REQUIRE(ctx, workspace_bytes >= l.total, "workspace smaller than svk_calibration_stats_workspace_bytes(n, n_sys)");
  char* w = static_cast<char*>(d_workspace);
  double* part = reinterpret_cast<double*>(w + l.part);
  auto* cnt = reinterpret_cast<unsigned long long*>(w + l.cnt);
  double* fin = reinterpret_cast<double*>(w + l.fin);
  auto* fcnt = reinterpret_cast<unsigned long long*>(w + l.fcnt);
  const bool vec = planes_vec(d_scores, n_sys, plane_stride) && (reinterpret_cast<uintptr_t>(d_labels) & 3) == 0;
  const int row_len = n_out(n_sys);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(stats_instance(n_sys, vec, value_only), dim3(g.grid), dim3(RT), 0, st, d_scores, (size_t)plane_stride,
                     d_labels, (size_t)n, g.quads, g.span, wt, row_len, part, cnt);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64 * FIN_GROUPS), 0, st, part, cnt, g.grid, row_len, n_val, fin, fcnt);
  SVK_LAUNCH_CHECK(ctx);
  unsigned long long hc[3];
  SVK_HIP(ctx, hipMemcpyAsync(h_out, fin, sizeof(double) * (size_t)n_val, hipMemcpyDeviceToHost, st));
  SVK_HIP(ctx, hipMemcpyAsync(hc, fcnt, sizeof(hc), hipMemcpyDeviceToHost, st));
  SVK_HIP(ctx, hipStreamSynchronize(st));
  for (int k = 0; k < 3; ++k) h_count[k] = (int64_t)hc[k];
  return SVK_OK;
}

int svk_calibration_apply(svk_ctx* ctx, const float* d_scores, int32_t n_sys, int64_t plane_stride, int64_t n,
                          const double* h_weights, float* d_out) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, h_weights, "NULL host buffer");
  SVK_REQUIRE(ctx, n >= 0, "negative size");
  SVK_REQUIRE(ctx, n_sys >= 1 && n_sys <= MAX_SYS, "1 to 8 systems");
  SVK_REQUIRE(ctx, plane_stride >= n, "plane_stride below n");
  Weights wt;
  for (int d = 0; d <= MAX_SYS; ++d) wt.w[d] = d <= n_sys ? h_weights[d] : 0.0;
  wt.tau = wt.c_tar = wt.c_non = 0.0;
  for (int d = 0; d <= n_sys; ++d) SVK_REQUIRE(ctx, finite_f64(wt.w[d]), "non-finite weight");
  if (n == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_scores && d_out, "NULL buffer");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_scores) | reinterpret_cast<uintptr_t>(d_out)) & 3) == 0,
              "scores and output must be 4-byte aligned");
  const size_t blocks = (((size_t)n + 3) / 4 + RT - 1) / RT;
  SVK_REQUIRE(ctx, blocks <= 0x7fffffffu, "n beyond 2^41");
  const bool vec = planes_vec(d_scores, n_sys, plane_stride) && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
  hipLaunchKernelGGL(apply_instance(n_sys, vec), dim3((unsigned)blocks), dim3(RT), 0, ctx->stream, d_scores, (size_t)plane_stride,
                     (size_t)n, wt, d_out);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
