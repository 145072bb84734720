// PLDA scoring (two-covariance model in the basis that diagonalises both covariances; plda.py fits it).
//   svk_plda_scores       the log-likelihood ratio of every test row against every enrolled row: a bilinear form plus a term
//       per row and a term per column.  A float64 pre-pass folds the coefficients into the enrolled operand and forms the
//       row / column terms; the product runs on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation), one pass
//       over the output.
//   svk_plda_pair_scores  one LLR per trial of a list, float64 throughout, a team of 16 lanes per trial.
// The leaf helpers of score_common.h are shared with the cosine kernels of scoring.hip / search.hip; the tile loop of the
// product and its K order are this kernel's own, as theirs are theirs: each keeps its bits.
#include <algorithm>

#include "score_common.h"
#include "svk_internal.h"

namespace {

// The coefficients of direction k for an enrolled model of n utterances (svk.h has the formulas):
//   alpha = n psi / d1,  beta = alpha psi / d3,  gamma = alpha n psi / d2,  with d1 = (n + 1) psi + 1, d2 = n psi + 1, d3 = psi + 1
//   half_log = 1/2 log(d1 / (d2 d3)) = 1/2 log1p(-n psi^2 / (d2 d3)): this direction's share of -c(n), accurate for small psi too.
// psi = 0 gives exact zeros.
struct PldaCoef {
  double alpha, beta, gamma, half_log;
};
__device__ __forceinline__ PldaCoef plda_coef(double psi, double n) {
  const double d1 = fma(n + 1.0, psi, 1.0), d2 = fma(n, psi, 1.0), d3 = psi + 1.0;
  const double np = n * psi;
  PldaCoef c;
  c.alpha = np / d1;
  c.beta = c.alpha * psi / d3;
  c.gamma = c.alpha * np / d2;
  c.half_log = 0.5 * log1p(-(np * psi) / (d2 * d3));
  return c;
}

// ---- pre-pass ----------------------------------------------------------------------------------------------------------
// One wave per row; lane l owns the columns l, l + 64, ... in order, the 64 partial sums meet in a butterfly: the order of
// additions depends on dim alone.
//
// Enrolled row j with n = count_j (1 when counts is NULL):  b0[j][k] = f32(alpha_k(n) u_jk),  t[j] = -1/2 sum_k gamma_k(n) u_jk^2
// + c(n);  with counts also  b1[j][k] = f32(-1/2 beta_k(n)).  n < 1: t[j] = NaN (the whole column comes out NaN).
__global__ __launch_bounds__(256) void plda_enroll_prep_kernel(const float* __restrict__ enroll, int ne, int dim,
                                                               const double* __restrict__ psi, const int32_t* __restrict__ counts,
                                                               float* __restrict__ b0, float* __restrict__ b1,
                                                               double* __restrict__ t) {
  const int lane = threadIdx.x & 63;
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < ne; j += (int64_t)gridDim.x * 4) {
    const int cnt = counts ? counts[j] : 1;
    const double n = cnt >= 1 ? (double)cnt : 1.0;
    const float* u = enroll + j * dim;
    double acc = 0.0;
    for (int k = lane; k < dim; k += 64) {
      const PldaCoef c = plda_coef(psi[k], n);
      const double x = (double)u[k];
      b0[j * dim + k] = (float)(c.alpha * x);
      if (b1) b1[j * dim + k] = (float)(-0.5 * c.beta);
      acc += -0.5 * (c.gamma * x * x) - c.half_log;
    }
    acc = wave_sum(acc);
    if (lane == 0) t[j] = cnt >= 1 ? acc : __builtin_nan("");
  }
}

// Test row i.  counts NULL:  s[i] = -1/2 sum_k beta_k(1) v_ik^2;  counts given:  a1[i][k] = f32(v_ik^2), s[i] = 0.
__global__ __launch_bounds__(256) void plda_test_prep_kernel(const float* __restrict__ test, int nt, int dim,
                                                             const double* __restrict__ psi, float* __restrict__ a1,
                                                             double* __restrict__ s) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nt; i += (int64_t)gridDim.x * 4) {
    const float* v = test + i * dim;
    double acc = 0.0;
    for (int k = lane; k < dim; k += 64) {
      const float x = v[k];
      if (a1) {
        a1[i * dim + k] = x * x;
      } else {
        const PldaCoef c = plda_coef(psi[k], 1.0);
        acc += -0.5 * (c.beta * ((double)x * (double)x));
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) s[i] = acc;
  }
}

// ---- product -----------------------------------------------------------------------------------------------------------
// out[i][j] = f32( (double) sum_k a_ik b_jk + s_i + t_j ),  k over one segment (a0 . b0, K = dim) or two (then a1 . b1, K = 2 dim).
// A workgroup owns 128 test rows (each of its 4 waves 32 of them: two 16-row tiles) and a span of 32-column blocks of the
// enrolled operand.  A 32 x 128 block of b is staged in LDS (rows padded to 136 floats: the ds_read_b128 of the fragments are
// conflict-free), double-buffered: the next block's global loads are issued before the MFMAs of the current one and written to
// the other buffer after them.  Fragments: lane (i = l & 15, g = l >> 4) holds floats [16 u + 4 g, +4) of row i, MFMA (u, e) uses
// element e of both operands: the order of k is the steps (segment, 128-block) in order, inside a step u = 0 .. 7, e = 0 .. 3, and
// inside one MFMA g = 0 .. 3 -- fixed by dim and the number of segments.  Columns past dim and rows past either matrix enter as
// zeros on BOTH sides (0 x 0 adds exactly nothing, and a NaN elsewhere never meets them).  The split is over output rows and
// columns, never over K: no reduction, and the bits of a score do not depend on where its rows lie or on the grid.
// HOIST (one step in all: one segment, dim <= 128): the test fragments stay in registers for the whole workgroup.
constexpr int PT_BM = 128, PT_BN = 32, PT_KB = 128, PT_LD = PT_KB + 8;

template <bool HOIST>
__global__ __launch_bounds__(256) void plda_product_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                           const float* __restrict__ b0, const float* __restrict__ b1,
                                                           const double* __restrict__ s, const double* __restrict__ t, int nt,
                                                           int ne, int dim, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float bs[2][PT_BN * PT_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int nkb = (dim + PT_KB - 1) / PT_KB;
  const int nsteps = (a1 ? 2 : 1) * nkb;
  const bool vec_b = (dim & 3) == 0;   // the workspace operands: sections are 256-byte aligned, rows 4 dim bytes apart
  const bool vec_a0 = vec_b && (reinterpret_cast<uintptr_t>(a0) & 15) == 0;
  const int n_cblocks = (int)(((int64_t)ne + PT_BN - 1) / PT_BN);
  const int cb_begin = (int)((long long)n_cblocks * blockIdx.y / gridDim.y);
  const int cb_end = (int)((long long)n_cblocks * (blockIdx.y + 1) / gridDim.y);
  if (cb_begin >= cb_end) return;   // workgroup-uniform
  const int64_t m0 = (int64_t)blockIdx.x * PT_BM + wave * 32;

  // staging assignment: thread x moves 4 float4 of the 32 x 128 block: row (x >> 5) + 8 j, floats [4 (x & 31), +4)
  const int srow = threadIdx.x >> 5, scol = (threadIdx.x & 31) * 4;
  auto fetch = [&](int cb, int step, f32x4 (&regs)[4]) {
    const float* b = step < nkb ? b0 : b1;
    const int kb = step < nkb ? step : step - nkb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = (int64_t)cb * PT_BN + srow + 8 * j;
      regs[j] = load4(b + r * dim, kb * PT_KB + scol, dim, r < ne, vec_b);
    }
  };
  auto stash = [&](float* buf, const f32x4 (&regs)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(buf + (srow + 8 * j) * PT_LD + scol) = regs[j];
  };
  auto a_frag = [&](int rt, int step, int u) {
    const bool first = step < nkb;
    const int kb = first ? step : step - nkb;
    const int64_t row = m0 + 16 * rt + i;
    return load4((first ? a0 : a1) + row * dim, kb * PT_KB + 16 * u + 4 * g, dim, row < nt, first ? vec_a0 : vec_b);
  };

  f32x4 ah[2][8];
  if (HOIST) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int u = 0; u < 8; ++u) ah[rt][u] = a_frag(rt, 0, u);
  }
  // the row terms of the eight output rows this lane writes (row 16 rt + 4 g + r of the wave's 32)
  double srow_term[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = m0 + 16 * rt + 4 * g + r;
      srow_term[rt][r] = row < nt ? s[row] : 0.0;
    }

  f32x4 pre[4];
  fetch(cb_begin, 0, pre);
  stash(bs[0], pre);
  __syncthreads();
  int cur = 0;
  for (int cb = cb_begin; cb < cb_end; ++cb) {
    f32x4 acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // this lane's two output columns: their term is needed after the MFMAs, load it now
    double tcol[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int64_t col = (int64_t)cb * PT_BN + 16 * ct + i;
      tcol[ct] = col < ne ? t[col] : 0.0;
    }
    for (int step = 0; step < nsteps; ++step) {
      const bool last = step + 1 == nsteps;
      const int ncb = last ? cb + 1 : cb, nstep = last ? 0 : step + 1;
      const bool more = ncb < cb_end;   // workgroup-uniform
      if (more) fetch(ncb, nstep, pre);
      const float* b = bs[cur];
      const int kb = step < nkb ? step : step - nkb;
      const int klen = min(PT_KB, dim - kb * PT_KB);   // floats of this step that lie inside the rows
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (16 * u < klen) {   // workgroup-uniform: chunks wholly past dim hold zeros on both sides, skip their MFMAs
          f32x4 av[2];
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) av[rt] = HOIST ? ah[rt][u] : a_frag(rt, step, u);
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(b + (16 * ct + i) * PT_LD + 16 * u + 4 * g);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][0], bv[0], acc[rt][ct], 0, 0, 0);
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][1], bv[1], acc[rt][ct], 0, 0, 0);
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][2], bv[2], acc[rt][ct], 0, 0, 0);
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][3], bv[3], acc[rt][ct], 0, 0, 0);
            }
          }
        }
      }
      if (more) stash(bs[cur ^ 1], pre);
      __syncthreads();   // everyone is done with bs[cur]; bs[cur ^ 1] is complete
      cur ^= 1;
    }
    // acc[rt][ct][r] = dot(test row m0 + 16 rt + 4 g + r, enrolled row 32 cb + 16 ct + i); one rounding to f32
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int64_t col = (int64_t)cb * PT_BN + 16 * ct + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = m0 + 16 * rt + 4 * g + r;
          if (row < nt && col < ne) out[row * ne + col] = (float)(((double)acc[rt][ct][r] + srow_term[rt][r]) + tcol[ct]);
        }
      }
  }
}

// ---- svk_plda_pair_scores ------------------------------------------------------------------------------------------------
// A team of 16 lanes owns one trial; lane x of it owns the columns 4 (x + 16 k) .. + 3 of both rows, k = 0, 1, ...  Each lane
// adds the terms of its columns in order in float64, the team's partial sums meet in a four-step butterfly: the order of
// additions depends on dim alone.  VEC4 (dim % 4 == 0, both matrices 16-byte aligned) and the scalar loads fill the same registers.
constexpr int PP_TEAM = 16, PP_THREADS = 256, PP_PER_WG = PP_THREADS / PP_TEAM;

template <bool VEC4>
__global__ __launch_bounds__(PP_THREADS) void plda_pair_kernel(const float* __restrict__ a, int64_t n_a, const float* __restrict__ b,
                                                               int64_t n_b, int dim, const double* __restrict__ psi,
                                                               const int32_t* __restrict__ count_b,
                                                               const int64_t* __restrict__ idx_a, const int64_t* __restrict__ idx_b,
                                                               int64_t n_pairs, float* __restrict__ out,
                                                               int32_t* __restrict__ bad_count) {
  const int x = threadIdx.x & (PP_TEAM - 1);
  for (int64_t p = (int64_t)blockIdx.x * PP_PER_WG + (threadIdx.x / PP_TEAM); p < n_pairs;
       p += (int64_t)gridDim.x * PP_PER_WG) {   // (whole teams leave: the butterfly stays inside a team)
    const int64_t ia = idx_a[p], ib = idx_b[p];
    if ((uint64_t)ia >= (uint64_t)n_a || (uint64_t)ib >= (uint64_t)n_b) {   // the caller's error: not followed
      if (x == 0) {
        out[p] = __builtin_nanf("");
        if (bad_count) atomicAdd(bad_count, 1);
      }
      continue;
    }
    const int cnt = count_b ? count_b[ib] : 1;
    const double n = cnt >= 1 ? (double)cnt : 1.0;
    const float* rv = a + ia * dim;   // the test side
    const float* ru = b + ib * dim;   // the enrolled side
    double sum = 0.0;
    for (int col = 4 * x; col < dim; col += 4 * PP_TEAM) {
      float v[4], u[4];
      if constexpr (VEC4) {
        const f32x4 vv = *reinterpret_cast<const f32x4*>(rv + col), vu = *reinterpret_cast<const f32x4*>(ru + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = vv[e], u[e] = vu[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = col + e < dim ? rv[col + e] : 0.f;
          u[e] = col + e < dim ? ru[col + e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (col + e < dim) {
          const PldaCoef c = plda_coef(psi[col + e], n);
          const double dv = (double)v[e], du = (double)u[e];
          sum += (c.alpha * du * dv - 0.5 * (c.beta * (dv * dv)) - 0.5 * (c.gamma * (du * du))) - c.half_log;
        }
      }
    }
#pragma unroll
    for (int m = PP_TEAM / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (x == 0) out[p] = cnt >= 1 ? (float)sum : __builtin_nanf("");
  }
}

constexpr size_t PLDA_ALIGN = 256;
inline size_t plda_round(size_t bytes) { return (bytes + PLDA_ALIGN - 1) & ~(PLDA_ALIGN - 1); }

}  // namespace

extern "C" {

size_t svk_plda_scores_workspace_bytes(int32_t n_test, int32_t n_enroll, int32_t dim, int32_t with_counts) {
  if (n_test <= 0 || n_enroll <= 0 || dim < 1 || dim > 512) return 0;
  const size_t row_t = plda_round(sizeof(float) * (size_t)n_test * dim), row_e = plda_round(sizeof(float) * (size_t)n_enroll * dim);
  size_t bytes = plda_round(sizeof(double) * (size_t)n_enroll) + plda_round(sizeof(double) * (size_t)n_test) + row_e;
  if (with_counts) bytes += row_e + row_t;
  return bytes;
}

int svk_plda_scores(svk_ctx* ctx, const float* d_test, int32_t n_test, const float* d_enroll, int32_t n_enroll, int32_t dim,
                    const double* d_psi, const int32_t* d_enroll_count, void* d_workspace, size_t workspace_bytes,
                    float* d_out) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_test >= 0 && n_enroll >= 0, "negative shape");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= 512, "dim must be in [1, 512]");
  if (n_test == 0 || n_enroll == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_test && d_enroll && d_psi && d_workspace && d_out, "NULL buffer");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_test) | reinterpret_cast<uintptr_t>(d_enroll) | reinterpret_cast<uintptr_t>(d_out) |
                     reinterpret_cast<uintptr_t>(d_enroll_count)) & 3) == 0, "rows, counts and scores must be 4-byte aligned");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_psi) & 7) == 0, "psi must be 8-byte aligned");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "the workspace must be 16-byte aligned");
  const bool with_counts = d_enroll_count != nullptr;
  SVK_REQUIRE(ctx, workspace_bytes >= svk_plda_scores_workspace_bytes(n_test, n_enroll, dim, with_counts),
              "the workspace is smaller than svk_plda_scores_workspace_bytes");
  // the workspace, by section (each a multiple of 256 bytes): t, s, b0[, b1, a1]
  char* w = static_cast<char*>(d_workspace);
  const size_t row_e = plda_round(sizeof(float) * (size_t)n_enroll * dim);
  double* t = reinterpret_cast<double*>(w);
  w += plda_round(sizeof(double) * (size_t)n_enroll);
  double* s = reinterpret_cast<double*>(w);
  w += plda_round(sizeof(double) * (size_t)n_test);
  float* b0 = reinterpret_cast<float*>(w);
  w += row_e;
  float* b1 = with_counts ? reinterpret_cast<float*>(w) : nullptr;
  float* a1 = with_counts ? reinterpret_cast<float*>(w + row_e) : nullptr;

  const int max_wg = ctx->num_cu * 8;
  hipLaunchKernelGGL(plda_enroll_prep_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)n_enroll + 3) / 4, max_wg)), dim3(256), 0, ctx->stream,
                     d_enroll, n_enroll, (int)dim, d_psi, d_enroll_count, b0, b1, t);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(plda_test_prep_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)n_test + 3) / 4, max_wg)), dim3(256), 0, ctx->stream, d_test,
                     n_test, (int)dim, d_psi, a1, s);
  SVK_LAUNCH_CHECK(ctx);
  // rows x column spans: enough workgroups for a few per resident slot where the shape has them
  const int row_blocks = (int)(((int64_t)n_test + PT_BM - 1) / PT_BM), col_blocks = (int)(((int64_t)n_enroll + PT_BN - 1) / PT_BN);
  const int want = ctx->num_cu * 8;
  const int spans = std::max(1, std::min(std::min(col_blocks, 65535), (want + row_blocks - 1) / row_blocks));
  const bool hoist = !with_counts && dim <= PT_KB;
  auto kern = hoist ? plda_product_kernel<true> : plda_product_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)row_blocks, (unsigned)spans), dim3(256), 0, ctx->stream, d_test,
                     static_cast<const float*>(a1), static_cast<const float*>(b0), static_cast<const float*>(b1),
                     static_cast<const double*>(s), static_cast<const double*>(t), (int)n_test, (int)n_enroll, (int)dim, d_out);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_plda_pair_scores(svk_ctx* ctx, const float* d_a, int64_t n_a, const float* d_b, int64_t n_b, int32_t dim,
                         const double* d_psi, const int32_t* d_count_b, const int64_t* d_idx_a, const int64_t* d_idx_b,
                         int64_t n_pairs, float* d_out, int32_t* d_bad_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_a >= 0 && n_b >= 0 && n_pairs >= 0, "negative shape");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= 512, "dim must be in [1, 512]");
  if (n_pairs == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_a && d_b && d_psi && d_idx_a && d_idx_b && d_out, "NULL buffer");
  const uintptr_t both = reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b);
  SVK_REQUIRE(ctx, ((both | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_count_b) |
                     reinterpret_cast<uintptr_t>(d_bad_count)) & 3) == 0, "rows, counts and scores must be 4-byte aligned");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_psi) | reinterpret_cast<uintptr_t>(d_idx_a) | reinterpret_cast<uintptr_t>(d_idx_b)) & 7) == 0,
              "psi and the indices must be 8-byte aligned");
  const bool vec4 = dim % 4 == 0 && (both & 15) == 0;
  const unsigned grid = (unsigned)std::min<int64_t>((n_pairs + PP_PER_WG - 1) / PP_PER_WG, (int64_t)ctx->num_cu * 8);
  auto kern = vec4 ? plda_pair_kernel<true> : plda_pair_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(PP_THREADS), 0, ctx->stream, d_a, n_a, d_b, n_b, (int)dim, d_psi, d_count_b, d_idx_a,
                     d_idx_b, n_pairs, d_out, d_bad_count);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
