// The embedding back end: what stands between the network's FC5 rows and the cosine scorer.
//
// svk_class_scatter -- the statistics a back end is fitted on: the float64 mean of every class (speaker) and the within-class
// scatter S_w = sum_c sum_{i in c} (x_i - m_c)(x_i - m_c)^T, two-pass, float64, on v_mfma_f64_16x16x4_f64 with the rows as K.
//   1. row_norm_kernel (flag bit 0 only): ||x|| of every row in float64, one team of 16 lanes per row -> workspace.  Both later
//      passes divide by THESE bits, so a one-row class centres to exactly zero.
//   2. class_mean_kernel: one workgroup per class, one thread per column, the class's rows added in order inside blocks of 64
//      rows and the blocks' sums in order (svk_embedding_pool's order): a mean depends on its own class alone.
//   3. eff_scan_kernel: classes of fewer than two rows contribute exactly zero and are left out; the others' row counts are
//      prefix-summed into the EFFECTIVE row sequence.  That sequence is cut into chunks of chunk_rows(dim) rows -- a function
//      of dim, not of the launch -- so adding or removing an empty or one-row class moves no chunk boundary.
//   4. scatter_kernel: one workgroup per (chunk, group of 36 upper-triangle 16 x 16 tiles).  The centred rows d = x/||x|| - m
//      are staged through LDS as float64, KC rows at a time (the next stage's loads are in flight while this one multiplies);
//      a wave reads each operand pair once per tile and K-step of 4 rows and chains the MFMAs of a tile in row order.  Rows
//      past the chunk's end and columns past dim are zeros: x + 0 = x, the padding changes no bit.
//   5. scatter_reduce_kernel: the chunks' partial tiles added in chunk order; a tile above the diagonal is written to both
//      halves and a diagonal tile from its upper triangle, so d_sw is symmetric bit for bit.
// No floating-point atomic anywhere; nothing depends on a counter or on which workgroup finishes first.
//
// svk_embedding_project -- y = l2(( l2(x) - mu ) W) in one trip through HBM.  A wave owns 16 rows and every output tile.  Lane l
// = (row l & 15, group g = l >> 4) owns the quads x[row][16 S + 4 g .. + 3] of its row, S = 0 .. : exactly the A fragments of
// v_mfma_f32_16x16x4_f32 when step e of super-step S multiplies k = 16 S + 4 g + e.  So no element of x is touched by two
// lanes: the lane that needs it normalises and centres it.  The row norm is each lane's float64 sum over its quads in order,
// then a butterfly over the four groups.  W goes through LDS sixteen k at a time, zero-padded; the products of column j run
// over k in the order (S, e, g), fixed by dim.  16-byte loads of x and mu when dim % 4 == 0 and both are 16-byte aligned, four
// guarded 4-byte loads otherwise: the same registers either way.
#include "svk_internal.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ class scatter
constexpr int SC_THREADS = 256;
constexpr int SC_TILES_PER_WAVE = 9;                         // 4 waves x 9 = the 36 upper tiles of dim 128
constexpr int SC_TILES_PER_GROUP = 4 * SC_TILES_PER_WAVE;
constexpr int SC_ROW_BLOCK = 64;                             // the mean's block of rows (pool.hip's)

inline int sc_blocks16(int dim) { return (dim + 15) / 16; }
inline int sc_tiles(int dim) { return sc_blocks16(dim) * (sc_blocks16(dim) + 1) / 2; }
// rows of the effective sequence per partial matrix: a function of dim alone (it is part of what fixes the bits)
inline int64_t sc_chunk_rows(int dim) { return 4 * (int64_t)std::max(16 * sc_blocks16(dim), 128); }

struct ScatterParams {
  const float* emb;
  int64_t n_rows, n_class;
  int32_t dim, flags;
  const int64_t* seg_start;
  const int64_t* row_index;
  const double* norms;     // [n_rows], valid under flag bit 0
  int64_t* eff;            // [n_class + 1]
  double* partial;         // [chunks][tiles][256]
  int64_t chunk_rows, chunks;
  double* class_mean;
  double* sw;
};

__device__ __forceinline__ void class_range(const ScatterParams& p, int64_t c, int64_t& lo, int64_t& hi) {
  // offsets outside [0, n_rows] or out of order are the caller's error; clamped, so that nothing outside the buffers is read
  lo = std::min<int64_t>(std::max<int64_t>(p.seg_start[c], 0), p.n_rows);
  hi = std::min<int64_t>(std::max<int64_t>(p.seg_start[c + 1], lo), p.n_rows);
}

// the value a row contributes at one column: x, or x / ||x|| (a zero row as zeros; a NaN norm divides)
__device__ __forceinline__ double entered(float x, double nrm, bool l2) {
  return l2 ? (nrm == 0.0 ? 0.0 : (double)x / nrm) : (double)x;
}

__global__ __launch_bounds__(256) void row_norm_kernel(const float* emb, int64_t n_rows, int dim, double* norms) {
  const int t = threadIdx.x & 15;
  const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  double ss = 0.0;
  if (r < n_rows)
    for (int col = t; col < dim; col += 16) {
      const double v = (double)emb[r * dim + col];
      ss += v * v;
    }
  for (int m = 8; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
  if (r < n_rows && t == 0) norms[r] = sqrt(ss);
}

__global__ __launch_bounds__(128) void class_mean_kernel(const ScatterParams p) {
  const int64_t c = blockIdx.x;
  int64_t lo, hi;
  class_range(p, c, lo, hi);
  const bool l2 = p.flags & 1;
  for (int col = threadIdx.x; col < p.dim; col += 128) {
    double acc = 0.0;
    for (int64_t b = lo; b < hi; b += SC_ROW_BLOCK) {
      const int64_t be = std::min<int64_t>(hi, b + SC_ROW_BLOCK);
      double part = 0.0;
      for (int64_t i = b; i < be; ++i) {
        const int64_t r = p.row_index ? p.row_index[i] : i;
        // a row index outside [0, n_rows) (the caller's error) is not followed: the row reads as NaN
        const bool ok = (uint64_t)r < (uint64_t)p.n_rows;
        part += ok ? entered(p.emb[r * p.dim + col], l2 ? p.norms[r] : 1.0, l2) : (double)__builtin_nanf("");
      }
      acc += part;
    }
    p.class_mean[c * p.dim + col] = hi > lo ? acc / (double)(hi - lo) : 0.0;
  }
}

__global__ __launch_bounds__(1024) void eff_scan_kernel(const ScatterParams p) {
  __shared__ int64_t s[1024];
  __shared__ int64_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) {
    carry = 0;
    p.eff[0] = 0;
  }
  __syncthreads();
  for (int64_t base = 0; base < p.n_class; base += 1024) {
    const int64_t c = base + tid;
    int64_t cnt = 0;
    if (c < p.n_class) {
      int64_t lo, hi;
      class_range(p, c, lo, hi);
      cnt = hi - lo >= 2 ? hi - lo : 0;
    }
    s[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int64_t add = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    if (c < p.n_class) p.eff[c + 1] = carry + s[tid];
    __syncthreads();
    if (tid == 1023) carry += s[1023];
    __syncthreads();
  }
}

// NQ: 16-column blocks a row can have (8: dim <= 128, 32: dim <= 512).  KC rows per stage.
template <int NQ>
__global__ __launch_bounds__(SC_THREADS) void scatter_kernel(const ScatterParams p) {
  constexpr int KC = NQ == 8 ? 16 : 8;
  constexpr int CGS = SC_THREADS / KC;          // threads along a staged row
  constexpr int NPT = 16 * NQ / CGS;            // columns per thread of a staged row
  extern __shared__ double sd[];                // [KC][ldp]
  const int dim = p.dim, nb = (dim + 15) / 16, ldp = 16 * nb + 2, n_tiles = nb * (nb + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t total = p.eff[p.n_class];
  const int64_t chunk = blockIdx.x, chunk_lo = chunk * p.chunk_rows;
  if (chunk_lo >= total) return;                // (the whole workgroup: before any barrier)
  const int64_t chunk_hi = std::min<int64_t>(chunk_lo + p.chunk_rows, total);
  const bool l2 = p.flags & 1;

  // this wave's tiles: ids group * 36 + 4 j + wave of the upper triangle, row-major
  int ta[SC_TILES_PER_WAVE], tb[SC_TILES_PER_WAVE];
  bool live[SC_TILES_PER_WAVE];
#pragma unroll
  for (int j = 0; j < SC_TILES_PER_WAVE; ++j) {
    int id = (int)blockIdx.y * SC_TILES_PER_GROUP + 4 * j + wave;
    live[j] = id < n_tiles;
    int a = 0;
    if (live[j])
      while (id >= nb - a) id -= nb - a, ++a;
    ta[j] = live[j] ? a : 0;
    tb[j] = live[j] ? a + id : 0;
  }
  d4 acc[SC_TILES_PER_WAVE];
#pragma unroll
  for (int j = 0; j < SC_TILES_PER_WAVE; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};

  // staging: thread = (row slot rs, column group cg); it walks the classes as its position advances by KC per stage
  const int rs = tid / CGS, cg = tid % CGS;
  int64_t pos = chunk_lo + rs, cls = 0, e0 = 0, e1 = 0, c_lo = 0;
  if (pos < chunk_hi) {
    int64_t lo = 0, hi = p.n_class;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (p.eff[mid + 1] <= pos) lo = mid + 1; else hi = mid;
    }
    cls = lo, e0 = p.eff[cls], e1 = p.eff[cls + 1];
    int64_t h;
    class_range(p, cls, c_lo, h);
  }
  float x[NPT];
  double m[NPT], nrm = 1.0;
  bool have = false, ok = false;
  auto fetch = [&]() {
    have = pos < chunk_hi;
    if (!have) return;
    if (pos >= e1) {
      do {
        ++cls, e0 = e1, e1 = p.eff[cls + 1];
      } while (pos >= e1);
      int64_t h;
      class_range(p, cls, c_lo, h);
    }
    const int64_t i = c_lo + (pos - e0);
    const int64_t r = p.row_index ? p.row_index[i] : i;
    ok = (uint64_t)r < (uint64_t)p.n_rows;
    const float* src = p.emb + (ok ? r : 0) * dim;
    const double* mean = p.class_mean + cls * dim;
    nrm = l2 && ok ? p.norms[r] : 1.0;
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
      const int col = cg + CGS * q;
      x[q] = col < dim ? src[col] : 0.f;
      m[q] = col < dim ? mean[col] : 0.0;
    }
  };
  fetch();
  for (int64_t base = chunk_lo; base < chunk_hi; base += KC) {
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
      const int col = cg + CGS * q;
      double d = 0.0;
      if (have && col < dim) d = (ok ? entered(x[q], nrm, l2) : (double)__builtin_nanf("")) - m[q];
      if (col < 16 * nb) sd[rs * ldp + col] = d;
    }
    __syncthreads();
    pos += KC;
    fetch();                                    // the next stage's loads fly while this one multiplies
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const double* rowp = sd + (4 * ks + (lane >> 4)) * ldp + (lane & 15);
#pragma unroll
      for (int j = 0; j < SC_TILES_PER_WAVE; ++j)
        if (live[j]) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(rowp[16 * ta[j]], rowp[16 * tb[j]], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg -> element 16 row + col = 64 reg + lane
#pragma unroll
  for (int j = 0; j < SC_TILES_PER_WAVE; ++j)
    if (live[j]) {
      const int id = (int)blockIdx.y * SC_TILES_PER_GROUP + 4 * j + wave;
      double* dst = p.partial + (chunk * n_tiles + id) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[64 * r + lane] = acc[j][r];
    }
}

__global__ __launch_bounds__(256) void scatter_reduce_kernel(const ScatterParams p) {
  const int dim = p.dim, nb = (dim + 15) / 16, n_tiles = nb * (nb + 1) / 2;
  int id = blockIdx.x, a = 0;
  while (id >= nb - a) id -= nb - a, ++a;
  const int ta = a, tb = a + id;
  const int64_t total = p.eff[p.n_class];
  const int64_t chunks = std::min<int64_t>((total + p.chunk_rows - 1) / p.chunk_rows, p.chunks);
  const int e = threadIdx.x, i = e >> 4, j = e & 15;
  double s = 0.0;
  for (int64_t k = 0; k < chunks; ++k) s += p.partial[(k * n_tiles + blockIdx.x) * 256 + e];
  const int ra = 16 * ta + i, cb = 16 * tb + j;
  if (ra < dim && cb < dim && (ta < tb || i <= j)) {
    p.sw[(int64_t)ra * dim + cb] = s;
    p.sw[(int64_t)cb * dim + ra] = s;
  }
}

// ------------------------------------------------------------------------------------------------ projection
constexpr int PJ_THREADS = 256;
constexpr int PJ_ROWS = 16 * (PJ_THREADS / 64);   // rows per workgroup
constexpr int PJ_MAX_OUT = 512;

struct ProjectParams {
  const float* emb;
  int64_t n_rows;
  int32_t dim, out_dim, flags;
  const float* mean;
  const float* w;
  float* out;
};

template <bool VEC4>
__device__ __forceinline__ void load_quad(const float* src, int k, int dim, float (&v)[4]) {
  if constexpr (VEC4) {
    const f4 q = k < dim ? *reinterpret_cast<const f4*>(src + k) : f4{0.f, 0.f, 0.f, 0.f};
    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < dim ? src[k + e] : 0.f;
  }
}

// NT: the 16-column output tiles of a wave, a power of two >= out_dim / 16.  Every instance runs all NT tiles of a K-step
// unconditionally (W is zero-padded to 16 NT columns in LDS; a tile skipped under a run-time test costs the compiler > 256
// registers): at most twice the products out_dim needs, and the padded columns are zeros that change no sum
template <int NT, bool VEC4>
__global__ __launch_bounds__(PJ_THREADS) void embedding_project_kernel(const ProjectParams p) {
  __shared__ float ws[16 * (16 * NT + 4)];
  const int dim = p.dim, out_dim = p.out_dim, steps = (dim + 15) / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int64_t row = (int64_t)blockIdx.x * PJ_ROWS + 16 * wave + (lane & 15);
  const bool row_ok = row < p.n_rows;
  const float* src = p.emb + (row_ok ? row : 0) * dim;

  // bit 0: ||x|| in float64 -- this lane's quads in order, then the four groups of the row
  double nrm = 1.0;
  if (p.flags & 1) {
    double ss = 0.0;
#pragma unroll 1
    for (int S = 0; S < steps; ++S) {
      float v[4];
      load_quad<VEC4>(src, 16 * S + 4 * g, row_ok ? dim : 0, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (double)v[e] * (double)v[e];
    }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    nrm = sqrt(ss);
  }
  // c = x' - mu for the quad of super-step S (zeros past dim and for the rows past n_rows)
  auto centred = [&](int S, float (&c)[4]) {
    const int k = 16 * S + 4 * g;
    float v[4], mu[4] = {0.f, 0.f, 0.f, 0.f};
    load_quad<VEC4>(src, k, row_ok ? dim : 0, v);
    if (p.mean) load_quad<VEC4>(p.mean, k, dim, mu);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xn = (p.flags & 1) ? (nrm == 0.0 ? 0.f : (float)((double)v[e] / nrm)) : v[e];
      c[e] = k + e < dim && row_ok ? xn - mu[e] : 0.f;
    }
  };

  if (!p.w) {
    // identity: y = c, no matrix pipe.  bit 1: sum of squares in this lane's order, then the four groups
    double on = 1.0;
    if (p.flags & 2) {
      double ss = 0.0;
#pragma unroll 1
    for (int S = 0; S < steps; ++S) {
        float c[4];
        centred(S, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += (double)c[e] * (double)c[e];
      }
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      on = sqrt(ss);
      if (on == 0.0) on = 1.0;
    }
#pragma unroll 1
    for (int S = 0; S < steps; ++S) {
      float c[4];
      centred(S, c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 16 * S + 4 * g + e;
        if (row_ok && k < dim) p.out[row * dim + k] = (p.flags & 2) ? (float)((double)c[e] / on) : c[e];
      }
    }
    return;
  }

  constexpr int LDW = 16 * NT + 4;
  constexpr int OUTP = 16 * NT;
  f4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int S = 0; S < steps; ++S) {
    float c[4];
    centred(S, c);
    __syncthreads();                            // the previous super-step's reads of ws are done
    for (int idx = tid; idx < 16 * OUTP; idx += PJ_THREADS) {
      const int kk = idx / OUTP, j = idx % OUTP, k = 16 * S + kk;
      ws[kk * LDW + j] = k < dim && j < out_dim ? p.w[(int64_t)k * out_dim + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* wrow = ws + (4 * g + e) * LDW + (lane & 15);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c[e], wrow[16 * t], acc[t], 0, 0, 0);
    }
  }
  // C/D: col = lane & 15, row = 4 (lane >> 4) + reg.  bit 1: the row's sum of squares, this lane's tiles in order, then the
  // row's sixteen lanes (the padded tiles add zeros)
  double on[4] = {1.0, 1.0, 1.0, 1.0};
  if (p.flags & 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double ss = 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) ss += (double)acc[t][r] * (double)acc[t][r];
      for (int msk = 8; msk >= 1; msk >>= 1) ss += __shfl_xor(ss, msk, 64);
      on[r] = sqrt(ss);
      if (on[r] == 0.0) on[r] = 1.0;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t orow = (int64_t)blockIdx.x * PJ_ROWS + 16 * wave + 4 * g + r;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = 16 * t + (lane & 15);
      if (orow < p.n_rows && col < out_dim)
        p.out[orow * out_dim + col] = (p.flags & 2) ? (float)((double)acc[t][r] / on[r]) : acc[t][r];
    }
  }
}

}  // namespace

extern "C" {

size_t svk_class_scatter_workspace_bytes(int64_t n_rows, int32_t dim, int64_t n_class) {
  if (n_rows < 0 || n_class <= 0 || dim < 1 || dim > 512) return 0;
  const int64_t chunk = sc_chunk_rows(dim), chunks = (n_rows + chunk - 1) / chunk;
  const size_t bytes = 8 * (size_t)n_rows + 8 * (size_t)(n_class + 1) + (size_t)chunks * sc_tiles(dim) * 256 * 8;
  return (bytes + 15) & ~(size_t)15;
}

int svk_class_scatter(svk_ctx* ctx, const float* d_emb, int64_t n_rows, int32_t dim, const int64_t* d_seg_start,
                      const int64_t* d_row_index, int64_t n_class, int32_t flags, void* d_workspace, size_t workspace_bytes,
                      double* d_class_mean, double* d_sw) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, (flags & ~1) == 0, "flags: bit 0 (L2-normalise rows) is defined");
  SVK_REQUIRE(ctx, n_rows >= 0 && n_class >= 0, "negative shape");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= 512, "dim must be in [1, 512]");
  SVK_REQUIRE(ctx, d_sw, "NULL buffer");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_sw) & 7) == 0, "d_sw must be 8-byte aligned");
  if (n_class == 0) {
    SVK_HIP(ctx, hipMemsetAsync(d_sw, 0, sizeof(double) * dim * dim, ctx->stream));
    return SVK_OK;
  }
  SVK_REQUIRE(ctx, d_seg_start && d_class_mean && d_workspace && (d_emb || n_rows == 0), "NULL buffer");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_emb) & 3) == 0, "rows must be 4-byte aligned");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_seg_start) | reinterpret_cast<uintptr_t>(d_row_index) |
                     reinterpret_cast<uintptr_t>(d_class_mean)) & 7) == 0, "offsets, indices and means must be 8-byte aligned");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "the workspace must be 16-byte aligned");
  SVK_REQUIRE(ctx, workspace_bytes >= svk_class_scatter_workspace_bytes(n_rows, dim, n_class), "the workspace is too small");
  SVK_REQUIRE(ctx, n_class < ((int64_t)1 << 31) && n_rows / 16 < ((int64_t)1 << 31) - 1, "too many classes or rows for one launch");

  ScatterParams p{};
  p.emb = d_emb, p.n_rows = n_rows, p.n_class = n_class, p.dim = dim, p.flags = flags;
  p.seg_start = d_seg_start, p.row_index = d_row_index;
  double* norms = static_cast<double*>(d_workspace);
  p.norms = norms;
  p.eff = reinterpret_cast<int64_t*>(norms + n_rows);
  p.partial = reinterpret_cast<double*>(p.eff + n_class + 1);
  p.chunk_rows = sc_chunk_rows(dim);
  p.chunks = (n_rows + p.chunk_rows - 1) / p.chunk_rows;
  p.class_mean = d_class_mean, p.sw = d_sw;

  if ((flags & 1) && n_rows > 0) {
    hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)((n_rows + 15) / 16)), dim3(256), 0, ctx->stream, d_emb, n_rows, (int)dim, norms);
    SVK_LAUNCH_CHECK(ctx);
  }
  hipLaunchKernelGGL(class_mean_kernel, dim3((unsigned)n_class), dim3(128), 0, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(eff_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  const int nb = sc_blocks16(dim), n_tiles = sc_tiles(dim);
  if (p.chunks > 0) {
    const dim3 grid((unsigned)p.chunks, (unsigned)((n_tiles + SC_TILES_PER_GROUP - 1) / SC_TILES_PER_GROUP));
    const size_t lds = sizeof(double) * (nb <= 8 ? 16 : 8) * (16 * nb + 2);
    if (nb <= 8) hipLaunchKernelGGL(scatter_kernel<8>, grid, dim3(SC_THREADS), lds, ctx->stream, p);
    else hipLaunchKernelGGL(scatter_kernel<32>, grid, dim3(SC_THREADS), lds, ctx->stream, p);
    SVK_LAUNCH_CHECK(ctx);
  }
  hipLaunchKernelGGL(scatter_reduce_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_embedding_project(svk_ctx* ctx, const float* d_emb, int64_t n_rows, int32_t dim, const float* d_mean, const float* d_w,
                          int32_t out_dim, int32_t flags, float* d_out) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, (flags & ~3) == 0, "flags: bits 0 (L2-normalise the input) and 1 (L2-normalise the output) are defined");
  SVK_REQUIRE(ctx, n_rows >= 0, "negative shape");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= PJ_MAX_OUT && out_dim >= 1 && out_dim <= dim, "1 <= out_dim <= dim <= 512");
  SVK_REQUIRE(ctx, d_w || out_dim == dim, "a NULL d_w is the identity: out_dim must equal dim");
  if (n_rows == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_emb && d_out, "NULL buffer");
  SVK_REQUIRE(ctx, d_out != d_emb, "d_out must not be d_emb");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_emb) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_mean) |
                     reinterpret_cast<uintptr_t>(d_w)) & 3) == 0, "buffers must be 4-byte aligned");
  const int64_t blocks = (n_rows + PJ_ROWS - 1) / PJ_ROWS;
  SVK_REQUIRE(ctx, blocks < ((int64_t)1 << 31), "too many rows for one launch");
  const bool vec4 = dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(d_emb) | reinterpret_cast<uintptr_t>(d_mean)) & 15) == 0;
  const ProjectParams p{d_emb, n_rows, dim, out_dim, flags, d_mean, d_w, d_out};
  void (*kern)(const ProjectParams);
  const int nt = d_w ? (out_dim + 15) / 16 : 1;
  if (nt <= 1) kern = vec4 ? embedding_project_kernel<1, true> : embedding_project_kernel<1, false>;
  else if (nt <= 2) kern = vec4 ? embedding_project_kernel<2, true> : embedding_project_kernel<2, false>;
  else if (nt <= 4) kern = vec4 ? embedding_project_kernel<4, true> : embedding_project_kernel<4, false>;
  else if (nt <= 8) kern = vec4 ? embedding_project_kernel<8, true> : embedding_project_kernel<8, false>;
  else if (nt <= 16) kern = vec4 ? embedding_project_kernel<16, true> : embedding_project_kernel<16, false>;
  else kern = vec4 ? embedding_project_kernel<32, true> : embedding_project_kernel<32, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(PJ_THREADS), 0, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
