// svk_embedding_pool: the mean over groups of embedding rows -- the K cubes of a clip (uniform groups of K consecutive rows) and
// the utterances of a speaker (CSR offsets + a row index: pipeline.enroll_mean) are the same operation.
//
// A TEAM of TPT threads (a power of two, at most one wave) owns one segment; thread t of it owns the columns 4 (t + TPT k) .. + 3,
// k < CPT.  dim = 128: 32 threads per segment, EIGHT segments per workgroup, and a segment of K = 2 .. 16 rows is K row loads per
// thread, four in flight at a time -- the pipeline's case, 148 642 x 4 rows, is one streaming pass.  Arithmetic in float64:
//   * a segment's rows are added in order inside blocks of POOL_ROW_BLOCK rows, and the blocks' partial sums are added in order:
//     the order of additions depends on the segment's length alone (not on n_seg, the grid, the other segments or the alignment:
//     16-byte loads and scalar loads fill the same registers), and the sum of 10^5 rows still carries the error of 64 + 10^5 / 64
//     additions, not of 10^5;
//   * bit 0: a row enters as x / ||x||, its norm summed over a thread's columns in order, then across the team by a butterfly
//     (every lane ends with the same bits); norm 0 -> zeros;   bit 1: the mean leaves as m / ||m||, 0 stays 0;
//   * an empty segment writes zeros and counts in *d_empty_count;  NaN propagates (a NaN norm divides, it is not "zero").
// A segment runs on ONE team whatever its length: the many-short-segments case pays nothing for the long one, and 1 211
// speakers of ~120 utterances are 1 211 teams.  (A single segment of 10^5 rows would want its blocks spread over workgroups; the
// block order above is what such a split has to keep.)
#include "svk_internal.h"

namespace {

constexpr int POOL_ROW_BLOCK = 64;
constexpr int POOL_THREADS = 256;

struct PoolParams {
  const float* emb;
  int64_t n_rows, n_seg;
  int32_t dim, rows_per_seg;
  const int64_t* seg_start;
  const int64_t* row_index;
  int32_t flags, tpt_log2;
  float* out;
  int32_t* empty_count;
};

__device__ __forceinline__ double team_sum(double v, int tpt) {
  for (int m = tpt >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// VEC4: dim % 4 == 0 and 16-byte aligned rows -> one 16-byte load per chunk; else four guarded 4-byte loads.  CPT: chunks per
// thread (1 for dim <= 256).  U rows are loaded before the first is added.
template <bool VEC4, int CPT>
__global__ __launch_bounds__(POOL_THREADS) void embedding_pool_kernel(const PoolParams p) {
  constexpr int U = CPT == 1 ? 4 : CPT == 4 ? 2 : 1;
  const int tpt = 1 << p.tpt_log2, t = threadIdx.x & (tpt - 1);
  const int64_t s = (int64_t)blockIdx.x * (POOL_THREADS >> p.tpt_log2) + (threadIdx.x >> p.tpt_log2);
  if (s >= p.n_seg) return;   // (whole teams leave: the butterflies below stay inside a team)
  int64_t lo, hi;
  if (p.seg_start) {
    // offsets outside [0, n_rows] or out of order are the caller's error; clamped, so that nothing outside the buffers is read
    lo = std::min<int64_t>(std::max<int64_t>(p.seg_start[s], 0), p.n_rows);
    hi = std::min<int64_t>(std::max<int64_t>(p.seg_start[s + 1], lo), p.n_rows);
  } else {
    lo = s * p.rows_per_seg;
    hi = lo + p.rows_per_seg;
  }
  const int dim = p.dim;
  float* const orow = p.out + s * dim;
  if (hi == lo) {
#pragma unroll
    for (int k = 0; k < CPT; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = 4 * (t + tpt * k) + e;
        if (col < dim) orow[col] = 0.f;
      }
    if (t == 0 && p.empty_count) atomicAdd(p.empty_count, 1);
    return;
  }

  // row r's columns of this thread; columns >= dim read as 0.  A row index outside [0, n_rows) (the caller's error) is not
  // followed: the row reads as NaN
  auto load_row = [&](int64_t r, float (&x)[CPT][4]) {
    const bool ok = (uint64_t)r < (uint64_t)p.n_rows;
    const float* src = p.emb + (ok ? r : 0) * dim;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int col = 4 * (t + tpt * k);
      if constexpr (VEC4) {
        const float4 v = col < dim ? *reinterpret_cast<const float4*>(src + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        x[k][0] = v.x, x[k][1] = v.y, x[k][2] = v.z, x[k][3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = col + e < dim ? src[col + e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!ok && col + e < dim) x[k][e] = __builtin_nanf("");
    }
  };
  auto add_row = [&](double (&sum)[CPT][4], const float (&x)[CPT][4]) {
    if (p.flags & 1) {
      double ss = 0.0;
#pragma unroll
      for (int k = 0; k < CPT; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += (double)x[k][e] * (double)x[k][e];
      const double nrm = sqrt(team_sum(ss, tpt));
#pragma unroll
      for (int k = 0; k < CPT; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[k][e] += nrm == 0.0 ? 0.0 : (double)x[k][e] / nrm;
    } else {
#pragma unroll
      for (int k = 0; k < CPT; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[k][e] += (double)x[k][e];
    }
  };

  double acc[CPT][4] = {};
  for (int64_t b = lo; b < hi; b += POOL_ROW_BLOCK) {
    const int64_t be = std::min<int64_t>(hi, b + POOL_ROW_BLOCK);
    double part[CPT][4] = {};
    for (int64_t i = b; i < be; i += U) {
      float x[U][CPT][4];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i + u < be) load_row(p.row_index ? p.row_index[i + u] : i + u, x[u]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i + u < be) add_row(part, x[u]);
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[k][e] += part[k][e];
  }

  const double count = (double)(hi - lo);
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[k][e] /= count;
      ss += acc[k][e] * acc[k][e];
    }
  double nrm = 1.0;
  if (p.flags & 2) {
    nrm = sqrt(team_sum(ss, tpt));
    if (nrm == 0.0) nrm = 1.0;   // a zero mean stays zero
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int col = 4 * (t + tpt * k);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)((p.flags & 2) ? acc[k][e] / nrm : acc[k][e]);
    if constexpr (VEC4) {
      if (col < dim) *reinterpret_cast<float4*>(orow + col) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < dim) orow[col + e] = o[e];
    }
  }
}

}  // namespace

extern "C" {

int svk_embedding_pool(svk_ctx* ctx, const float* d_emb, int64_t n_rows, int32_t dim, int64_t n_seg, int32_t rows_per_seg,
                       const int64_t* d_seg_start, const int64_t* d_row_index, int32_t flags, float* d_out,
                       int32_t* d_empty_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, (flags & ~3) == 0, "flags: bits 0 (L2-normalise rows) and 1 (L2-normalise the mean) are defined");
  SVK_REQUIRE(ctx, n_rows >= 0 && n_seg >= 0, "negative shape");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= 4096, "dim must be in [1, 4096]");
  if (!d_seg_start) {
    SVK_REQUIRE(ctx, rows_per_seg >= 1, "rows_per_seg must be at least 1 when d_seg_start is NULL");
    SVK_REQUIRE(ctx, n_seg <= n_rows / rows_per_seg, "n_seg * rows_per_seg exceeds n_rows");
  }
  if (n_seg == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_out && (d_emb || n_rows == 0), "NULL buffer");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_emb) | reinterpret_cast<uintptr_t>(d_out)) & 3) == 0, "rows must be 4-byte aligned");
  const int quads = (dim + 3) / 4;
  int tpt_log2 = 0;
  while ((1 << tpt_log2) < quads && tpt_log2 < 6) ++tpt_log2;
  const int cpt = (quads + (1 << tpt_log2) - 1) >> tpt_log2;   // 1 for dim <= 256, at most 16
  const int64_t teams = POOL_THREADS >> tpt_log2, blocks = (n_seg + teams - 1) / teams;
  SVK_REQUIRE(ctx, blocks < ((int64_t)1 << 31), "too many segments for one launch");
  const bool vec4 = dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(d_emb) | reinterpret_cast<uintptr_t>(d_out)) & 15) == 0;
  const PoolParams p{d_emb, n_rows, n_seg, dim, rows_per_seg, d_seg_start, d_row_index, flags, tpt_log2, d_out, d_empty_count};
  void (*kern)(const PoolParams);
  if (cpt == 1) kern = vec4 ? embedding_pool_kernel<true, 1> : embedding_pool_kernel<false, 1>;
  else if (cpt <= 4) kern = vec4 ? embedding_pool_kernel<true, 4> : embedding_pool_kernel<false, 4>;
  else kern = vec4 ? embedding_pool_kernel<true, 16> : embedding_pool_kernel<false, 16>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(POOL_THREADS), 0, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
