// Speaker diarization: what stands between per-window embeddings and "who spoke when".
//
// svk_window_crops      per-recording frame counts -> the [n_rec][max_windows][n_crops] crop table of svk_c3d2_stage1_multi:
//                       one thread per (recording, window), integer arithmetic only.
// svk_segment_affinity  the cosine of every pair of live rows of every recording, float64 on v_mfma_f64_16x16x4_f64.  One wave
//                       owns one 16 x 16 tile of the upper triangle of one recording: lane (r = lane & 15, g = lane >> 4) loads
//                       columns 16 S + 4 g .. + 3 of row r of both tile sides per super-step S and feeds four MFMAs, e = 0 .. 3,
//                       whose k of lane group g is 16 S + 4 g + e.  The same registers give the squared norms: each lane adds its
//                       columns in order, then the four g meet in a two-step butterfly (every lane of a row ends with the same
//                       bits, and a row has the same norm on either side of a tile).  Entries with i <= j are written to [i][j] and
//                       [j][i].  Dead rows read as zeros and are never written: nothing outside the live block is touched.
// svk_ahc               average-linkage agglomerative clustering, one workgroup per recording, thread m owns rows m, m + 256, ...
//                       W is a full symmetric float64 matrix (both copies are kept, so a row's entries lie along the row) in LDS
//                       for n <= 128 and in the recording's slot of d_workspace above; both instances are ONE function body.
//                       Every row keeps its best partner j > m (the lowest j among equals); a step is a workgroup reduction of
//                       those n candidates under the strict order (larger value, then lower i).  After merging j into i, row i and
//                       the rows whose best was i or j are listed and searched again, a WAVE per row; any other row m < i only
//                       compares the new W[m][i] with what it holds (average linkage is reducible: the new value cannot beat the
//                       row's best by more than rounding, and where it does or ties at a lower index the comparison takes it).
//                       The update is two products, a sum and a quotient, each rounded once (no contraction in this file).
// (Corpus clustering, svk_knn_cluster, is a file of its own: knn_cluster.hip.)
#include "svk_internal.h"

#pragma clang fp contract(off)

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ window crops
__global__ __launch_bounds__(256) void window_crops_kernel(const int32_t* __restrict__ n_frames, int n_rec, int win, int hop,
                                                           int crop, int n_crops, int max_windows,
                                                           int32_t* __restrict__ crop_idx, int32_t* __restrict__ n_windows,
                                                           int32_t* __restrict__ span, int32_t* __restrict__ bad_count) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)n_rec * max_windows) return;
  const int r = (int)(id / max_windows), w = (int)(id % max_windows);
  const int T = std::max(n_frames[r], 0);
  int64_t need;   // windows the rule asks for
  if (T < crop) need = 0;
  else if (T < win) need = 1;
  else need = (int64_t)(T - win) / hop + 1 + ((T - win) % hop != 0);
  if (w == 0) {
    n_windows[r] = (int32_t)std::min<int64_t>(need, max_windows);
    if (need > max_windows && bad_count) atomicAdd(bad_count, 1);
  }
  int32_t* out = crop_idx + id * n_crops;
  if (w >= need) {
    for (int c = 0; c < n_crops; ++c) out[c] = -1;
    if (span) span[2 * id] = -1, span[2 * id + 1] = 0;
    return;
  }
  int w0, len;
  if (T < win) w0 = 0, len = T;
  else if (w <= (T - win) / hop) w0 = w * hop, len = win;
  else w0 = T - win, len = win;
  const int64_t room = len - crop, den = std::max(n_crops - 1, 1);
  for (int c = 0; c < n_crops; ++c) out[c] = (int32_t)(w0 + (c * room) / den);
  if (span) span[2 * id] = w0, span[2 * id + 1] = len;
}

// ------------------------------------------------------------------------------------------------ segment affinity
constexpr int AFF_THREADS = 256, AFF_WAVES = AFF_THREADS / 64;

// columns [col, col + 4) of a row; zeros for a dead row and past dim
template <bool VEC4>
__device__ __forceinline__ void aff_load4(const float* row, int col, int dim, bool live, float (&x)[4]) {
  if constexpr (VEC4) {
    const f4 v = live && col < dim ? *reinterpret_cast<const f4*>(row + col) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = v[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = live && col + e < dim ? row[col + e] : 0.f;
  }
}

template <bool VEC4>
__global__ __launch_bounds__(AFF_THREADS) void segment_affinity_kernel(const float* __restrict__ emb, int stride, int dim,
                                                                       const int32_t* __restrict__ n_seg,
                                                                       float* __restrict__ aff, int tiles, int chunks) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int rec = blockIdx.x / chunks;
  const int n = std::min(std::max(n_seg[rec], 0), stride);
  // the wave's tile of the upper triangle: tile rows ti <= tj, counted row by row (at most `tiles` scalar steps)
  int w = (blockIdx.x % chunks) * AFF_WAVES + (threadIdx.x >> 6), ti = 0;
  while (ti < tiles && w >= tiles - ti) w -= tiles - ti, ++ti;
  if (ti >= tiles) return;
  const int tj = ti + w;
  if (16 * tj >= n) return;   // (no barrier in this kernel: whole waves leave)
  const float* base = emb + (size_t)rec * stride * dim;
  const int ia = 16 * ti + r, ib = 16 * tj + r;
  const bool la = ia < n, lb = ib < n;
  const float* pa = base + (size_t)(la ? ia : 0) * dim;
  const float* pb = base + (size_t)(lb ? ib : 0) * dim;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  double sa = 0.0, sb = 0.0;
  for (int k0 = 0; k0 < dim; k0 += 16) {
    float xa[4], xb[4];
    aff_load4<VEC4>(pa, k0 + 4 * g, dim, la, xa);
    aff_load4<VEC4>(pb, k0 + 4 * g, dim, lb, xb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double da = (double)xa[e], db = (double)xb[e];
      sa = fma(da, da, sa);   // (a product of two floats is exact in float64: one rounding per addition)
      sb = fma(db, db, sb);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(da, db, acc, 0, 0, 0);
    }
  }
  sa += __shfl_xor(sa, 16, 64);
  sa += __shfl_xor(sa, 32, 64);
  sb += __shfl_xor(sb, 16, 64);
  sb += __shfl_xor(sb, 32, 64);
  double na = sqrt(sa), nb = sqrt(sb);
  na = na == 0.0 ? 1.0 : na;   // sklearn normalize(): a zero norm divides by 1
  nb = nb == 0.0 ? 1.0 : nb;
  float* out = aff + (size_t)rec * stride * stride;
  // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = g + 4 * reg;
    const double nrow = __shfl(na, row, 64);   // lane `row` holds tile row `row` of the A side
    const int gi = 16 * ti + row, gj = 16 * tj + r;
    if (gi < n && gj < n && gi <= gj) {
      const float v = (float)(acc[reg] / (nrow * nb));
      out[(size_t)gi * stride + gj] = v;
      out[(size_t)gj * stride + gi] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ AHC
constexpr int AHC_THREADS = 256, AHC_WAVES = AHC_THREADS / 64;
constexpr int AHC_LDS_N = 128;        // the largest n whose float64 matrix lives in LDS: 128 KiB of the 160
constexpr int AHC_MAX_STRIDE = 2048;

struct AhcParams {
  const float* aff;
  int32_t n_rec, stride;
  const int32_t* n_seg;
  double threshold;
  int32_t min_clusters, max_clusters;
  const int32_t* target;
  double* work;
  int32_t* labels;
  int32_t* n_clusters;
  int32_t* merge_pair;
  double* merge_sim;
  int32_t* bad_count;
};

// a merge candidate: row i's best partner j > i.  The order is strict and total over live rows: larger value, then lower i
struct Cand {
  double v;
  int i, j;
};
__device__ __forceinline__ bool ahc_better(const Cand& a, const Cand& b) { return a.v > b.v || (a.v == b.v && a.i < b.i); }

constexpr int AHC_NO_ROW = 0x7fffffff;

// the per-row vectors of a recording of up to `cap` rows (cap even: best value, best partner, size, representative, the scan
// list), then -- LDS instance -- the matrix, its rows an ODD number of float64 apart (a column write then walks all banks)
__host__ __device__ constexpr size_t ahc_vec_bytes(int cap) { return (size_t)cap * (sizeof(double) + 4 * sizeof(int)); }
__host__ __device__ constexpr int ahc_even(int n) { return (n + 1) & ~1; }

// labels -1 over `rows` rows, count -1, the merge slots unused, one more bad recording
__device__ void ahc_reject(int rows, int stride, int32_t* labels, int32_t* n_clusters, int32_t* mp, double* ms, int32_t* bad) {
  for (int m = threadIdx.x; m < rows; m += AHC_THREADS) labels[m] = -1;
  for (int s = threadIdx.x; s < stride; s += AHC_THREADS) {
    if (mp) mp[2 * s] = -1, mp[2 * s + 1] = -1;
    if (ms) ms[s] = __builtin_nan("");
  }
  if (threadIdx.x == 0) {
    *n_clusters = -1;
    if (bad) atomicAdd(bad, 1);
  }
}

// One recording.  W: n rows of float64, `ld` apart (LDS: n | 1, workspace: n), A: the recording's f32 matrix with row stride
// `stride`.  todo / todo_n: the rows whose best partner has to be searched again, filled by their owners, scanned by whole waves.
template <bool LDSW>
__device__ __forceinline__ void ahc_run(double* W, const float* __restrict__ A, int n, int stride, double thr, int min_c,
                                        int max_c, double* bestv, int* bestj, int* size, int* rep, int* todo, int* todo_n,
                                        Cand* red, int32_t* labels, int32_t* n_clusters, int32_t* mp, double* ms, int32_t* bad) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ld = LDSW ? (n | 1) : n;
  // W[a][b] = W[b][a] = the entry ABOVE the diagonal; nothing below it is read
  int flag = 0;
  for (int idx = tid; idx < n * n; idx += AHC_THREADS) {
    const int a = idx / n, b = idx - a * n;
    double v = 0.0;
    if (a != b) {
      v = (double)A[(size_t)std::min(a, b) * stride + std::max(a, b)];
      flag |= !(fabs(v) <= 1.79769313486231570815e+308);
    }
    W[a * ld + b] = v;
  }
  for (int m = tid; m < n; m += AHC_THREADS) size[m] = 1, rep[m] = m, todo[m] = m;
  if (__syncthreads_or(flag)) {
    ahc_reject(n, stride, labels, n_clusters, mp, ms, bad);
    return;
  }

  // The best live partner c > m of every row in todo[0 .. count), the lowest c among equals: a wave per row, lane l looks at
  // c = m + 1 + l, + 64, ... in ascending order (a strict > keeps its lowest), then a butterfly under (larger value, lower c).
  // Row m is read along itself (W[m][c], consecutive lanes at consecutive addresses).  A selection only: no arithmetic
  auto scan_rows = [&](int count) {
    for (int q = wave; q < count; q += AHC_WAVES) {
      const int m = todo[q];
      double bv = -__builtin_inf();
      int bj = AHC_NO_ROW;
      for (int c = m + 1 + lane; c < n; c += 64) {
        if (size[c] == 0) continue;
        const double v = W[m * ld + c];
        if (v > bv) bv = v, bj = c;
      }
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) {
        const double ov = __shfl_xor(bv, x, 64);
        const int oj = __shfl_xor(bj, x, 64);
        if (ov > bv || (ov == bv && oj < bj)) bv = ov, bj = oj;
      }
      if (lane == 0) bestv[m] = bv, bestj[m] = bj == AHC_NO_ROW ? -1 : bj;
    }
  };
  scan_rows(n);
  __syncthreads();

  int steps = 0;
  for (int t = 0; t + 1 < n; ++t) {   // at most n - 1 merges
    Cand c{-__builtin_inf(), AHC_NO_ROW, -1};
    for (int m = tid; m < n; m += AHC_THREADS)
      if (size[m] > 0 && bestj[m] >= 0) {
        const Cand o{bestv[m], m, bestj[m]};
        if (ahc_better(o, c)) c = o;
      }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const Cand o{__shfl_xor(c.v, x, 64), __shfl_xor(c.i, x, 64), __shfl_xor(c.j, x, 64)};
      if (ahc_better(o, c)) c = o;
    }
    if (lane == 0) red[wave] = c;
    __syncthreads();
    c = red[0];
#pragma unroll
    for (int x = 1; x < AHC_WAVES; ++x)
      if (ahc_better(red[x], c)) c = red[x];
    // (every thread holds the same c from here on: the loop is uniform)
    const int k = n - t;
    if (c.j < 0 || !(k > max_c || (k > min_c && c.v >= thr))) break;
    const int i = c.i, j = c.j;
    const double si = (double)size[i], sj = (double)size[j];
    if (tid == 0) {
      if (mp) mp[2 * t] = i, mp[2 * t + 1] = j;
      if (ms) ms[t] = c.v;
    }
    const double ssum = si + sj;
    for (int m = tid; m < n; m += AHC_THREADS) {
      if (rep[m] == j) rep[m] = i;
      if (size[m] == 0 || m == i || m == j) continue;
      const double a = W[i * ld + m], b = W[j * ld + m];
      // plain operators under this file's `fp contract(off)`: the header intrinsics (__dmul_rn, __dadd_rn) are compiled with
      // the default contraction and fuse into one fma once inlined
      const double pa = si * a, pb = sj * b;
      const double nv = (pa + pb) / ssum;
      W[i * ld + m] = nv;
      W[m * ld + i] = nv;
    }
    __syncthreads();
    if (tid == 0) size[i] = (int)ssum, size[j] = 0, *todo_n = 0;
    __syncthreads();
    // row i and the rows whose best was i or j are searched again; any other row m < i compares the one entry that changed
    for (int m = tid; m < n; m += AHC_THREADS) {
      if (size[m] == 0) continue;
      if (m == i || (m < j && (bestj[m] == j || bestj[m] == i))) {
        todo[atomicAdd(todo_n, 1)] = m;   // (an integer LDS atomic: the order of the list changes no result)
      } else if (m < i) {
        const double nv = W[i * ld + m];
        if (nv > bestv[m] || (nv == bestv[m] && i < bestj[m])) bestv[m] = nv, bestj[m] = i;
      }
    }
    __syncthreads();
    scan_rows(*todo_n);
    __syncthreads();
    ++steps;
  }
  __syncthreads();   // rep and size of the last step

  // clusters in the order of their lowest member: a cluster's representative IS its lowest member (j merges into i < j)
  for (int m = tid; m < n; m += AHC_THREADS) {
    const int root = rep[m];
    int lower = 0;
    for (int c = 0; c < root; ++c) lower += size[c] > 0;
    labels[m] = lower;
  }
  for (int s = steps + tid; s < stride; s += AHC_THREADS) {
    if (mp) mp[2 * s] = -1, mp[2 * s + 1] = -1;
    if (ms) ms[s] = __builtin_nan("");
  }
  if (tid == 0) *n_clusters = n - steps;
}

__global__ __launch_bounds__(AHC_THREADS) void ahc_kernel(const AhcParams p) {
  extern __shared__ double ahc_smem[];
  __shared__ Cand red[AHC_WAVES];
  __shared__ int todo_n;
  const int rec = blockIdx.x, stride = p.stride;
  const int n = p.n_seg[rec];
  int32_t* labels = p.labels + (size_t)rec * stride;
  int32_t* mp = p.merge_pair ? p.merge_pair + (size_t)rec * stride * 2 : nullptr;
  double* ms = p.merge_sim ? p.merge_sim + (size_t)rec * stride : nullptr;
  if (n < 0 || n > stride) {   // not followed: every label of the slot says so
    ahc_reject(stride, stride, labels, p.n_clusters + rec, mp, ms, p.bad_count);
    return;
  }
  int min_c = p.min_clusters, max_c = p.max_clusters;
  if (p.target && p.target[rec] >= 1) min_c = max_c = p.target[rec];
  const float* A = p.aff + (size_t)rec * stride * stride;
  const bool in_lds = n <= AHC_LDS_N;
  const int cap = in_lds ? ahc_even(std::min(stride, AHC_LDS_N)) : ahc_even(stride);
  double* bestv = ahc_smem;
  int* bestj = reinterpret_cast<int*>(bestv + cap);
  int* size = bestj + cap;
  int* rep = size + cap;
  int* todo = rep + cap;
  if (in_lds)
    ahc_run<true>(reinterpret_cast<double*>(todo + cap), A, n, stride, p.threshold, min_c, max_c, bestv, bestj, size, rep, todo,
                  &todo_n, red, labels, p.n_clusters + rec, mp, ms, p.bad_count);
  else
    ahc_run<false>(p.work + (size_t)rec * stride * stride, A, n, stride, p.threshold, min_c, max_c, bestv, bestj, size, rep, todo,
                   &todo_n, red, labels, p.n_clusters + rec, mp, ms, p.bad_count);
}

// dynamic LDS of a launch: the vectors and the matrix of the LDS instance, or the vectors of the workspace instance
size_t ahc_lds_bytes(int stride) {
  const int lc = std::min(stride, AHC_LDS_N);
  const size_t lds_inst = ahc_vec_bytes(ahc_even(lc)) + sizeof(double) * (size_t)lc * (lc | 1);
  return stride > AHC_LDS_N ? std::max(lds_inst, ahc_vec_bytes(ahc_even(stride))) : lds_inst;
}

}  // namespace

extern "C" {

int svk_window_crops(svk_ctx* ctx, const int32_t* d_n_frames, int32_t n_rec, int32_t win_frames, int32_t hop_frames,
                     int32_t crop_frames, int32_t n_crops, int32_t max_windows, int32_t* d_crop_idx, int32_t* d_n_windows,
                     int32_t* d_window_span, int32_t* d_bad_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rec >= 0, "negative shape");
  SVK_REQUIRE(ctx, crop_frames >= 1 && win_frames >= crop_frames && hop_frames >= 1, "windows need win_frames >= crop_frames >= 1 and hop_frames >= 1");
  SVK_REQUIRE(ctx, n_crops >= 1 && max_windows >= 1, "n_crops and max_windows must be at least 1");
  SVK_REQUIRE(ctx, (int64_t)max_windows * n_crops < ((int64_t)1 << 31) && (int64_t)n_crops * win_frames < ((int64_t)1 << 31),
              "max_windows * n_crops and n_crops * win_frames must stay below 2^31");
  if (n_rec == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_n_frames && d_crop_idx && d_n_windows, "NULL buffer");
  SVK_REQUIRE(ctx, !misaligned(d_n_frames, 4) && !misaligned(d_crop_idx, 4) && !misaligned(d_n_windows, 4) &&
                       !misaligned(d_window_span, 4) && !misaligned(d_bad_count, 4), "int32 buffers must be 4-byte aligned");
  const int64_t blocks = ((int64_t)n_rec * max_windows + 255) / 256;
  SVK_REQUIRE(ctx, blocks < ((int64_t)1 << 31), "too many windows for one launch");
  hipLaunchKernelGGL(window_crops_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_n_frames, (int)n_rec,
                     (int)win_frames, (int)hop_frames, (int)crop_frames, (int)n_crops, (int)max_windows, d_crop_idx, d_n_windows,
                     d_window_span, d_bad_count);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_segment_affinity(svk_ctx* ctx, const float* d_emb, int32_t n_rec, int32_t seg_stride, int32_t dim,
                         const int32_t* d_n_seg, float* d_aff) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rec >= 0 && seg_stride >= 0, "negative shape");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= 512, "dim must be in [1, 512]");
  if (n_rec == 0 || seg_stride == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_emb && d_n_seg && d_aff, "NULL buffer");
  SVK_REQUIRE(ctx, !misaligned(d_emb, 4) && !misaligned(d_n_seg, 4) && !misaligned(d_aff, 4), "buffers must be 4-byte aligned");
  const int64_t tiles = (seg_stride + 15) / 16, upper = tiles * (tiles + 1) / 2;
  const int64_t chunks = (upper + AFF_WAVES - 1) / AFF_WAVES;
  SVK_REQUIRE(ctx, chunks * n_rec < ((int64_t)1 << 31), "too many tiles for one launch");
  const bool vec4 = dim % 4 == 0 && !misaligned(d_emb, 16);
  auto kern = vec4 ? segment_affinity_kernel<true> : segment_affinity_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(chunks * n_rec)), dim3(AFF_THREADS), 0, ctx->stream, d_emb, (int)seg_stride, (int)dim,
                     d_n_seg, d_aff, (int)tiles, (int)chunks);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_ahc_limits(int32_t out[2]) {
  if (!out) return SVK_ERR_BAD_ARG;
  out[0] = AHC_LDS_N;
  out[1] = AHC_MAX_STRIDE;
  return SVK_OK;
}

size_t svk_ahc_workspace_bytes(int32_t n_rec, int32_t seg_stride) {
  if (n_rec <= 0 || seg_stride <= AHC_LDS_N || seg_stride > AHC_MAX_STRIDE) return 0;
  return sizeof(double) * (size_t)n_rec * seg_stride * seg_stride;
}

int svk_ahc(svk_ctx* ctx, const float* d_aff, int32_t n_rec, int32_t seg_stride, const int32_t* d_n_seg, double threshold,
            int32_t min_clusters, int32_t max_clusters, const int32_t* d_target, void* d_workspace, size_t workspace_bytes,
            int32_t* d_labels, int32_t* d_n_clusters, int32_t* d_merge_pair, double* d_merge_sim, int32_t* d_bad_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rec >= 0 && seg_stride >= 0, "negative shape");
  SVK_REQUIRE(ctx, seg_stride <= AHC_MAX_STRIDE, "seg_stride above svk_ahc_limits()[1]");
  SVK_REQUIRE(ctx, min_clusters >= 1 && max_clusters >= min_clusters, "stop rule needs 1 <= min_clusters <= max_clusters");
  SVK_REQUIRE(ctx, threshold == threshold, "threshold is NaN");
  if (n_rec == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_n_seg && d_labels && d_n_clusters && (d_aff || seg_stride == 0), "NULL buffer");
  SVK_REQUIRE(ctx, !misaligned(d_aff, 4) && !misaligned(d_n_seg, 4) && !misaligned(d_target, 4) && !misaligned(d_labels, 4) &&
                       !misaligned(d_n_clusters, 4) && !misaligned(d_merge_pair, 4) && !misaligned(d_bad_count, 4) &&
                       !misaligned(d_merge_sim, 8), "misaligned buffer (int32 / f32: 4 bytes, float64: 8)");
  const size_t need = svk_ahc_workspace_bytes(n_rec, seg_stride);
  if (need) {
    SVK_REQUIRE(ctx, d_workspace && workspace_bytes >= need, "workspace below svk_ahc_workspace_bytes");
    SVK_REQUIRE(ctx, !misaligned(d_workspace, 16), "workspace must be 16-byte aligned");
  }
  const size_t lds = ahc_lds_bytes(seg_stride);
  if (lds + 256 > (size_t)ctx->lds_per_cu)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "svk_ahc needs %zu bytes of LDS per workgroup (device: %d)", lds, ctx->lds_per_cu);
  SVK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(ahc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const AhcParams p{d_aff, n_rec, seg_stride, d_n_seg, threshold, min_clusters, max_clusters, d_target,
                    static_cast<double*>(d_workspace), d_labels, d_n_clusters, d_merge_pair, d_merge_sim, d_bad_count};
  hipLaunchKernelGGL(ahc_kernel, dim3((unsigned)n_rec), dim3(AHC_THREADS), lds, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
