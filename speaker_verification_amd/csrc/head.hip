// C3D2's classification head, model.py:170-174 (forward, development=True): PReLU5 -> FC6 -> softmax, plus the top-k of the
// probabilities and the hit counts of train.py:104-119's accuracy pass, in one kernel on v_mfma_f32_16x16x4_f32.
//
// Layout.  FC6 is a GEMM with the labels as M and the rows as N: A = W6 (lane: label i = l & 15), B = PReLU5(emb)
// (lane: row j = l & 15), so D[label 4 (l >> 4) + r][row l & 15] -- every lane holds four labels of ONE row and keeps that row's
// running state (max, sum, top-k) in registers; the four lane groups of a row are combined by two xor shuffles at the end.
// K = 128 runs as 32 steps; lane group kk = l >> 4 takes K index 32 kk + s at step s, so a lane's A and B operands of all 32
// steps are 32 consecutive floats of a weight row / an embedding row (eight 16-byte loads, W6 read row-major as it is stored).
// Each of the eight 4-step K blocks q (K indices 32 kk + 4 q + e) is one fma chain of 16 products from zero; the eight partial
// sums are added pairwise, ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)), and the bias last -- a fixed order.
//
// A wave owns RT_TILES x 16 rows, their B fragments live in VGPRs for the whole kernel, and it walks the label tiles three times:
//   pass 1  m = max l                      (a NaN logit makes m NaN)
//   pass 2  s = sum exp(l - m)             per lane in label order (Kahan), then (s0 + s1) + (s2 + s3) over the lane groups
//   pass 3  p = e / s (IEEE division), written to d_probs when asked; the row's top-k of p kept sorted per lane, merged at the end
// The logits are recomputed in every pass (no read-back of an intermediate): what a row gets is a function of that row's
// embedding and the tables alone, whatever n, the row's position or the grid (DESIGN 3.7 has the costs).
#include <cmath>

#include "svk_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_WAVES = HEAD_THREADS / 64;
constexpr int RT_TILES = 2;                    // 16-row tiles per wave: 32 rows, 64 VGPRs of B fragments
constexpr int HEAD_ROWS = 16 * RT_TILES;
constexpr int HEAD_MAX_K = 8;
constexpr int HEAD_MAX_LABELS = 65536;

// Descending p, a NaN above every number (torch.sort's order), ties to the lower label.
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

template <int KT>
__device__ __forceinline__ void insert(float (&v)[KT], int (&ix)[KT], float c, int ci) {
  if (!before(c, ci, v[KT - 1], ix[KT - 1])) return;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    if (before(c, ci, v[j], ix[j])) {
      const float tv = v[j];
      const int ti = ix[j];
      v[j] = c;
      ix[j] = ci;
      c = tv;
      ci = ti;
    }
  }
}

struct HeadParams {
  const float* emb;
  int64_t n;
  int n_labels;
  float slope;
  const float* w;
  const float* b;
  float* probs;
  int k;
  int32_t* topk;
  const int32_t* tru;
  unsigned long long* hits;
};

template <int KT>
__global__ __launch_bounds__(HEAD_THREADS) void head_kernel(const HeadParams p) {
  const int lane = threadIdx.x & 63, kk = lane >> 4, j = lane & 15;
  const int wave = threadIdx.x >> 6;
  const int n_tiles = (p.n_labels + 15) >> 4;
  const int64_t n_groups = (p.n + HEAD_ROWS - 1) / HEAD_ROWS;
  unsigned long long hit[KT];
#pragma unroll
  for (int r = 0; r < KT; ++r) hit[r] = 0;

  for (int64_t g = (int64_t)blockIdx.x * HEAD_WAVES + wave; g < n_groups; g += (int64_t)gridDim.x * HEAD_WAVES) {
    // B fragments: row 16 t + j of the group, K indices 32 kk .. 32 kk + 31, PReLU5 applied (nn.PReLU: x, or slope * x for x <= 0)
    f32x4 bf[RT_TILES][8];
    int64_t row[RT_TILES];
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t) {
      row[t] = g * HEAD_ROWS + 16 * t + j;
      const f32x4* src = reinterpret_cast<const f32x4*>(p.emb + (size_t)min(row[t], p.n - 1) * 128 + 32 * kk);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        f32x4 x = src[q];
        if (row[t] >= p.n) x = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] > 0.f ? x[e] : p.slope * x[e];
        bf[t][q] = x;
      }
    }
    // the logits of label tile lt for every row tile: acc[t][r] = l[label 16 lt + 4 kk + r][row 16 t + j]
    auto logits = [&](int lt, f32x4 (&acc)[RT_TILES]) {
      const int lab = 16 * lt + j;                                   // the A row this lane loads
      const bool live = lab < p.n_labels;
      const f32x4* wr = reinterpret_cast<const f32x4*>(p.w + (size_t)min(lab, p.n_labels - 1) * 128 + 32 * kk);
      f32x4 af[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) af[q] = live ? wr[q] : (f32x4){0.f, 0.f, 0.f, 0.f};
      f32x4 bias;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lb = 16 * lt + 4 * kk + r;
        bias[r] = lb < p.n_labels ? p.b[lb] : 0.f;
      }
      // eight partial sums per row tile (K step q: 16 K values each, one fma chain), added pairwise, then the bias: an error
      // like torch's tree-reduced GEMV, not the 128-long chain's
      f32x4 part[RT_TILES][8];
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int t = 0; t < RT_TILES; ++t) {
          part[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) part[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[q][e], bf[t][q][e], part[t][q], 0, 0, 0);
        }
#pragma unroll
      for (int t = 0; t < RT_TILES; ++t)
        acc[t] = (((part[t][0] + part[t][1]) + (part[t][2] + part[t][3])) + ((part[t][4] + part[t][5]) + (part[t][6] + part[t][7]))) + bias;
    };

    // pass 1: the row maximum (NaN wins)
    float m[RT_TILES];
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t) m[t] = -INFINITY;
#pragma unroll 1
    for (int lt = 0; lt < n_tiles; ++lt) {
      f32x4 acc[RT_TILES];
      logits(lt, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (16 * lt + 4 * kk + r >= p.n_labels) continue;
#pragma unroll
        for (int t = 0; t < RT_TILES; ++t) {
          const float v = acc[t][r];
          if (v > m[t] || v != v) m[t] = v != v || m[t] != m[t] ? NAN : v;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t) {
#pragma unroll
      for (int x = 16; x <= 32; x <<= 1) {
        const float o = __shfl_xor(m[t], x, 64);
        m[t] = (m[t] != m[t] || o != o) ? NAN : fmaxf(m[t], o);
      }
    }

    // pass 2: s = sum of exp(l - m), label order within a lane, then the lane groups pairwise (commutative: every lane agrees)
    // (compensated: a lane adds up to 16 384 terms, whose plain f32 sum drifts by ~1e-5 of s at 65 536 labels)
    float s[RT_TILES], comp[RT_TILES];
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t) s[t] = comp[t] = 0.f;
#pragma unroll 1
    for (int lt = 0; lt < n_tiles; ++lt) {
      f32x4 acc[RT_TILES];
      logits(lt, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (16 * lt + 4 * kk + r >= p.n_labels) continue;
#pragma unroll
        for (int t = 0; t < RT_TILES; ++t) {
          const float y = expf(acc[t][r] - m[t]) - comp[t];
          const float u = s[t] + y;
          comp[t] = (u - s[t]) - y;
          s[t] = u;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t) {
      s[t] += __shfl_xor(s[t], 16, 64);
      s[t] += __shfl_xor(s[t], 32, 64);
    }

    // pass 3: p = e / s; the stored probabilities and the top-k see the same values
    float tv[RT_TILES][KT];
    int ti[RT_TILES][KT];
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t)
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        tv[t][c] = -INFINITY;
        ti[t][c] = 0x7fffffff;
      }
    const bool want_rank = p.topk || p.tru;
#pragma unroll 1
    for (int lt = 0; lt < n_tiles; ++lt) {
      f32x4 acc[RT_TILES];
      logits(lt, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lb = 16 * lt + 4 * kk + r;
        if (lb >= p.n_labels) continue;
#pragma unroll
        for (int t = 0; t < RT_TILES; ++t) {
          const float pr = __fdiv_rn(expf(acc[t][r] - m[t]), s[t]);
          if (row[t] < p.n) {
            if (p.probs) p.probs[(size_t)row[t] * (size_t)p.n_labels + lb] = pr;
            if (want_rank) insert<KT>(tv[t], ti[t], pr, lb);
          }
        }
      }
    }
    if (!want_rank) continue;
    // merge the four lane groups' lists (disjoint labels, a total order: every lane of the row ends with the same list)
#pragma unroll
    for (int t = 0; t < RT_TILES; ++t) {
#pragma unroll
      for (int x = 16; x <= 32; x <<= 1) {
        float ov[KT];
        int oi[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) {
          ov[c] = __shfl_xor(tv[t][c], x, 64);
          oi[c] = __shfl_xor(ti[t][c], x, 64);
        }
#pragma unroll
        for (int c = 0; c < KT; ++c) insert<KT>(tv[t], ti[t], ov[c], oi[c]);
      }
      if (kk == 0 && row[t] < p.n) {
        if (p.topk)
          for (int c = 0; c < p.k; ++c) p.topk[(size_t)row[t] * p.k + c] = ti[t][c];
        if (p.tru) {
          const int32_t want = p.tru[row[t]];
          bool found = false;
#pragma unroll
          for (int c = 0; c < KT; ++c) {
            found = found || (c < p.k && ti[t][c] == want && want >= 0 && want < p.n_labels);
            hit[c] += found ? 1 : 0;
          }
        }
      }
    }
  }
  if (!p.tru) return;
  __shared__ unsigned long long red[HEAD_WAVES][KT];
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    const unsigned long long h = (unsigned long long)wave_sum((long long)hit[c]);
    if (lane == 0) red[wave][c] = h;
  }
  __syncthreads();
  if (threadIdx.x < KT && threadIdx.x < p.k) {
    unsigned long long h = 0;
    for (int w = 0; w < HEAD_WAVES; ++w) h += red[w][threadIdx.x];
    if (h) atomicAdd(p.hits + threadIdx.x, h);
  }
}

template <int KT>
int launch_head(svk_ctx* ctx, const HeadParams& p) {
  const int64_t groups = (p.n + HEAD_ROWS - 1) / HEAD_ROWS;
  int per_cu = 1;
  SVK_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(head_kernel<KT>), HEAD_THREADS, 0));
  const int64_t resident = (int64_t)std::max(1, per_cu) * ctx->num_cu;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + HEAD_WAVES - 1) / HEAD_WAVES, resident));
  hipLaunchKernelGGL(head_kernel<KT>, dim3(grid), dim3(HEAD_THREADS), 0, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // namespace

extern "C" int svk_c3d2_head(svk_ctx* ctx, const float* d_emb, int64_t n, int32_t n_labels, float prelu_slope, const float* d_w6,
                             const float* d_b6, float* d_probs, int32_t k, int32_t* d_topk, const int32_t* d_true,
                             int64_t* h_hits) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 0, "n negative");
  SVK_REQUIRE(ctx, n_labels >= 1, "n_labels < 1");
  if (n_labels > HEAD_MAX_LABELS)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "n_labels %d above the head kernel's %d", n_labels, HEAD_MAX_LABELS);
  SVK_REQUIRE(ctx, d_w6 && d_b6, "NULL FC6 weights or bias");
  const bool rank = d_topk || d_true;
  if (rank) {
    SVK_REQUIRE(ctx, k >= 1, "k < 1 with a top-k or true labels asked for");
    SVK_REQUIRE(ctx, k <= n_labels, "k > n_labels");
    if (k > HEAD_MAX_K) return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "k = %d above the head kernel's %d", k, HEAD_MAX_K);
  }
  SVK_REQUIRE(ctx, !d_true || h_hits, "true labels without h_hits");
  SVK_REQUIRE(ctx, n == 0 || d_emb, "NULL embeddings");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_emb) | reinterpret_cast<uintptr_t>(d_w6)) & 15) == 0,
              "embeddings and FC6 weights must be 16-byte aligned");
  if (d_true)
    for (int c = 0; c < k; ++c) h_hits[c] = 0;
  if (n == 0 || (!d_probs && !rank)) return SVK_OK;
  hipStream_t st = ctx->stream;
  auto* hits = reinterpret_cast<unsigned long long*>(static_cast<char*>(ctx->scratch) + SVK_SLOT_HEAD);
  if (d_true) SVK_HIP(ctx, hipMemsetAsync(hits, 0, 8 * HEAD_MAX_K, st));
  const HeadParams p{d_emb, n, n_labels, prelu_slope, d_w6, d_b6, d_probs, rank ? (int)k : 0, d_topk, d_true, d_true ? hits : nullptr};
  const int kt = rank ? (int)k : 1;
  int rc = kt <= 1 ? launch_head<1>(ctx, p) : kt <= 2 ? launch_head<2>(ctx, p) : kt <= 4 ? launch_head<4>(ctx, p) : launch_head<8>(ctx, p);
  if (rc != SVK_OK) return rc;
  if (d_true) {
    unsigned long long h[HEAD_MAX_K] = {0};
    SVK_HIP(ctx, hipMemcpyAsync(h, hits, 8 * HEAD_MAX_K, hipMemcpyDeviceToHost, st));
    SVK_HIP(ctx, hipStreamSynchronize(st));
    for (int c = 0; c < k; ++c) h_hits[c] = (int64_t)h[c];
  }
  return SVK_OK;
}
