// Speaker search: the k best gallery rows of every query row by cosine score, without the score matrix.
//   svk_cosine_topk <- 1:N identification against enrolled embeddings (evaluation.py:112-134 takes the argmax of a row of
//       the [n_test x n_enroll] matrix; open-set search and large galleries cannot hold that matrix).
// Phase 1 is the tiled product of svk_cosine_scores (scoring.hip: cosine_tiled_kernel's LDS-staged, double-buffered 32-row
// gallery block on v_mfma_f32_16x16x4_f32) with an on-chip selection in place of the store epilogue; phase 2 merges the
// partial lists of the gallery spans, and the list of earlier calls with the accumulate flag, under the same total order.
#include <algorithm>

#include "score_common.h"
#include "svk_internal.h"

namespace {

constexpr int SR_BM = 128, SR_BN = 32, SR_KB = 128, SR_LD = SR_KB + 8;
constexpr int SR_KMAX = 32;            // list slots per row (k <= 32)
// The split of the gallery into spans depends on the shape alone (never on the device), so that the workspace size is a
// function of the shape: about SR_TARGET_UNITS (row block, span) units -- four rounds of the 2 x 256 resident workgroups
// of the MI355X -- while a span keeps at least SR_MIN_SPAN_TILES 32-row tiles (the lists' write-out and the query
// fragments' loads are paid per unit).  148 642 x 1 211: 1 162 row blocks, 38 tiles -> one span.  1 x 10^6: 976 spans.
constexpr int SR_TARGET_UNITS = 2048, SR_MIN_SPAN_TILES = 32, SR_MAX_SPANS = 1024;

struct sr_plan {
  long long n_rb = 0;
  int tiles = 0, spans = 1;
  size_t off_ginv = 0, off_score = 0, off_idx = 0, bytes = 0;   // the query's 1 / norms sit at offset 0
};

inline size_t sr_align(size_t v) { return (v + 15) & ~(size_t)15; }

inline bool sr_make_plan(int32_t nq, int32_t ng, int32_t dim, int32_t k, sr_plan* p) {
  if (nq < 0 || ng < 0 || dim < 1 || dim > 4096 || k < 1 || k > SR_KMAX) return false;
  *p = sr_plan();
  if (nq == 0 || ng == 0) return true;   // nothing is launched that needs a workspace
  p->n_rb = ((long long)nq + SR_BM - 1) / SR_BM;
  p->tiles = (int)(((long long)ng + SR_BN - 1) / SR_BN);
  const long long want = (SR_TARGET_UNITS + p->n_rb - 1) / p->n_rb;
  p->spans = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(want, p->tiles / SR_MIN_SPAN_TILES), SR_MAX_SPANS));
  const size_t entries = (size_t)p->spans * (size_t)nq * (size_t)k;
  p->off_ginv = sr_align(sizeof(float) * (size_t)nq);
  p->off_score = p->off_ginv + sr_align(sizeof(float) * (size_t)ng);
  p->off_idx = p->off_score + sr_align(sizeof(float) * entries);
  p->bytes = p->off_idx + sr_align(sizeof(int32_t) * entries);
  return true;
}

// ---- the total order ----------------------------------------------------------------------------------------------
// A higher score first, NaN above every number, -0 == +0, all NaNs equal; among equal scores the lower index first; an
// empty slot (index < 0) after everything.  sr_key maps a score to an unsigned that sorts the same way.
__device__ __forceinline__ unsigned sr_key(float s) {
  unsigned b = __float_as_uint(s);
  if (s != s) return 0xFFFFFFFFu;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ bool sr_before(float sa, long long ia, float sb, long long ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  const unsigned ka = sr_key(sa), kb = sr_key(sb);
  return ka > kb || (ka == kb && ia < ib);
}

constexpr unsigned SR_EMPTY_SCORE = 0xFF800000u, SR_EMPTY_INDEX = 0xFFFFFFFFu;   // -inf, -1

// Inserts (cs, col) into one row's sorted list of k entries, the whole wave at it: lane j holds entry j, the entries that
// stay in front of the candidate are a prefix, the others move down one slot and the last one falls off.
__device__ __forceinline__ void sr_insert(uint2* __restrict__ row_list, int k, int lane, float cs, int col) {
  wave_sync();
  uint2 e = make_uint2(SR_EMPTY_SCORE, SR_EMPTY_INDEX);
  if (lane < k) e = row_list[lane];
  const bool stays = lane < k && sr_before(__uint_as_float(e.x), (long long)(int)e.y, cs, (long long)col);
  const int pos = __popcll(__ballot(stays));
  if (pos < k) {   // wave-uniform
    if (lane >= pos && lane + 1 < k) row_list[lane + 1] = e;
    if (lane == pos) row_list[pos] = make_uint2(__float_as_uint(cs), (unsigned)col);
  }
}

// ---- phase 1 -------------------------------------------------------------------------------------------------------
// Workgroup = (128-row query block rb, gallery span sp); wave w owns rows [32 w, 32 w + 32) of the block: two 16-row MFMA
// tiles whose fragments stay in registers when dim <= 128 (HOIST).  K order, staging and MFMA sequence are
// cosine_tiled_kernel's: kb, u, element e, so a score's bits depend on its two rows and dim alone.
// Accumulator layout: acc[rt][ct][r] of lane (i = l & 15, kk = l >> 4) = row 16 rt + 4 kk + r, column 16 ct + i.
// Selection: every row has a sorted list of k (score, column) entries in LDS, private to its wave; the lane keeps its eight
// rows' k-th scores as thresholds (NaN while the list is not full: everything passes; +inf for a k-th score of NaN).
// Columns arrive in ascending order, so a score EQUAL to the threshold loses on its index: the test is one `>` per score
// and one ballot per block; only a block in which some score passes walks its candidates, one insertion at a time.
// NORM (svk_cosine_topk_norm): bit 0 = the query rows' {mean, std} table qmom is given, bit 1 = the gallery rows' gmom.  The
// selection then ranks norm_value of the raw score (score_common.h: svk_score_norm's expression, float64) in place of the
// raw score; thresholds, lists, write-out and phase 2 hold normalised values and do not know it.  A lane keeps the moment
// pairs of its eight rows in registers for the whole kernel and loads its two columns' pairs per gallery tile, next to sinv
// (the kernel is LDS-bound at two waves per SIMD, so the registers are free: DESIGN 3.19).  NORM == 0 is the plain search and
// reads neither table.
template <bool HOIST, int NORM>
__global__ __launch_bounds__(256) void search_tiles_kernel(const float* __restrict__ query, const float* __restrict__ gallery,
                                                           const float* __restrict__ qinv, const float* __restrict__ ginv,
                                                           int nq, int ng, int dim, int k, int spans, int tiles,
                                                           long long index_base, const long long* __restrict__ exclude,
                                                           float* __restrict__ ws_score, int* __restrict__ ws_idx,
                                                           const double* __restrict__ qmom, const double* __restrict__ gmom) {
  constexpr bool NORM_Q = (NORM & 1) != 0, NORM_G = (NORM & 2) != 0;
  __shared__ __attribute__((aligned(16))) float bs[2][SR_BN * SR_LD];
  __shared__ __attribute__((aligned(16))) uint2 lists[SR_BM * SR_KMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kk = lane >> 4;
  const int nkb = (dim + SR_KB - 1) / SR_KB;
  const bool vec_ok = (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(gallery)) & 15) == 0;
  const int rb = (int)(blockIdx.x / (unsigned)spans), sp = (int)(blockIdx.x - (unsigned)rb * (unsigned)spans);
  const int st_begin = (int)((long long)tiles * sp / spans), st_end = (int)((long long)tiles * (sp + 1) / spans);
  const int m0 = rb * SR_BM + wave * 32;
  uint2* const mine = lists + wave * 32 * SR_KMAX;
  for (int e = lane; e < 32 * SR_KMAX; e += 64) mine[e] = make_uint2(SR_EMPTY_SCORE, SR_EMPTY_INDEX);

  // staging assignment: thread t moves 4 float4 of the 32 x 128 block: row = (t >> 5) + 8 j, float4 column = t & 31
  const int srow = threadIdx.x >> 5, scol = (threadIdx.x & 31) * 4;
  auto fetch = [&](int st, int kb, f32x4 (&regs)[4]) {
    if (vec_ok && (kb + 1) * SR_KB <= dim) {  // workgroup-uniform: whole K block inside
      // rows past the gallery (ragged last block) re-read its last row: those columns are never candidates
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = min(st * SR_BN + srow + 8 * j, ng - 1);
        regs[j] = *reinterpret_cast<const f32x4*>(gallery + (int64_t)r * dim + kb * SR_KB + scol);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = st * SR_BN + srow + 8 * j;
        regs[j] = load4(gallery + (int64_t)r * dim, kb * SR_KB + scol, dim, r < ng, vec_ok);
      }
    }
  };
  auto stash = [&](float* buf, const f32x4 (&regs)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(buf + (srow + 8 * j) * SR_LD + scol) = regs[j];
  };

  // query fragments (dim <= 128), and per output row of this lane: 1 / norm, threshold, excluded column
  f32x4 a[2][8];
  if (HOIST) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int row = m0 + 16 * rt + i;
#pragma unroll
      for (int u = 0; u < 8; ++u) a[rt][u] = load4(query + (int64_t)row * dim, 16 * u + 4 * kk, dim, row < nq, vec_ok);
    }
  }
  float rinv[2][4], thr[2][4];
  int exc[2][4];
  double qmu[2][4], qsd[2][4];   // NORM_Q only; a row past the query reads the last row's pair and is never a candidate
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + 16 * rt + 4 * kk + r;
      rinv[rt][r] = qinv[min(row, nq - 1)];
      qmu[rt][r] = NORM_Q ? qmom[2 * (size_t)min(row, nq - 1)] : 0.0;
      qsd[rt][r] = NORM_Q ? qmom[2 * (size_t)min(row, nq - 1) + 1] : 0.0;
      thr[rt][r] = __builtin_nanf("");
      exc[rt][r] = -1;
      if (exclude && row < nq) {
        const long long ex = exclude[row];
        if (ex >= index_base && ex - index_base < (long long)ng) exc[rt][r] = (int)(ex - index_base);
      }
    }
  const bool rows_in = m0 + 32 <= nq;  // wave-uniform

  auto select = [&](const f32x4 (&accv)[2][2], int st, const float (&sinv)[2], const double (&gmu)[2],
                    const double (&gsd)[2]) __attribute__((always_inline)) {
    const bool ragged = !rows_in || (st + 1) * SR_BN > ng;  // wave-uniform
    float sc[2][2][4];
    bool pass[2][2][4];
    bool any = false;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sc[rt][ct][r] = accv[rt][ct][r] * rinv[rt][r] * sinv[ct];
          if (NORM) sc[rt][ct][r] = norm_value(sc[rt][ct][r], NORM_Q, qmu[rt][r], qsd[rt][r], NORM_G, gmu[ct], gsd[ct]);
          bool p = !(sc[rt][ct][r] <= thr[rt][r]);
          if (ragged) p = p && (m0 + 16 * rt + 4 * kk + r < nq) && (st * SR_BN + 16 * ct + i < ng);
          pass[rt][ct][r] = p;
          any = any || p;
        }
    if (__ballot(any) == 0ull) return;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          unsigned long long mask = __ballot(pass[rt][ct][r]);
          while (mask) {   // wave-uniform
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const float cs = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(sc[rt][ct][r]), l));
            const int ce = __builtin_amdgcn_readlane(exc[rt][r], l);
            const int col = st * SR_BN + 16 * ct + (l & 15);
            if (col == ce) continue;
            sr_insert(mine + (16 * rt + 4 * (l >> 4) + r) * SR_KMAX, k, lane, cs, col);
          }
        }
    wave_sync();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint2 e = mine[(16 * rt + 4 * kk + r) * SR_KMAX + k - 1];
        const float s = __uint_as_float(e.x);
        thr[rt][r] = (int)e.y < 0 ? __builtin_nanf("") : (s != s ? __builtin_inff() : s);
      }
  };

  f32x4 pre[4];
  fetch(st_begin, 0, pre);
  stash(bs[0], pre);
  __syncthreads();
  int cur = 0;
  for (int st = st_begin; st < st_end; ++st) {
    f32x4 acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float sinv[2];
    double gmu[2], gsd[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int col = st * SR_BN + 16 * ct + i;
      sinv[ct] = ginv[col < ng ? col : ng - 1];
      gmu[ct] = NORM_G ? gmom[2 * (size_t)(col < ng ? col : ng - 1)] : 0.0;
      gsd[ct] = NORM_G ? gmom[2 * (size_t)(col < ng ? col : ng - 1) + 1] : 0.0;
    }
    for (int kb = 0; kb < nkb; ++kb) {
      // prefetch the next (gallery block, K block) while this one is multiplied
      const bool last_kb = kb + 1 == nkb;
      const int nst = last_kb ? st + 1 : st, nkb_i = last_kb ? 0 : kb + 1;
      const bool more = nst < st_end;
      if (more) fetch(nst, nkb_i, pre);
      const float* b = bs[cur];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        f32x4 av[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          if (HOIST) {
            av[rt] = a[rt][u];
          } else {
            const int row = m0 + 16 * rt + i;
            av[rt] = load4(query + (int64_t)row * dim, kb * SR_KB + 16 * u + 4 * kk, dim, row < nq, vec_ok);
          }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(b + (16 * ct + i) * SR_LD + 16 * u + 4 * kk);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][0], bv[0], acc[rt][ct], 0, 0, 0);
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][1], bv[1], acc[rt][ct], 0, 0, 0);
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][2], bv[2], acc[rt][ct], 0, 0, 0);
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][3], bv[3], acc[rt][ct], 0, 0, 0);
          }
        }
      }
      if (more) stash(bs[cur ^ 1], pre);
      __syncthreads();  // everyone is done with bs[cur]; bs[cur ^ 1] is complete
      cur ^= 1;
    }
    select(acc, st, sinv, gmu, gsd);   // between two workgroup barriers: the lists are this wave's own
  }

  // this unit's partial lists: [span][query row][k], columns still local to this call's gallery
  wave_sync();
  for (int e = lane; e < 32 * k; e += 64) {
    const int rl = e / k, j = e - rl * k;
    const int row = m0 + rl;
    if (row < nq) {
      const uint2 v = mine[rl * SR_KMAX + j];
      const size_t o = ((size_t)sp * (size_t)nq + (size_t)row) * (size_t)k + (size_t)j;
      ws_score[o] = __uint_as_float(v.x);
      ws_idx[o] = (int)v.y;
    }
  }
}

// ---- phase 2 -------------------------------------------------------------------------------------------------------
// One span and no earlier list: the partial list IS the result; only the index changes form.
__global__ __launch_bounds__(256) void search_convert_kernel(const float* __restrict__ ws_score, const int* __restrict__ ws_idx,
                                                             long long n, long long index_base, float* __restrict__ out_score,
                                                             long long* __restrict__ out_idx) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int li = ws_idx[e];
    out_score[e] = ws_score[e];
    out_idx[e] = li < 0 ? -1ll : index_base + li;
  }
}

__global__ __launch_bounds__(256) void search_fill_kernel(long long n, float* __restrict__ out_score, long long* __restrict__ out_idx) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    out_score[e] = -__builtin_inff();
    out_idx[e] = -1ll;
  }
}

// One wave per query merges its `spans` sorted partial lists, and with `accumulate` the list already in the outputs: lane t
// owns the lists t, t + 64, ... with a cursor each and keeps the best of their heads; k rounds of a wave-wide "first under the
// total order" pick the result, and only the winning lane advances a cursor and looks at its heads again.  Two entries with
// the same score and index (overlapping chunks: the caller's error) are told apart by their list, so every lane agrees.
__global__ __launch_bounds__(64) void search_merge_kernel(const float* __restrict__ ws_score, const int* __restrict__ ws_idx,
                                                          int nq, int k, int spans, long long index_base, int accumulate,
                                                          float* __restrict__ out_score, long long* __restrict__ out_idx) {
  __shared__ unsigned char cursor[SR_MAX_SPANS + 1];
  __shared__ float old_s[SR_KMAX];
  __shared__ long long old_i[SR_KMAX];
  const int lane = threadIdx.x;
  const int n_lists = spans + (accumulate ? 1 : 0);
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    wave_sync();   // the previous query's reads of old_s / old_i are done
    const size_t ob = (size_t)q * (size_t)k;
    if (accumulate && lane < k) {
      old_s[lane] = out_score[ob + lane];
      old_i[lane] = out_idx[ob + lane];
    }
    for (int c = lane; c < n_lists; c += 64) cursor[c] = 0;
    wave_sync();

    float bs = 0.f;
    long long bi = -1;
    int bc = 0;
    auto rescan = [&]() {
      bi = -1;
      bs = -__builtin_inff();
      bc = 0;
      for (int c = lane; c < n_lists; c += 64) {
        const int j = cursor[c];
        if (j >= k) continue;
        float s;
        long long gi;
        if (c < spans) {
          const size_t o = ((size_t)c * (size_t)nq + (size_t)q) * (size_t)k + (size_t)j;
          const int li = ws_idx[o];
          s = ws_score[o];
          gi = li < 0 ? -1ll : index_base + li;
        } else {
          s = old_s[j];
          gi = old_i[j];
        }
        if (sr_before(s, gi, bs, bi)) {   // strict: among this lane's equal heads the lower list stays
          bs = s;
          bi = gi;
          bc = c;
        }
      }
    };
    rescan();
    for (int r = 0; r < k; ++r) {
      float ws = bs;
      long long wi = bi;
      int wc = bc;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float os = __shfl_xor(ws, m, 64);
        const long long oi = __shfl_xor(wi, m, 64);
        const int oc = __shfl_xor(wc, m, 64);
        const bool take = sr_before(os, oi, ws, wi) || (oi >= 0 && !sr_before(ws, wi, os, oi) && oc < wc);
        if (take) {
          ws = os;
          wi = oi;
          wc = oc;
        }
      }
      if (wi < 0) {   // wave-uniform: every list is exhausted
        for (int j = r + lane; j < k; j += 64) {
          out_score[ob + j] = -__builtin_inff();
          out_idx[ob + j] = -1ll;
        }
        break;
      }
      if (lane == 0) {
        out_score[ob + r] = ws;
        out_idx[ob + r] = wi;
      }
      if ((wc & 63) == lane) {   // cursor[c] is touched by its owner lane alone
        cursor[wc] = (unsigned char)(cursor[wc] + 1);
        rescan();
      }
    }
  }
}

using sr_tiles_fn = void (*)(const float*, const float*, const float*, const float*, int, int, int, int, int, int, long long,
                             const long long*, float*, int*, const double*, const double*);
// [dim <= SR_KB: the hoisted instance][NORM]
const sr_tiles_fn sr_tiles_kernels[2][4] = {
    {search_tiles_kernel<false, 0>, search_tiles_kernel<false, 1>, search_tiles_kernel<false, 2>, search_tiles_kernel<false, 3>},
    {search_tiles_kernel<true, 0>, search_tiles_kernel<true, 1>, search_tiles_kernel<true, 2>, search_tiles_kernel<true, 3>}};

// svk_cosine_topk (both tables NULL) and svk_cosine_topk_norm: one set of argument rules, one plan, one launch sequence.
int sr_search(svk_ctx* ctx, const float* d_query, int32_t n_query, const float* d_gallery, int32_t n_gallery, int32_t dim,
              int32_t k, int64_t index_base, const int64_t* d_exclude, int32_t flags, const double* d_query_moments,
              const double* d_gallery_moments, void* d_workspace, size_t workspace_bytes, float* d_top_score,
              int64_t* d_top_index) {
  SVK_REQUIRE(ctx, n_query >= 0 && n_gallery >= 0, "negative size");
  SVK_REQUIRE(ctx, dim >= 1 && dim <= 4096, "dim must be in [1, 4096]");
  SVK_REQUIRE(ctx, k >= 1 && k <= SR_KMAX, "k must be in [1, 32]");
  SVK_REQUIRE(ctx, (flags & ~1) == 0, "undefined flag bits");
  SVK_REQUIRE(ctx, index_base >= 0 && index_base <= INT64_MAX - (int64_t)n_gallery, "index_base must be >= 0 and leave room for n_gallery");
  if (n_query == 0) return SVK_OK;
  const bool accumulate = (flags & 1) != 0;
  if (n_gallery == 0 && accumulate) return SVK_OK;   // the lists stay as they are
  SVK_REQUIRE(ctx, d_top_score && d_top_index, "NULL buffer");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_top_score) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_top_index) & 7) == 0,
              "outputs must be aligned to their element size");
  const long long n_out = (long long)n_query * k;
  const unsigned flat_grid = (unsigned)std::min<long long>((n_out + 255) / 256, (long long)ctx->num_cu * 8);
  if (n_gallery == 0) {
    hipLaunchKernelGGL(search_fill_kernel, dim3(flat_grid), dim3(256), 0, ctx->stream, n_out, d_top_score,
                       reinterpret_cast<long long*>(d_top_index));
    SVK_LAUNCH_CHECK(ctx);
    return SVK_OK;
  }
  SVK_REQUIRE(ctx, d_query && d_gallery && d_workspace, "NULL buffer");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_query) | reinterpret_cast<uintptr_t>(d_gallery)) & 3) == 0,
              "rows must be 4-byte aligned");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "the workspace must be 16-byte aligned");
  SVK_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_query_moments) | reinterpret_cast<uintptr_t>(d_gallery_moments)) & 7) == 0,
              "the moment tables must be 8-byte aligned");
  sr_plan p;
  sr_make_plan(n_query, n_gallery, dim, k, &p);
  if (workspace_bytes < p.bytes)
    return svk_fail(ctx, SVK_ERR_BAD_ARG, "bad argument: workspace of %zu bytes, svk_cosine_topk_workspace_bytes asks for %zu",
                    workspace_bytes, p.bytes);
  char* const w = static_cast<char*>(d_workspace);
  float* const qinv = reinterpret_cast<float*>(w);
  float* const ginv = reinterpret_cast<float*>(w + p.off_ginv);
  float* const ws_score = reinterpret_cast<float*>(w + p.off_score);
  int* const ws_idx = reinterpret_cast<int*>(w + p.off_idx);

  svk_launch_inv_norm(ctx, d_query, n_query, dim, qinv);   // scoring.hip's pre-pass (one wave per row), here for both matrices
  svk_launch_inv_norm(ctx, d_gallery, n_gallery, dim, ginv);
  const int norm = (d_query_moments ? 1 : 0) | (d_gallery_moments ? 2 : 0);
  const sr_tiles_fn kern = sr_tiles_kernels[dim <= SR_KB ? 1 : 0][norm];
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.n_rb * p.spans)), dim3(256), 0, ctx->stream, d_query, d_gallery, qinv, ginv,
                     n_query, n_gallery, dim, k, p.spans, p.tiles, (long long)index_base,
                     reinterpret_cast<const long long*>(d_exclude), ws_score, ws_idx, d_query_moments, d_gallery_moments);
  if (p.spans == 1 && !accumulate) {
    hipLaunchKernelGGL(search_convert_kernel, dim3(flat_grid), dim3(256), 0, ctx->stream, ws_score, ws_idx, n_out,
                       (long long)index_base, d_top_score, reinterpret_cast<long long*>(d_top_index));
  } else {
    const unsigned grid = (unsigned)std::min<long long>(n_query, (long long)ctx->num_cu * 32);
    hipLaunchKernelGGL(search_merge_kernel, dim3(grid), dim3(64), 0, ctx->stream, ws_score, ws_idx, n_query, k, p.spans,
                       (long long)index_base, accumulate ? 1 : 0, d_top_score, reinterpret_cast<long long*>(d_top_index));
  }
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // namespace

extern "C" {

size_t svk_cosine_topk_workspace_bytes(int32_t n_query, int32_t n_gallery, int32_t dim, int32_t k) {
  sr_plan p;
  return sr_make_plan(n_query, n_gallery, dim, k, &p) ? p.bytes : 0;
}

int svk_cosine_topk(svk_ctx* ctx, const float* d_query, int32_t n_query, const float* d_gallery, int32_t n_gallery,
                    int32_t dim, int32_t k, int64_t index_base, const int64_t* d_exclude, int32_t flags, void* d_workspace,
                    size_t workspace_bytes, float* d_top_score, int64_t* d_top_index) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  return sr_search(ctx, d_query, n_query, d_gallery, n_gallery, dim, k, index_base, d_exclude, flags, nullptr, nullptr, d_workspace,
                   workspace_bytes, d_top_score, d_top_index);
}

size_t svk_cosine_topk_norm_workspace_bytes(int32_t n_query, int32_t n_gallery, int32_t dim, int32_t k) {
  return svk_cosine_topk_workspace_bytes(n_query, n_gallery, dim, k);
}

int svk_cosine_topk_norm(svk_ctx* ctx, const float* d_query, int32_t n_query, const float* d_gallery, int32_t n_gallery,
                         int32_t dim, int32_t k, int64_t index_base, const int64_t* d_exclude, int32_t flags,
                         const double* d_query_moments, const double* d_gallery_moments, void* d_workspace,
                         size_t workspace_bytes, float* d_top_score, int64_t* d_top_index) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, d_query_moments || d_gallery_moments,
              "no moment table: give the query table, the gallery table or both (svk_cosine_topk ranks raw scores)");
  return sr_search(ctx, d_query, n_query, d_gallery, n_gallery, dim, k, index_base, d_exclude, flags, d_query_moments,
                   d_gallery_moments, d_workspace, workspace_bytes, d_top_score, d_top_index);
}

}  // extern "C"
