// Adaptive score normalisation (include/svk.h "score normalisation"): the mean and standard deviation of the top_k largest
// scores of every row of a rows x cohort score matrix, and the Z- / T- / S-norm built on them.  The reference has neither (its
// scores are raw cosines); on a framework the moments are a top-k selection that writes K values per row, a conversion and
// two reductions over them.
//
// svk_cohort_moments gives every row ONE team -- a wave for rows up to WAVE_ROW_MAX columns (four rows per workgroup), a
// 256-thread workgroup above -- and walks the row six times: four radix-select passes over the order-preserving key of
// roc.hip / search.hip (an LDS histogram of one 8-bit digit each, most significant first: the m-th largest key, exactly), then
// the sum and the centred squares of what lies strictly above it; the copies of the m-th largest value itself enter as ONE
// term each time, so no index decides between equal values.  A row of up to ROW_LDS_MAX columns is read from memory once, as
// keys into LDS; a longer one goes through the same LDS buffer ROW_LDS_MAX columns at a time in every pass.  Lane l of the
// team owns the columns l, l + T, .. on both routes and with both load widths: one order of additions, the one svk.h states.
#include "score_common.h"
#include "svk_internal.h"

namespace {

constexpr int RT = 256;                   // threads per workgroup, whatever the team
constexpr int WAVE_ROW_MAX = 2048;        // a row of up to this many columns is one wave's (8 KiB of keys; measured: DESIGN 3.14)
constexpr int ROW_LDS_MAX = 16384;        // columns of a row kept in LDS: 64 KiB, two workgroups to a CU's 160 KiB
constexpr int ROW_BATCH = 4;              // keys a lane reads from LDS before it works on them
static_assert(ROW_LDS_MAX % RT == 0 && WAVE_ROW_MAX % 64 == 0, "a lane's columns keep their order across LDS chunks");

// sr_key's map for the candidates, 0 for everything else: a finite score's key is never 0 (that would be a negative NaN),
// -0.0 gets +0.0's key, and a larger score has the larger key.
__device__ __forceinline__ unsigned cand_key(unsigned b) {
  if ((b & 0x7f800000u) == 0x7f800000u) return 0u;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cand_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int TEAM>
__device__ __forceinline__ void team_sync() {
  if (TEAM == 64)
    wave_sync();
  else
    __syncthreads();
}

// Columns [c0, c0 + len) of the row as keys into LDS.  VEC: the row starts on a 16-byte boundary (and c0 % 4 == 0): one
// 16-byte load per whole quad inside the row, guarded 4-byte loads for the last one; else 4-byte loads.
template <int TEAM, bool VEC>
__device__ __forceinline__ void stage_keys(const unsigned* __restrict__ row, long long c0, int len, unsigned* keys, int t) {
  if (VEC) {
    for (int q = 4 * t; q < len; q += 4 * TEAM) {
      unsigned k[4] = {0u, 0u, 0u, 0u};            // the padding of the last quad: key 0, no candidate
      if (q + 4 <= len) {
        const uint4 u = *reinterpret_cast<const uint4*>(row + c0 + q);
        k[0] = cand_key(u.x), k[1] = cand_key(u.y), k[2] = cand_key(u.z), k[3] = cand_key(u.w);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (q + e < len) k[e] = cand_key(row[c0 + q + e]);
      }
      *reinterpret_cast<uint4*>(keys + q) = make_uint4(k[0], k[1], k[2], k[3]);
    }
  } else {
    for (int i = t; i < len; i += TEAM) keys[i] = cand_key(row[c0 + i]);
  }
}

// f(key) for the lane's columns t, t + TEAM, .. in column order; a column past the row reads as key 0 (no candidate), so
// that every lane of a wave makes the same number of calls.  resident: the whole row is in `keys` already.
template <int TEAM, bool VEC, class F>
__device__ __forceinline__ void for_row(const unsigned* __restrict__ row, int n, unsigned* keys, bool resident, int t, F f) {
  for (long long c0 = 0; c0 < n; c0 += ROW_LDS_MAX) {
    const int len = (int)min((long long)ROW_LDS_MAX, n - c0);
    if (!resident) {
      team_sync<TEAM>();                 // the chunk before this one has been read
      stage_keys<TEAM, VEC>(row, c0, len, keys, t);
      team_sync<TEAM>();
    }
    // ROW_BATCH LDS reads in flight, then their calls in column order (a call with key 0 does nothing: +0.0 moves no bit)
    for (int i = t; i - t < len; i += ROW_BATCH * TEAM) {
      unsigned k[ROW_BATCH];
#pragma unroll
      for (int u = 0; u < ROW_BATCH; ++u) k[u] = i + u * TEAM < len ? keys[i + u * TEAM] : 0u;
#pragma unroll
      for (int u = 0; u < ROW_BATCH; ++u) f(k[u]);
    }
  }
}

// The sum over the team, the same value in every thread: a 64-lane xor butterfly, then (workgroup team) the four wave sums
// from 0.0 in wave order.
template <int TEAM>
__device__ __forceinline__ double team_sum(double v, double* red, int t) {
  v = wave_sum(v);
  if (TEAM == 64) return v;
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < TEAM / 64; ++i) s += red[i];
  __syncthreads();
  return s;
}

template <int O>
__device__ __forceinline__ unsigned row_shl(unsigned v) {      // lane i reads lane i + O of its row of 16, 0 past its end
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + O, 0xf, 0xf, true);
}
// v of this lane and of every higher lane of the wave: a shift-and-add inside each row of 16 lanes on the DPP path, then the
// totals of the rows above.  No LDS round trip.
__device__ __forceinline__ unsigned suffix_sum(unsigned v, int lane) {
  v += row_shl<1>(v);
  v += row_shl<2>(v);
  v += row_shl<4>(v);
  v += row_shl<8>(v);
  const unsigned t1 = __builtin_amdgcn_readlane(v, 16), t2 = __builtin_amdgcn_readlane(v, 32), t3 = __builtin_amdgcn_readlane(v, 48);
  const int row = lane >> 4;
  return v + (row == 0 ? t1 + t2 + t3 : row == 1 ? t2 + t3 : row == 2 ? t3 : 0u);
}

// The digit holding the r-th largest of the candidates counted in h[256] (1 <= r <= their number) and r less the candidates in
// higher digits; every wave of the team works it out for itself, the same values in all lanes.  Lane l owns the bins 4 l .. 4 l
// + 3.  first: the top digit's pass, which fixes m = min(top_k, candidates) (top_k == 0: all) and starts from r = m; m == 0
// gives r = 0.
struct Pick {
  unsigned digit, r, m;
};
__device__ __forceinline__ Pick pick_digit(const unsigned* h, unsigned r, int top_k, bool first, int lane) {
  const uint4 c4 = *reinterpret_cast<const uint4*>(h + 4 * lane);
  const unsigned c[4] = {c4.x, c4.y, c4.z, c4.w};
  const unsigned own = c[0] + c[1] + c[2] + c[3];
  const unsigned incl = suffix_sum(own, lane);
  unsigned m = 0u;
  if (first) {
    const unsigned total = __builtin_amdgcn_readlane(incl, 0);
    r = m = (top_k > 0 && (unsigned)top_k < total) ? (unsigned)top_k : total;
  }
  unsigned above = incl - own, digit = 0u, left = 0u;       // `above`: the candidates in higher bins
#pragma unroll
  for (int b = 3; b >= 0; --b) {
    const bool hit = above < r && r <= above + c[b];        // true in exactly one lane and bin when r >= 1
    digit = hit ? 4u * lane + b : digit;
    left = hit ? r - above : left;
    above += c[b];
  }
  const unsigned long long who = __ballot(left != 0u);
  if (who == 0ull) return Pick{0u, 0u, m};
  const int src = __ffsll((long long)who) - 1;
  return Pick{(unsigned)__builtin_amdgcn_readlane(digit, src), (unsigned)__builtin_amdgcn_readlane(left, src), m};
}

template <int TEAM, bool VEC>
__global__ __launch_bounds__(RT) void cohort_moments_kernel(const unsigned* __restrict__ scores, long long n_rows, int n,
                                                            long long row_stride, int top_k, double* __restrict__ moments,
                                                            int* __restrict__ used, float* __restrict__ kth, int cap) {
  constexpr int TEAMS = RT / TEAM;
  // a wave-sized team orders its passes over ONE histogram by itself; a workgroup has one per pass, zeroed up front, so that
  // a pass costs it one barrier
  constexpr int HISTS = TEAM == 64 ? 1 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned key_lds[];     // [TEAMS][cap]
  __shared__ __attribute__((aligned(16))) unsigned hist[TEAMS][HISTS][256];
  __shared__ double red_lds[TEAMS][RT / 64];
  const int team = threadIdx.x / TEAM, t = threadIdx.x % TEAM, lane = threadIdx.x & 63;
  const long long r_idx = (long long)blockIdx.x * TEAMS + team;
  if (r_idx >= n_rows) return;           // a whole team (a wave-sized one) leaves; it shares no barrier with the others
  const unsigned* row = scores + (size_t)r_idx * (size_t)row_stride;
  unsigned* keys = key_lds + (size_t)team * cap;
  double* red = red_lds[team];
  const bool resident = n <= ROW_LDS_MAX;
  unsigned* all_hists = &hist[team][0][0];
  for (int i = t; i < HISTS * 256; i += TEAM) all_hists[i] = 0u;
  if (resident) stage_keys<TEAM, VEC>(row, 0, n, keys, t);
  team_sync<TEAM>();

  // ---- the m-th largest key: four digits, most significant first --------------------------------------------------------
  unsigned prefix = 0u, mask = 0u, r = 0u, m = 0u;
#pragma unroll 1
  for (int p = 3; p >= 0; --p) {
    unsigned* h = hist[team][HISTS == 1 ? 0 : p];
    if (HISTS == 1 && p < 3) {
      for (int i = t; i < 256; i += TEAM) h[i] = 0u;
      team_sync<TEAM>();
    }
    const int shift = 8 * p;
    for_row<TEAM, VEC>(row, n, keys, resident, t, [&](unsigned k) {
      const bool valid = k != 0u && (k & mask) == prefix;
      const unsigned long long act = __ballot(valid);
      if (act == 0ull) return;
      const unsigned d = (k >> shift) & 255u;
      // a digit that all of the wave's candidates share (clustered scores) is one add, not 64 conflicting ones
      const int first = __ffsll((long long)act) - 1;
      const unsigned d0 = __builtin_amdgcn_readlane(d, first);
      if (__ballot(valid && d == d0) == act) {
        if (lane == first) atomicAdd(&h[d0], (unsigned)__popcll(act));
      } else if (valid) {
        atomicAdd(&h[d], 1u);
      }
    });
    team_sync<TEAM>();
    const Pick pick = pick_digit(h, r, top_k, p == 3, lane);
    if (p == 3) m = pick.m;
    r = pick.r;
    if (r == 0u) break;                  // no candidate: team-uniform, only in the first pass
    prefix |= pick.digit << shift;
    mask |= 255u << shift;
  }
  if (m == 0u) {
    if (t == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      moments[2 * r_idx] = nan, moments[2 * r_idx + 1] = nan;
      if (used) used[r_idx] = 0;
      if (kth) kth[r_idx] = __uint_as_float(0x7fc00000u);
    }
    return;
  }

  // ---- moments of the multiset: everything above the key `prefix`, and r copies of its value -------------------------------
  const double vstar = (double)cand_value(prefix);
  double mean = vstar, sd = 0.0;         // all m selected values equal: the value itself, +0.0
  if (m != r) {
#pragma clang fp contract(off)
    double acc = 0.0;                    // (a key that is not selected adds + 0.0, which moves no bit)
    for_row<TEAM, VEC>(row, n, keys, resident, t, [&](unsigned k) { acc += k > prefix ? (double)cand_value(k) : 0.0; });
    const double s = team_sum<TEAM>(acc, red, t) + (double)r * vstar;
    mean = s / (double)m;
    acc = 0.0;
    for_row<TEAM, VEC>(row, n, keys, resident, t, [&](unsigned k) {
#pragma clang fp contract(off)
      const double d = (double)cand_value(k) - mean;
      acc += k > prefix ? d * d : 0.0;
    });
    const double dv = vstar - mean;
    const double q = team_sum<TEAM>(acc, red, t) + (double)r * (dv * dv);
    sd = sqrt(q / (double)m);
  }
  if (t == 0) {
    moments[2 * r_idx] = mean, moments[2 * r_idx + 1] = sd;
    if (used) used[r_idx] = (int)m;
    if (kth) kth[r_idx] = cand_value(prefix);
  }
}

// Four consecutive columns of one row per thread; workgroup b = row b / tiles, columns 4 RT (b % tiles) onwards.  Every load
// of a thread precedes its stores and no other thread touches its entries: d_out may be the scores themselves.
template <bool VEC>
__global__ __launch_bounds__(RT) void score_norm_kernel(const float* sc, int n_cols, size_t row_stride, unsigned tiles,
                                                        const double* __restrict__ mom_r, const double* __restrict__ mom_c,
                                                        float* out, size_t out_stride) {
  const size_t row = blockIdx.x / tiles;
  const long long c0 = 4ll * ((long long)(blockIdx.x % tiles) * RT + threadIdx.x);
  if (c0 >= n_cols) return;
  const bool has_r = mom_r != nullptr, has_c = mom_c != nullptr;
  const double mu_r = has_r ? mom_r[2 * row] : 0.0, sd_r = has_r ? mom_r[2 * row + 1] : 0.0;
  const float* src = sc + row * row_stride + c0;
  float* dst = out + row * out_stride + c0;
  const bool whole = c0 + 4 <= n_cols;
  float s[4], v[4];
  if (VEC && whole) {
    const float4 u = *reinterpret_cast<const float4*>(src);
    s[0] = u.x, s[1] = u.y, s[2] = u.z, s[3] = u.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = c0 + e < n_cols ? src[e] : 0.0f;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = c0 + e < n_cols;
    const double mu_c = has_c && in ? mom_c[2 * (c0 + e)] : 0.0, sd_c = has_c && in ? mom_c[2 * (c0 + e) + 1] : 0.0;
    v[e] = norm_value(s[e], has_r, mu_r, sd_r, has_c, mu_c, sd_c);
  }
  if (VEC && whole) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + e < n_cols) dst[e] = v[e];
  }
}

// Four consecutive trials per thread.  A table that is not given is not indexed (its index list may be NULL); an index
// outside a given table reads nothing, makes that trial NaN and counts.
template <bool VEC>
__global__ __launch_bounds__(RT) void score_norm_pairs_kernel(const float* sc, size_t n, const double* __restrict__ mom_a,
                                                              long long n_a, const double* __restrict__ mom_b, long long n_b,
                                                              const long long* __restrict__ idx_a,
                                                              const long long* __restrict__ idx_b, float* out,
                                                              int* __restrict__ bad_count) {
  const size_t i0 = 4 * ((size_t)blockIdx.x * RT + threadIdx.x);
  if (i0 >= n) return;
  const bool has_a = mom_a != nullptr, has_b = mom_b != nullptr, whole = i0 + 4 <= n;
  float s[4], v[4];
  if (VEC && whole) {
    const float4 u = *reinterpret_cast<const float4*>(sc + i0);
    s[0] = u.x, s[1] = u.y, s[2] = u.z, s[3] = u.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = i0 + e < n ? sc[i0 + e] : 0.0f;
  }
  int bad = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = i0 + e < n;
    const long long ia = has_a && in ? idx_a[i0 + e] : 0, ib = has_b && in ? idx_b[i0 + e] : 0;
    const bool ok = (!has_a || (ia >= 0 && ia < n_a)) && (!has_b || (ib >= 0 && ib < n_b));
    const bool rd = in && ok;
    const double mu_a = has_a && rd ? mom_a[2 * ia] : 0.0, sd_a = has_a && rd ? mom_a[2 * ia + 1] : 0.0;
    const double mu_b = has_b && rd ? mom_b[2 * ib] : 0.0, sd_b = has_b && rd ? mom_b[2 * ib + 1] : 0.0;
    v[e] = ok ? norm_value(s[e], has_a, mu_a, sd_a, has_b, mu_b, sd_b) : __uint_as_float(0x7fc00000u);
    bad += in && !ok;
  }
  if (VEC && whole) {
    *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < n) out[i0 + e] = v[e];
  }
  if (bad && bad_count) atomicAdd(bad_count, bad);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int svk_cohort_moments(svk_ctx* ctx, const float* d_scores, int64_t n_rows, int32_t n_cohort, int64_t row_stride, int32_t top_k,
                       double* d_moments, int32_t* d_used, float* d_kth) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rows >= 0, "negative size");
  SVK_REQUIRE(ctx, n_cohort >= 1, "n_cohort below 1");
  SVK_REQUIRE(ctx, top_k >= 0, "negative top_k");
  SVK_REQUIRE(ctx, row_stride >= n_cohort, "row_stride below n_cohort");
  if (n_rows == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_scores && d_moments, "NULL buffer");
  SVK_REQUIRE(ctx, aligned(d_scores, 4) && aligned(d_moments, 8) && aligned(d_used, 4) && aligned(d_kth, 4),
              "misaligned buffer (f32 / int32: 4 bytes; float64: 8)");
  const bool wave_team = n_cohort <= WAVE_ROW_MAX;
  const int teams = wave_team ? RT / 64 : 1;
  const int64_t blocks = (n_rows + teams - 1) / teams;
  SVK_REQUIRE(ctx, blocks <= 0x7fffffff, "n_rows beyond 2^31 workgroups");
  const int cap = (std::min<int>(n_cohort, ROW_LDS_MAX) + 3) & ~3;
  const size_t lds = (size_t)teams * cap * sizeof(unsigned);
  const bool vec = aligned(d_scores, 16) && row_stride % 4 == 0;
  using Kernel = void (*)(const unsigned*, long long, int, long long, int, double*, int*, float*, int);
  const Kernel kern = wave_team ? (vec ? cohort_moments_kernel<64, true> : cohort_moments_kernel<64, false>)
                                : (vec ? cohort_moments_kernel<RT, true> : cohort_moments_kernel<RT, false>);
  if (lds > 32 * 1024)
    SVK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(RT), lds, ctx->stream, reinterpret_cast<const unsigned*>(d_scores),
                     (long long)n_rows, (int)n_cohort, (long long)row_stride, (int)top_k, d_moments, d_used, d_kth, cap);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_score_norm(svk_ctx* ctx, const float* d_scores, int64_t n_rows, int64_t n_cols, int64_t row_stride,
                   const double* d_row_moments, const double* d_col_moments, float* d_out, int64_t out_stride) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rows >= 0 && n_cols >= 0, "negative size");
  SVK_REQUIRE(ctx, n_cols <= 0x7fffffff, "n_cols beyond 2^31 - 1");
  SVK_REQUIRE(ctx, row_stride >= n_cols && out_stride >= n_cols, "a stride below n_cols");
  SVK_REQUIRE(ctx, d_row_moments || d_col_moments, "no moment table: give the row table, the column table or both");
  if (n_rows == 0 || n_cols == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_scores && d_out, "NULL buffer");
  SVK_REQUIRE(ctx, d_out != d_scores || out_stride == row_stride, "in place wants out_stride == row_stride");
  SVK_REQUIRE(ctx, aligned(d_scores, 4) && aligned(d_out, 4) && aligned(d_row_moments, 8) && aligned(d_col_moments, 8),
              "misaligned buffer (f32: 4 bytes; float64: 8)");
  const int64_t tiles = (n_cols + 4 * RT - 1) / (4 * RT);
  SVK_REQUIRE(ctx, n_rows <= 0x7fffffff / tiles, "n_rows x column tiles beyond 2^31 workgroups");
  const bool vec = aligned(d_scores, 16) && aligned(d_out, 16) && row_stride % 4 == 0 && out_stride % 4 == 0;
  hipLaunchKernelGGL(vec ? score_norm_kernel<true> : score_norm_kernel<false>, dim3((unsigned)(n_rows * tiles)), dim3(RT), 0,
                     ctx->stream, d_scores, (int)n_cols, (size_t)row_stride, (unsigned)tiles, d_row_moments, d_col_moments, d_out,
                     (size_t)out_stride);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_score_norm_pairs(svk_ctx* ctx, const float* d_scores, int64_t n, const double* d_mom_a, int64_t n_a,
                         const double* d_mom_b, int64_t n_b, const int64_t* d_idx_a, const int64_t* d_idx_b, float* d_out,
                         int32_t* d_bad_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 0 && n_a >= 0 && n_b >= 0, "negative size");
  SVK_REQUIRE(ctx, d_mom_a || d_mom_b, "no moment table: give table a, table b or both");
  if (n == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_scores && d_out, "NULL buffer");
  SVK_REQUIRE(ctx, (!d_mom_a || d_idx_a) && (!d_mom_b || d_idx_b), "a moment table without its index list");
  SVK_REQUIRE(ctx, aligned(d_scores, 4) && aligned(d_out, 4) && aligned(d_bad_count, 4) && aligned(d_mom_a, 8) &&
                       aligned(d_mom_b, 8) && aligned(d_idx_a, 8) && aligned(d_idx_b, 8),
              "misaligned buffer (f32 / int32: 4 bytes; float64 / int64: 8)");
  const size_t blocks = (((size_t)n + 3) / 4 + RT - 1) / RT;
  SVK_REQUIRE(ctx, blocks <= 0x7fffffffu, "n beyond 2^41");
  const bool vec = aligned(d_scores, 16) && aligned(d_out, 16);
  hipLaunchKernelGGL(vec ? score_norm_pairs_kernel<true> : score_norm_pairs_kernel<false>, dim3((unsigned)blocks), dim3(RT), 0,
                     ctx->stream, d_scores, (size_t)n, d_mom_a, (long long)n_a, d_mom_b, (long long)n_b,
                     reinterpret_cast<const long long*>(d_idx_a), reinterpret_cast<const long long*>(d_idx_b), d_out,
                     d_bad_count);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
