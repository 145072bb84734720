// ROC / EER / AUC on the device: what /root/reference/evaluation.py:11-52 gets from
// sklearn.roc_curve + roc_auc_score + brentq(interp1d) -- one sort of all (label, score) pairs --
// for score sets too large to bring back to the host (148 642 x 1 211 = 1.8e8 pairs), and the top-1
// pass of evaluation.py:112-134 (argmax per row, hits, one-hot labels).
//
// Every kernel is this file's own; nothing waits on another workgroup.  Per split of m pairs:
//   1. hist_kernel: the four 8-bit digit histograms of the keys, the non-finite scores and the positives,
//      read back to the host (argument checks; a pass whose digit is the same for every key is skipped).
//   2. LSD radix sort, descending, the 0/1 label riding along: per pass count_kernel (digit counts of
//      each workgroup's contiguous span), offsets_kernel (each digit's row of the [256][grid] count matrix
//      scanned by one workgroup, on top of the keys of lower digits) and scatter_kernel (the span again, tile by tile, stable: wave-level digit match
//      + per-(item, wave) counts give each key its rank; the tile is ordered in LDS and written out
//      in digit runs at running per-digit offsets).  Keys: f32 -> u32 order-preserving map, inverted;
//      -0.0 is +0.0 first (one tie group, as sklearn and the float compare below see them).
//   3. the ROC's threshold points (one per distinct score, roc_curve before drop_intermediate) by the
//      same reduce-then-scan: span sums of (label, boundary flag), a scan, then a pass that writes
//      (fps, tps) at every boundary.
//   4. roc_points_kernel: trapezoid area (AUC) and the segment where 1 - fpr - tpr changes sign,
//      solved linearly (the root brentq finds on the linear interpolant).
//      Each workgroup leaves its share of the area in the workspace; roc_finish_kernel, ONE workgroup, adds the shares in a
//      fixed order (the AUC is the same bits on every run and from every entry point) and looks up the score at the upper end
//      of the EER segment.
//   5. svk_roc_k only: roc_curve's drop_intermediate (second differences of fps, tps) and its
//      prepended origin, compacted by the same pattern into the caller's curve planes.
//   6. svk_roc_dcf only: dcf_part_kernel, one pass over the origin + the distinct-score points that leaves every workgroup's
//      (cost, index) minimum per operating point in the workspace; roc_finish_kernel reduces them (no float64 atomics, no
//      workgroup waits on another).  The first point among equal costs wins: the highest threshold.
//   7. svk_rocch only (include/svk.h "the ROC convex hull", kernels in rocch.h): behind roc_finish_kernel, the upper convex hull of the origin +
//      the points, exact in int64: one hull per tile of 2 048 points (a monotone chain per thread, 8 merge levels in LDS), then
//      ceil(log2(tiles)) levels that join adjacent hulls pairwise by their bridge; the vertices' scores come from the sorted keys.
// svk_pav_apply (same header) maps scores through a step table by one binary search each.
// svk_decision_counts is a pass of its own over UNSORTED scores: accepted targets / non-targets at up to 16 thresholds.
// Bit-level equality of eer / auc with sklearn is not expected (float64 accumulation order), |d| ~ 1e-15;
// the curve counts are exact.  Element indices are u32 (n < 2^32), every address is 64-bit.
#include "svk_internal.h"

namespace {

constexpr int RT = 256;                  // threads per workgroup (all but scan_kernel and offsets_kernel)
constexpr int WAVES = RT / 64;
constexpr int ITEMS = 8;                 // keys per thread per scatter tile
constexpr int TILE = RT * ITEMS;         // 2048 keys
constexpr int GROUPS = ITEMS * WAVES;    // (item, wave) groups of a tile, in stable order
constexpr int SPAN_ITEMS = 4;            // elements per thread per step of the point / curve passes
constexpr unsigned GMAX = 1024;          // workgroups of a span-parallel kernel (count matrix [256][GMAX])
constexpr int SCAN_T = 1024;
constexpr unsigned PMAX = 2048;          // workgroups of a pass over the ROC points (their partial results: [PMAX] rows)
constexpr int DCF_MAX_OPS = 8;           // operating points of one svk_roc_dcf call
constexpr int DC_MAX_THR = 16;           // thresholds of one svk_decision_counts call

__device__ __forceinline__ unsigned desc_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;                      // -0.0 -> +0.0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);    // ascending order-preserving map
  return ~u;                                         // descending
}
__device__ __forceinline__ float key_value(unsigned k) {
  const unsigned a = ~k;
  return __uint_as_float((a & 0x80000000u) ? (a & 0x7fffffffu) : ~a);
}

// Lanes of this wave holding the same 8-bit digit (only meaningful for valid lanes).
__device__ __forceinline__ unsigned long long match_digit(unsigned d, bool valid) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}
__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << __lane_id()) - 1ull; }

// Exclusive scan of one value per thread over an NT-wide workgroup; *total gets the sum.  lds: NT / 64 words.
template <int NT = RT>
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* lds, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds[w] = x;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const unsigned c = lds[i];
    base += i < w ? c : 0u;
    tot += c;
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}

// ---- 1. digit histograms + argument counts -------------------------------------------------------------------
// hist[p * 256 + d] for the four digits p, hist[1024] = non-finite scores, hist[1025] = positives.
__global__ __launch_bounds__(RT) void hist_kernel(const unsigned* __restrict__ bits, const uint8_t* __restrict__ lab, size_t n,
                                                  unsigned* __restrict__ hist) {
  __shared__ unsigned h[4 * 256];
  for (int i = threadIdx.x; i < 4 * 256; i += RT) h[i] = 0;
  __syncthreads();
  unsigned bad = 0, pos = 0;
  const size_t stride = (size_t)gridDim.x * RT;
  for (size_t b = (size_t)blockIdx.x * RT; b < n; b += stride) {   // wave-uniform trip count
    const size_t i = b + threadIdx.x;
    const bool valid = i < n;
    unsigned k = 0;
    if (valid) {
      const unsigned u = bits[i];
      bad += (u & 0x7f800000u) == 0x7f800000u;
      pos += lab[i] != 0;
      k = desc_key(u);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned d = (k >> (8 * p)) & 255u;
      // a digit the whole wave shares (clustered scores) is one add, not 64 conflicting ones
      const unsigned d0 = __shfl(d, 0, 64);
      const unsigned long long same = __ballot(valid && d == d0), act = __ballot(valid);
      if (same == act) {
        if (__lane_id() == 0 && act) atomicAdd(&h[p * 256 + d0], (unsigned)__popcll(act));
      } else if (valid) {
        atomicAdd(&h[p * 256 + d], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * 256; i += RT)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  __shared__ unsigned red[2 * WAVES];
  bad = (unsigned)wave_sum((long long)bad);
  pos = (unsigned)wave_sum((long long)pos);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = bad;
    red[WAVES + (threadIdx.x >> 6)] = pos;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned b = 0, q = 0;
    for (int i = 0; i < WAVES; ++i) {
      b += red[i];
      q += red[WAVES + i];
    }
    if (b) atomicAdd(&hist[1024], b);
    atomicAdd(&hist[1025], q);
  }
}

// ---- 2. one radix pass: count, scan, scatter -------------------------------------------------------------------
// counts[d * G + g] = keys of workgroup g's span [g * span, (g + 1) * span) whose digit is d.  raw: the source is the
// caller's f32 scores (the first pass that runs), else keys already mapped.
__global__ __launch_bounds__(RT) void count_kernel(const unsigned* __restrict__ src, int raw, size_t n, size_t span, int shift,
                                                   unsigned* __restrict__ counts) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const size_t lo = (size_t)blockIdx.x * span, hi = std::min(n, lo + span);
  constexpr int U = 8;
  for (size_t b = lo; b < hi; b += (size_t)RT * U) {
    unsigned k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = b + (size_t)u * RT + threadIdx.x;
      k[u] = i < hi ? src[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = b + (size_t)u * RT + threadIdx.x < hi;
      const unsigned d = ((raw ? desc_key(k[u]) : k[u]) >> shift) & 255u;
      const unsigned long long peers = match_digit(d, valid);
      if (valid && !(peers & lanes_below())) atomicAdd(&h[d], (unsigned)__popcll(peers));
    }
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// In-place exclusive scan of data[0, len) (the [grid] partial sums of a span pass) by one workgroup; *total (if given) =
// the sum.  Each thread owns a contiguous chunk.
__global__ __launch_bounds__(SCAN_T) void scan_kernel(unsigned* __restrict__ data, unsigned len, unsigned* __restrict__ total) {
  __shared__ unsigned part[SCAN_T];
  const unsigned per = (len + SCAN_T - 1) / SCAN_T;
  const unsigned lo = std::min(len, threadIdx.x * per), hi = std::min(len, lo + per);
  unsigned s = 0;
  for (unsigned i = lo; i < hi; ++i) s += data[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (unsigned o = 1; o < SCAN_T; o <<= 1) {   // Hillis-Steele, inclusive
    const unsigned y = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
    __syncthreads();
    part[threadIdx.x] += y;
    __syncthreads();
  }
  unsigned base = part[threadIdx.x] - s;
  for (unsigned i = lo; i < hi; ++i) {
    const unsigned v = data[i];
    data[i] = base;
    base += v;
  }
  if (total && threadIdx.x == SCAN_T - 1) *total = part[SCAN_T - 1];
}

// offs[d * G + g] = keys whose digit is below d (the pass's global histogram dh, from hist_kernel) + keys of digit d in
// the spans before g: one workgroup per digit, one span per thread (G <= GMAX).
__global__ __launch_bounds__(GMAX) void offsets_kernel(unsigned* __restrict__ counts, unsigned G, const unsigned* __restrict__ dh) {
  __shared__ unsigned red[GMAX / 64];
  const unsigned d = blockIdx.x, t = threadIdx.x;
  unsigned below, tot;
  block_excl_scan<GMAX>(t < d ? dh[t] : 0u, red, &below);
  const unsigned v = t < G ? counts[(size_t)d * G + t] : 0u;
  const unsigned ex = block_excl_scan<GMAX>(v, red, &tot);
  if (t < G) counts[(size_t)d * G + t] = below + ex;
}

// Stable scatter of workgroup g's span to dst at offs[d * G + g] (the scanned counts), tile by tile.
__global__ __launch_bounds__(RT) void scatter_kernel(const unsigned* __restrict__ src, const uint8_t* __restrict__ vsrc, int raw,
                                                     size_t n, size_t span, int shift, const unsigned* __restrict__ offs,
                                                     unsigned* __restrict__ dst, uint8_t* __restrict__ vdst) {
  __shared__ unsigned short cnt[GROUPS][256];   // per (item, wave) group and digit: count, then exclusive offset
  __shared__ unsigned sk[TILE];
  __shared__ uint8_t sv[TILE];
  __shared__ unsigned run[256], tstart[256], red[WAVES];
  const int t = threadIdx.x, w = t >> 6;
  run[t] = offs[(size_t)t * gridDim.x + blockIdx.x];
  const size_t lo = (size_t)blockIdx.x * span, hi = std::min(n, lo + span);
  for (size_t base = lo; base < hi; base += TILE) {
    const unsigned tn = (unsigned)std::min((size_t)TILE, hi - base);
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) cnt[g][t] = 0;
    unsigned key[ITEMS], rank[ITEMS];
    uint8_t val[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const unsigned e = it * RT + t;
      key[it] = 0;
      val[it] = 0;
      if (e < tn) {
        key[it] = src[base + e];
        val[it] = vsrc[base + e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const bool valid = it * RT + t < (int)tn;
      if (raw) {
        key[it] = desc_key(key[it]);
        val[it] = val[it] != 0;
      }
      const unsigned d = (key[it] >> shift) & 255u;
      const unsigned long long peers = match_digit(d, valid);
      rank[it] = (unsigned)__popcll(peers & lanes_below());
      if (valid && rank[it] == 0) cnt[it * WAVES + w][d] = (unsigned short)__popcll(peers);
    }
    __syncthreads();
    unsigned s = 0;   // thread t = digit t: offsets of the groups in stable order
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
      const unsigned c = cnt[g][t];
      cnt[g][t] = (unsigned short)s;
      s += c;
    }
    unsigned tot;
    tstart[t] = block_excl_scan(s, red, &tot);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      if (it * RT + t < (int)tn) {
        const unsigned d = (key[it] >> shift) & 255u;
        const unsigned lp = tstart[d] + cnt[it * WAVES + w][d] + rank[it];
        sk[lp] = key[it];
        sv[lp] = val[it];
      }
    }
    __syncthreads();
    for (unsigned i = t; i < tn; i += RT) {
      const unsigned k = sk[i], d = (k >> shift) & 255u;
      const size_t gp = (size_t)run[d] + (i - tstart[d]);
      dst[gp] = k;
      vdst[gp] = sv[i];
    }
    __syncthreads();
    run[t] += s;
  }
}

// ---- 3 / 5. span reduce-then-scan over the sorted pairs and over the ROC points ---------------------------------
// An Op yields two 0/1 values per element, (a, b); part_kernel sums them over each workgroup's span, emit_kernel
// walks the span again and hands each element its global inclusive prefix sums.
struct PointsOp {   // sorted pairs -> one point per distinct score: a = label, b = last of its tie group
  const unsigned* keys;
  const uint8_t* vals;
  size_t n;
  unsigned *pf, *pt;
  __device__ void get(size_t i, unsigned& a, unsigned& b) const {
    a = vals[i];
    // equal keys are equal scores (-0.0 was mapped to +0.0); a NaN, unequal to itself, is a point of its own
    const unsigned k = keys[i];
    b = (i + 1 == n || k != keys[i + 1] || key_value(k) != key_value(k)) ? 1u : 0u;
  }
  __device__ void emit(size_t i, unsigned a_incl, unsigned b_incl) const {
    pf[b_incl - 1] = (unsigned)(i + 1) - a_incl;
    pt[b_incl - 1] = a_incl;
  }
};

struct CurveOp {    // ROC points -> roc_curve(drop_intermediate=True) after the origin: b = point kept
  const unsigned *pf, *pt;
  size_t n;
  unsigned *cf, *ct;
  __device__ void get(size_t i, unsigned& a, unsigned& b) const {
    a = 0;
    b = 1;
    if (n > 2 && i > 0 && i + 1 < n) {   // len(fps) > 2: keep where a second difference of fps or tps is non-zero
      const unsigned f0 = pf[i - 1], f1 = pf[i], f2 = pf[i + 1], t0 = pt[i - 1], t1 = pt[i], t2 = pt[i + 1];
      b = (f2 - f1 != f1 - f0 || t2 - t1 != t1 - t0) ? 1u : 0u;
    }
  }
  __device__ void emit(size_t i, unsigned, unsigned b_incl) const {
    cf[b_incl] = pf[i];   // [0] is the origin
    ct[b_incl] = pt[i];
  }
};

template <class Op>
__global__ __launch_bounds__(RT) void part_kernel(Op op, size_t span, unsigned* __restrict__ pa, unsigned* __restrict__ pb) {
  const size_t lo = (size_t)blockIdx.x * span, hi = std::min(op.n, lo + span);
  unsigned sa = 0, sb = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += RT) {
    unsigned a, b;
    op.get(i, a, b);
    sa += a;
    sb += b;
  }
  __shared__ unsigned red[2 * WAVES];
  sa = (unsigned)wave_sum((long long)sa);
  sb = (unsigned)wave_sum((long long)sb);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = sa;
    red[WAVES + (threadIdx.x >> 6)] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned a = 0, b = 0;
    for (int i = 0; i < WAVES; ++i) {
      a += red[i];
      b += red[WAVES + i];
    }
    pa[blockIdx.x] = a;
    pb[blockIdx.x] = b;
  }
}

template <class Op>
__global__ __launch_bounds__(RT) void emit_kernel(Op op, size_t span, const unsigned* __restrict__ pa,
                                                  const unsigned* __restrict__ pb) {
  __shared__ unsigned red[WAVES];
  const size_t lo = (size_t)blockIdx.x * span, hi = std::min(op.n, lo + span);
  unsigned ca = pa[blockIdx.x], cb = pb[blockIdx.x];
  for (size_t base = lo; base < hi; base += (size_t)RT * SPAN_ITEMS) {
    const size_t i0 = base + (size_t)threadIdx.x * SPAN_ITEMS;   // SPAN_ITEMS consecutive elements per thread
    unsigned a[SPAN_ITEMS], b[SPAN_ITEMS], x = 0;
#pragma unroll
    for (int j = 0; j < SPAN_ITEMS; ++j) {
      a[j] = b[j] = 0;
      if (i0 + j < hi) op.get(i0 + j, a[j], b[j]);
      x += (a[j] << 16) | b[j];   // both sums of a step are <= RT * SPAN_ITEMS < 2^16
    }
    unsigned tot;
    unsigned pre = block_excl_scan(x, red, &tot);
    unsigned ia = ca + (pre >> 16), ib = cb + (pre & 0xffffu);
#pragma unroll
    for (int j = 0; j < SPAN_ITEMS; ++j) {
      ia += a[j];
      ib += b[j];
      if (b[j]) op.emit(i0 + j, ia, ib);
    }
    ca += tot >> 16;
    cb += tot & 0xffffu;
  }
}

// ---- 4. AUC and EER over the points ---------------------------------------------------------------------------
// out[0] = eer, *eer_point = the point at the upper end of its segment, area_parts[workgroup] = its share of the AUC
__global__ __launch_bounds__(RT) void roc_points_kernel(const unsigned* __restrict__ pf, const unsigned* __restrict__ pt,
                                                        size_t m, double P, double N, double* __restrict__ out,
                                                        double* __restrict__ area_parts, unsigned* __restrict__ eer_point) {
  __shared__ double red[WAVES];
  double area = 0.0;
  for (size_t j = (size_t)blockIdx.x * RT + threadIdx.x; j < m; j += (size_t)gridDim.x * RT) {
    const double t1 = (double)pt[j], f1 = (double)pf[j];
    double t0 = 0.0, f0 = 0.0;  // roc_curve prepends the point (0, 0)
    if (j > 0) {
      t0 = (double)pt[j - 1];
      f0 = (double)pf[j - 1];
    }
    const double x0 = f0 / N, x1 = f1 / N, y0 = t0 / P, y1 = t1 / P;
    area += (x1 - x0) * (y0 + y1) * 0.5;
    const double g0 = 1.0 - x0 - y0, g1 = 1.0 - x1 - y1;
    if (g0 > 0.0 && g1 <= 0.0) {  // exactly one segment qualifies
      out[0] = x0 + (x1 - x0) * g0 / (g0 - g1);
      *eer_point = (unsigned)j;
    }
  }
  area = wave_sum(area);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = area;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < WAVES; ++i) s += red[i];
    area_parts[blockIdx.x] = s;
  }
}

// ---- 6. detection cost over the points --------------------------------------------------------------------------
// Operating point o: a[o] = c_miss p_target, b[o] = c_fa (1 - p_target); the cost of a point is a (1 - tps / P) + b fps / N.
struct DcfOps {
  int n;
  double a[DCF_MAX_OPS], b[DCF_MAX_OPS];
};

// (c, i) beats (bc, bi): the smaller cost, then the smaller index (the earlier point, the higher threshold)
__device__ __forceinline__ void dcf_take(double& bc, unsigned& bi, double c, unsigned i) {
  if (c < bc || (c == bc && i < bi)) {
    bc = c;
    bi = i;
  }
}
__device__ __forceinline__ void dcf_wave_min(double& bc, unsigned& bi) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double oc = __shfl_xor(bc, m, 64);
    const unsigned oi = __shfl_xor(bi, m, 64);
    dcf_take(bc, bi, oc, oi);
  }
}

// Index 0 is roc_curve's origin (reject everything: tps = fps = 0), index j + 1 the distinct-score point j.
// pcost / pidx [DCF_MAX_OPS][PMAX]: this workgroup's minimum per operating point.
__global__ __launch_bounds__(RT) void dcf_part_kernel(const unsigned* __restrict__ pf, const unsigned* __restrict__ pt, size_t m,
                                                      double P, double N, const DcfOps ops, double* __restrict__ pcost,
                                                      unsigned* __restrict__ pidx) {
  double bc[DCF_MAX_OPS];
  unsigned bi[DCF_MAX_OPS];
#pragma unroll
  for (int o = 0; o < DCF_MAX_OPS; ++o) {
    bc[o] = INFINITY;
    bi[o] = 0xffffffffu;
  }
  for (size_t j = (size_t)blockIdx.x * RT + threadIdx.x; j <= m; j += (size_t)gridDim.x * RT) {
    double t = 0.0, f = 0.0;
    if (j > 0) {
      t = (double)pt[j - 1];
      f = (double)pf[j - 1];
    }
    const double miss = 1.0 - t / P, fa = f / N;
#pragma unroll
    for (int o = 0; o < DCF_MAX_OPS; ++o) {
      if (o < ops.n) {
#pragma clang fp contract(off)   // two products and a sum, each rounded: the host path's arithmetic
        const double cost = ops.a[o] * miss + ops.b[o] * fa;
        if (cost < bc[o]) {   // a thread's indices only grow: the first of equal costs stays
          bc[o] = cost;
          bi[o] = (unsigned)j;
        }
      }
    }
  }
  __shared__ double rc[DCF_MAX_OPS][WAVES];
  __shared__ unsigned ri[DCF_MAX_OPS][WAVES];
#pragma unroll
  for (int o = 0; o < DCF_MAX_OPS; ++o) {
    if (o < ops.n) {
      dcf_wave_min(bc[o], bi[o]);
      if ((threadIdx.x & 63) == 0) {
        rc[o][threadIdx.x >> 6] = bc[o];
        ri[o][threadIdx.x >> 6] = bi[o];
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < ops.n) {
    const int o = threadIdx.x;
    double c = rc[o][0];
    unsigned i = ri[o][0];
    for (int w = 1; w < WAVES; ++w) dcf_take(c, i, rc[o][w], ri[o][w]);
    pcost[(size_t)o * PMAX + blockIdx.x] = c;
    pidx[(size_t)o * PMAX + blockIdx.x] = i;
  }
}

// One workgroup: out[1] = the AUC, the pgrid shares added in a fixed order; fin[0] = the score of the EER point; per operating
// point o, fin[1 + 4 o ..] = {the smallest cost, its index (0 = the origin), fps, tps} and thr[o] = that point's score.  A
// point's score is the sorted key of the last pair at or above it, element fps + tps - 1.
__global__ __launch_bounds__(RT) void roc_finish_kernel(const double* __restrict__ area_parts, unsigned pgrid,
                                                        const unsigned* __restrict__ eer_point, const unsigned* __restrict__ pf,
                                                        const unsigned* __restrict__ pt, const unsigned* __restrict__ keys,
                                                        int n_op, const double* __restrict__ pcost,
                                                        const unsigned* __restrict__ pidx, unsigned dgrid,
                                                        double* __restrict__ out, double* __restrict__ fin,
                                                        float* __restrict__ thr) {
  __shared__ double red[WAVES];
  __shared__ unsigned redi[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double area = 0.0;
  for (unsigned i = threadIdx.x; i < pgrid; i += RT) area += area_parts[i];
  area = wave_sum(area);
  if (lane == 0) red[w] = area;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < WAVES; ++i) s += red[i];
    out[1] = s;
    const unsigned j = *eer_point;
    fin[0] = (double)key_value(keys[(size_t)pf[j] + pt[j] - 1]);
  }
  for (int o = 0; o < n_op; ++o) {
    double bc = INFINITY;
    unsigned bi = 0xffffffffu;
    for (unsigned i = threadIdx.x; i < dgrid; i += RT) dcf_take(bc, bi, pcost[(size_t)o * PMAX + i], pidx[(size_t)o * PMAX + i]);
    dcf_wave_min(bc, bi);
    __syncthreads();
    if (lane == 0) {
      red[w] = bc;
      redi[w] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 1; i < WAVES; ++i) dcf_take(bc, bi, red[i], redi[i]);
      double f = 0.0, t = 0.0;
      float score = INFINITY;   // the origin accepts nothing
      if (bi > 0) {
        const unsigned fi = pf[bi - 1], ti = pt[bi - 1];
        f = (double)fi;
        t = (double)ti;
        score = key_value(keys[(size_t)fi + ti - 1]);
      }
      fin[1 + 4 * o] = bc;
      fin[2 + 4 * o] = (double)bi;
      fin[3 + 4 * o] = f;
      fin[4 + 4 * o] = t;
      thr[o] = score;
    }
  }
}

// ---- decision counts ----------------------------------------------------------------------------------------------
struct DcThr {
  float v[DC_MAX_THR];
};

// One streaming pass, four consecutive pairs per thread and step (VEC: one 16-byte and one 4-byte load).  counts[2 t] =
// targets with score >= v[t], counts[2 t + 1] = non-targets with score >= v[t], counts[2 MAXT] = targets; a NaN score (and a
// NaN threshold: the unused slots up to MAXT) accepts nothing.  Per-thread counts are 32-bit: n < 2^32 x the threads launched.
template <int MAXT, bool VEC>
__global__ __launch_bounds__(RT) void decision_counts_kernel(const float* __restrict__ sc, const uint8_t* __restrict__ lab, size_t n,
                                                             const DcThr thr, unsigned long long* __restrict__ counts) {
  unsigned acc[MAXT], tgt[MAXT], pos = 0;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) acc[t] = tgt[t] = 0;
  const size_t quads = (n + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * RT + threadIdx.x; q < quads; q += (size_t)gridDim.x * RT) {
    const size_t i0 = 4 * q;
    float s[4];
    unsigned l[4];
    if (VEC && i0 + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(sc + i0);
      const uchar4 u = *reinterpret_cast<const uchar4*>(lab + i0);
      s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
      l[0] = u.x != 0, l[1] = u.y != 0, l[2] = u.z != 0, l[3] = u.w != 0;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = i0 + e < n;
        s[e] = ok ? sc[i0 + e] : __builtin_nanf("");
        l[e] = ok ? lab[i0 + e] != 0 : 0u;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pos += l[e];
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        const unsigned hit = s[e] >= thr.v[t];
        acc[t] += hit;
        tgt[t] += hit & l[e];
      }
    }
  }
  constexpr int NC = 2 * MAXT + 1;
  __shared__ long long red[WAVES][NC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const long long a = wave_sum((long long)tgt[t]), b = wave_sum((long long)(acc[t] - tgt[t]));
    if (lane == 0) {
      red[w][2 * t] = a;
      red[w][2 * t + 1] = b;
    }
  }
  const long long p = wave_sum((long long)pos);
  if (lane == 0) red[w][2 * MAXT] = p;
  __syncthreads();
  if ((int)threadIdx.x < NC) {
    long long h = 0;
    for (int i = 0; i < WAVES; ++i) h += red[i][threadIdx.x];
    if (h) atomicAdd(&counts[threadIdx.x], (unsigned long long)h);
  }
}

// ---- top-1 ----------------------------------------------------------------------------------------------------
// (v, i) beats (bv, bi) as np.argmax orders them: a NaN first, then the larger value, then the smaller index.
__device__ __forceinline__ void top1_take(float& bv, unsigned& bi, float v, unsigned i) {
  const bool vn = v != v, bn = bv != bv;
  const bool take = (vn || bn) ? (vn && (!bn || i < bi)) : (v > bv || (v == bv && i < bi));
  if (take) {
    bv = v;
    bi = i;
  }
}

// One wave per row: the row's maximum, the hit against the enrolled column, the one-hot row.
__global__ __launch_bounds__(RT) void top1_kernel(const float* __restrict__ s, int64_t rows, int cols, const int32_t* __restrict__ tru,
                                                  int32_t* __restrict__ amax, uint8_t* __restrict__ lab,
                                                  unsigned long long* __restrict__ correct) {
  const int lane = threadIdx.x & 63;
  long long hits = 0;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    const float* row = s + (size_t)r * cols;
    float bv = -INFINITY;
    unsigned bi = 0xffffffffu;
#pragma unroll 4
    for (int c = lane; c < cols; c += 64) top1_take(bv, bi, row[c], (unsigned)c);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(bv, m, 64);
      const unsigned oi = __shfl_xor(bi, m, 64);
      top1_take(bv, bi, ov, oi);
    }
    const int32_t want = tru[r];
    if (lane == 0) {
      amax[r] = (int32_t)bi;
      hits += want >= 0 && (int32_t)bi == want;
    }
    if (lab) {
      uint8_t* lr = lab + (size_t)r * cols;
      for (int c = lane; c < cols; c += 64) lr[c] = c == want ? 1 : 0;
    }
  }
  __shared__ long long red[WAVES];
  hits = wave_sum(hits);
  if (lane == 0) red[threadIdx.x >> 6] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long h = 0;
    for (int i = 0; i < WAVES; ++i) h += red[i];
    if (h) atomicAdd(correct, (unsigned long long)h);
  }
}

// ---- 7. svk_rocch only: the convex hull of the points; svk_pav_apply's kernel ------------------------------------------
#include "rocch.h"

// ---- host side ------------------------------------------------------------------------------------------------
struct RocLayout {
  size_t keys[2], vals[2], pf, pt, counts, parts, hist, misc, total;
  size_t hull[2], hcount, total_hull;   // svk_rocch only, behind `total`: what every other entry asks for is unchanged
};

// Workspace of one split of m pairs (splits run one after another through it).
RocLayout roc_layout(size_t m) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  RocLayout l;
  size_t o = 0;
  for (int b = 0; b < 2; ++b) {
    l.keys[b] = o;
    o += up(m * 4);
  }
  for (int b = 0; b < 2; ++b) {
    l.vals[b] = o;
    o += up(m);
  }
  l.pf = o;     o += up(m * 4);
  l.pt = o;     o += up(m * 4);
  l.counts = o; o += up((size_t)256 * GMAX * 4);   // after the sort: the point passes' per-workgroup results (POST_* below)
  l.parts = o;  o += up((size_t)4 * GMAX * 4);   // four [GMAX] partial-sum rows: (a, b) of the points, of the curve
  l.hist = o;   o += up(1026 * 4);
  l.misc = o;   o += 256;                       // [0..1] doubles eer, auc; then u32 totals at +64
  l.total = o;
  // two hull buffers of one (f, t) pair per point (the origin + at most m distinct scores), each hull anchored at its first
  // tile's offset; then every hull's vertex count, level after level: the tile pass's, then each merge level's (half as many
  // each time, rounded up: below 2 tiles + 64 in all).  svk_rocch_level_counts_offset gives their offset (svk.h, "the ROC convex hull", Diagnostics).
  const size_t tiles = (m + 1 + TILE - 1) / TILE;
  for (int b = 0; b < 2; ++b) {
    l.hull[b] = o;
    o += up((m + 1) * 8);
  }
  l.hcount = o;
  o += up((2 * tiles + 64) * 4);
  l.total_hull = o;
  return l;
}

// The count matrix's bytes once the sort is done, by byte offset: what the passes over the ROC points leave per workgroup.
constexpr size_t POST_AREA = 0;                                               // double [PMAX]
constexpr size_t POST_COST = POST_AREA + PMAX * 8;                            // double [DCF_MAX_OPS][PMAX]
constexpr size_t POST_IDX = POST_COST + (size_t)DCF_MAX_OPS * PMAX * 8;       // u32 [DCF_MAX_OPS][PMAX]
constexpr size_t POST_FIN = POST_IDX + (size_t)DCF_MAX_OPS * PMAX * 4;        // double [1 + 4 DCF_MAX_OPS]
constexpr size_t POST_THR = POST_FIN + (1 + 4 * DCF_MAX_OPS) * 8;             // float [DCF_MAX_OPS]
static_assert(POST_THR + DCF_MAX_OPS * 4 <= (size_t)256 * GMAX * 4, "the point passes' results outgrow the count matrix");

// What svk_roc_dcf asks of a split beyond {eer, auc, positives, points}: fin / thr as roc_finish_kernel writes them.
struct DcfRequest {
  DcfOps ops;
  double fin[1 + 4 * DCF_MAX_OPS];
  float thr[DCF_MAX_OPS];
};

// What svk_rocch asks of a split beyond that: the hull of the origin + the points in the caller's planes, count = its vertices.
struct HullRequest {
  unsigned *vf, *vt;
  float* vscore;
  int64_t capacity;
  unsigned count;
};

// span (a multiple of `unit`) and grid so that at most GMAX workgroups cover n elements
void spans(size_t n, size_t unit, size_t* span, unsigned* grid) {
  const size_t units = std::max<size_t>(1, (n + unit - 1) / unit);
  *span = (units + GMAX - 1) / GMAX * unit;
  *grid = (unsigned)std::max<size_t>(1, (n + *span - 1) / *span);
}

template <class Op>
int span_pass(svk_ctx* ctx, const Op& op, unsigned* pa, unsigned* pb, unsigned* tot_a, unsigned* tot_b, bool emit) {
  size_t span;
  unsigned grid;
  spans(op.n, (size_t)RT * SPAN_ITEMS, &span, &grid);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(part_kernel<Op>, dim3(grid), dim3(RT), 0, st, op, span, pa, pb);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, st, pa, grid, tot_a);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, st, pb, grid, tot_b);
  SVK_LAUNCH_CHECK(ctx);
  if (emit) {
    hipLaunchKernelGGL(emit_kernel<Op>, dim3(grid), dim3(RT), 0, st, op, span, pa, pb);
    SVK_LAUNCH_CHECK(ctx);
  }
  return SVK_OK;
}

// One split of m pairs.  strict (svk_roc_k): non-finite scores and a single class are errors found before the
// sort, named by `split`.  cf / ct: the split's curve planes, or NULL.  h4 = {eer, auc, positives, points}: points =
// distinct scores (curve == false) or the length of roc_curve's output (curve == true).  dcf: NULL, or the operating points
// whose detection-cost minima this split's points are searched for; it also takes the EER point's score.  hull: NULL (nothing
// more is launched), or the planes the hull of the points goes to; the workspace then holds l.total_hull bytes.
int roc_split(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, size_t m, char* w, const RocLayout& l,
              bool strict, int split, bool curve, unsigned* cf, unsigned* ct, double* h4, DcfRequest* dcf = nullptr,
              HullRequest* hull = nullptr) {
  hipStream_t st = ctx->stream;
  unsigned* keys[2] = {reinterpret_cast<unsigned*>(w + l.keys[0]), reinterpret_cast<unsigned*>(w + l.keys[1])};
  uint8_t* vals[2] = {reinterpret_cast<uint8_t*>(w + l.vals[0]), reinterpret_cast<uint8_t*>(w + l.vals[1])};
  unsigned* pf = reinterpret_cast<unsigned*>(w + l.pf);
  unsigned* pt = reinterpret_cast<unsigned*>(w + l.pt);
  unsigned* counts = reinterpret_cast<unsigned*>(w + l.counts);
  unsigned* parts = reinterpret_cast<unsigned*>(w + l.parts);
  unsigned* hist = reinterpret_cast<unsigned*>(w + l.hist);
  double* out = reinterpret_cast<double*>(w + l.misc);
  unsigned* totals = reinterpret_cast<unsigned*>(w + l.misc + 64);   // [0] pos, [1] points, [2] -, [3] curve points, [4] EER point
  char* post = w + l.counts;
  double* area_parts = reinterpret_cast<double*>(post + POST_AREA);
  double* pcost = reinterpret_cast<double*>(post + POST_COST);
  unsigned* pidx = reinterpret_cast<unsigned*>(post + POST_IDX);
  double* fin = reinterpret_cast<double*>(post + POST_FIN);
  float* thr = reinterpret_cast<float*>(post + POST_THR);
  const unsigned* bits = reinterpret_cast<const unsigned*>(d_scores);

  SVK_HIP(ctx, hipMemsetAsync(hist, 0, 1026 * 4, st));
  SVK_HIP(ctx, hipMemsetAsync(out, 0, 64, st));
  const unsigned hgrid = (unsigned)std::max<size_t>(1, std::min<size_t>((m + RT - 1) / RT, (size_t)ctx->num_cu * 4));
  hipLaunchKernelGGL(hist_kernel, dim3(hgrid), dim3(RT), 0, st, bits, d_labels, m, hist);
  SVK_LAUNCH_CHECK(ctx);
  unsigned h[1026];
  SVK_HIP(ctx, hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, st));
  SVK_HIP(ctx, hipStreamSynchronize(st));
  const unsigned P = h[1025];
  if (strict && h[1024])
    return svk_fail(ctx, SVK_ERR_BAD_ARG, "split %d: %u non-finite scores (NaN or inf): roc_curve rejects them", split, h[1024]);
  if (P == 0 || (size_t)P == m) {
    if (strict)
      return svk_fail(ctx, SVK_ERR_BAD_ARG, "split %d has only one class: %u positives of %zu pairs", split, P, m);
    return svk_fail(ctx, SVK_ERR_BAD_ARG, "ROC needs both classes: %u positives of %lld", P, (long long)m);
  }

  // the sort: passes whose digit is the same for every key are skipped; at least one pass runs (it maps the keys)
  size_t span;
  unsigned grid;
  spans(m, TILE, &span, &grid);
  const unsigned* src = bits;
  const uint8_t* vsrc = d_labels;
  int raw = 1, cur = 0;
  for (int p = 0; p < 4; ++p) {
    bool constant = false;
    for (int d = 0; d < 256; ++d) constant |= (size_t)h[p * 256 + d] == m;
    if (constant && !(p == 3 && raw)) continue;
    hipLaunchKernelGGL(count_kernel, dim3(grid), dim3(RT), 0, st, src, raw, m, span, 8 * p, counts);
    SVK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(offsets_kernel, dim3(256), dim3(GMAX), 0, st, counts, grid, hist + 256 * p);
    SVK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(scatter_kernel, dim3(grid), dim3(RT), 0, st, src, vsrc, raw, m, span, 8 * p, counts, keys[cur],
                       vals[cur]);
    SVK_LAUNCH_CHECK(ctx);
    src = keys[cur];
    vsrc = vals[cur];
    raw = 0;
    cur ^= 1;
  }

  // the distinct-score points, then AUC / EER
  const PointsOp pop{src, vsrc, m, pf, pt};
  if (int rc = span_pass(ctx, pop, parts, parts + GMAX, totals, totals + 1, true)) return rc;
  unsigned M = 0;
  SVK_HIP(ctx, hipMemcpyAsync(&M, totals + 1, 4, hipMemcpyDeviceToHost, st));
  SVK_HIP(ctx, hipStreamSynchronize(st));
  const size_t pcap = std::min<size_t>((size_t)ctx->num_cu * 8, PMAX);
  const unsigned pgrid = (unsigned)std::max<size_t>(1, std::min<size_t>((M + RT - 1) / RT, pcap));
  const double Pd = (double)P, Nd = (double)m - (double)P;
  hipLaunchKernelGGL(roc_points_kernel, dim3(pgrid), dim3(RT), 0, st, pf, pt, (size_t)M, Pd, Nd, out, area_parts, totals + 4);
  SVK_LAUNCH_CHECK(ctx);
  const int n_op = dcf ? dcf->ops.n : 0;
  const unsigned dgrid = (unsigned)std::min<size_t>(((size_t)M + 1 + RT - 1) / RT, pcap);
  if (n_op) {
    hipLaunchKernelGGL(dcf_part_kernel, dim3(dgrid), dim3(RT), 0, st, pf, pt, (size_t)M, Pd, Nd, dcf->ops, pcost, pidx);
    SVK_LAUNCH_CHECK(ctx);
  }
  hipLaunchKernelGGL(roc_finish_kernel, dim3(1), dim3(RT), 0, st, area_parts, pgrid, totals + 4, pf, pt, src, n_op, pcost, pidx,
                     dgrid, out, fin, thr);
  SVK_LAUNCH_CHECK(ctx);
  // the hull, behind the last reader of pf / pt: one hull per tile, then pairwise merges; the level count depends on M alone
  const uint2* hfinal = nullptr;
  if (hull) {
    uint2* hb[2] = {reinterpret_cast<uint2*>(w + l.hull[0]), reinterpret_cast<uint2*>(w + l.hull[1])};
    unsigned* hc = reinterpret_cast<unsigned*>(w + l.hcount);   // this level's counts; the next level's follow them
    const size_t points = (size_t)M + 1;
    unsigned hulls = (unsigned)((points + TILE - 1) / TILE);
    hipLaunchKernelGGL(hull_tile_kernel, dim3(hulls), dim3(RT), 0, st, pf, pt, points, hb[0], hc);
    SVK_LAUNCH_CHECK(ctx);
    int at = 0;
    for (size_t hspan = TILE; hulls > 1; hspan *= 2, hc += hulls, hulls = (hulls + 1) / 2, at ^= 1) {
      hipLaunchKernelGGL(hull_merge_kernel, dim3((hulls + 1) / 2), dim3(RT), 0, st, hb[at], hc, hulls, hspan, hb[at ^ 1],
                         hc + hulls);
      SVK_LAUNCH_CHECK(ctx);
    }
    hfinal = hb[at];
    SVK_HIP(ctx, hipMemcpyAsync(&hull->count, hc, 4, hipMemcpyDeviceToHost, st));
  }
  unsigned C = M;
  if (curve) {
    const CurveOp cop{pf, pt, M, cf, ct};
    if (int rc = span_pass(ctx, cop, parts + 2 * GMAX, parts + 3 * GMAX, totals + 2, totals + 3, cf != nullptr)) return rc;
    if (cf) {
      SVK_HIP(ctx, hipMemsetAsync(cf, 0, 4, st));   // the prepended origin
      SVK_HIP(ctx, hipMemsetAsync(ct, 0, 4, st));
    }
    SVK_HIP(ctx, hipMemcpyAsync(&C, totals + 3, 4, hipMemcpyDeviceToHost, st));
  }
  SVK_HIP(ctx, hipMemcpyAsync(h4, out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (dcf) {
    SVK_HIP(ctx, hipMemcpyAsync(dcf->fin, fin, sizeof(double) * (1 + 4 * (size_t)n_op), hipMemcpyDeviceToHost, st));
    if (n_op) SVK_HIP(ctx, hipMemcpyAsync(dcf->thr, thr, sizeof(float) * (size_t)n_op, hipMemcpyDeviceToHost, st));
  }
  SVK_HIP(ctx, hipStreamSynchronize(st));
  h4[2] = (double)P;
  h4[3] = curve ? (double)C + 1.0 : (double)M;
  if (hull) {
    if ((int64_t)hull->count > hull->capacity)
      return svk_fail(ctx, SVK_ERR_BAD_ARG, "bad argument: capacity %lld is below the hull's %u vertices", (long long)hull->capacity,
                      hull->count);
    hipLaunchKernelGGL(hull_emit_kernel, dim3((hull->count + RT - 1) / RT), dim3(RT), 0, st, hfinal, hull->count, src, hull->vf,
                       hull->vt, hull->vscore);
    SVK_LAUNCH_CHECK(ctx);
  }
  return SVK_OK;
}

}  // namespace

extern "C" {

size_t svk_roc_workspace_bytes(int64_t n) { return n > 0 ? roc_layout((size_t)n).total : 0; }

int svk_roc_eer(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, void* d_workspace,
                size_t workspace_bytes, double* h_out) {
  if (!ctx || !h_out) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 2, "need at least two (label, score) pairs");
  SVK_REQUIRE(ctx, n < ((int64_t)1 << 32), "at most 2^32 - 1 pairs");
  SVK_REQUIRE(ctx, d_scores && d_labels && d_workspace, "NULL buffer");
  const RocLayout l = roc_layout((size_t)n);
  SVK_REQUIRE(ctx, workspace_bytes >= l.total, "workspace smaller than svk_roc_workspace_bytes(n)");
  return roc_split(ctx, d_scores, d_labels, (size_t)n, reinterpret_cast<char*>(d_workspace), l, false, 0, false, nullptr,
                   nullptr, h_out);
}

size_t svk_roc_k_workspace_bytes(int64_t n, int32_t k) {
  if (n < 2 || k < 1 || n / k < 2) return 0;
  return roc_layout((size_t)(n / k)).total;
}

int svk_roc_k(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, int32_t k, void* d_workspace,
              size_t workspace_bytes, uint32_t* d_curve, double* h_out) {
  if (!ctx || !h_out) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, k >= 1, "k < 1");
  SVK_REQUIRE(ctx, n >= 0 && n < ((int64_t)1 << 32), "n outside [0, 2^32)");
  const int64_t step = n / k;   // = int(n / float(k)) of evaluation.py:13 for n < 2^32
  if (step < 2)
    return svk_fail(ctx, SVK_ERR_BAD_ARG, "bad argument: %lld pairs in %d splits leave %lld per split (need >= 2)", (long long)n,
                    k, (long long)step);
  SVK_REQUIRE(ctx, d_scores && d_labels && d_workspace, "NULL buffer");
  const RocLayout l = roc_layout((size_t)step);
  SVK_REQUIRE(ctx, workspace_bytes >= l.total, "workspace smaller than svk_roc_k_workspace_bytes(n, k)");
  const size_t plane = (size_t)k * (size_t)(step + 1);
  for (int s = 0; s < k; ++s) {
    const size_t lo = (size_t)s * (size_t)step;
    uint32_t* cf = d_curve ? d_curve + (size_t)s * (size_t)(step + 1) : nullptr;
    uint32_t* ct = d_curve ? cf + plane : nullptr;
    if (int rc = roc_split(ctx, d_scores + lo, d_labels + lo, (size_t)step, reinterpret_cast<char*>(d_workspace), l, true, s,
                           true, cf, ct, h_out + 4 * (size_t)s))
      return rc;
  }
  return SVK_OK;
}

int svk_top1(svk_ctx* ctx, const float* d_scores, int64_t n_rows, int32_t n_cols, const int32_t* d_true, int32_t* d_argmax,
             uint8_t* d_labels, int64_t* h_correct) {
  if (!ctx || !h_correct) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rows >= 1 && n_cols >= 1, "empty score matrix");
  SVK_REQUIRE(ctx, d_scores && d_true && d_argmax, "NULL buffer");
  hipStream_t st = ctx->stream;
  auto* hits = reinterpret_cast<unsigned long long*>(static_cast<char*>(ctx->scratch) + SVK_SLOT_TOP1);
  SVK_HIP(ctx, hipMemsetAsync(hits, 0, 8, st));
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_rows + WAVES - 1) / WAVES, (int64_t)ctx->num_cu * 8));
  hipLaunchKernelGGL(top1_kernel, dim3(grid), dim3(RT), 0, st, d_scores, n_rows, (int)n_cols, d_true, d_argmax, d_labels, hits);
  SVK_LAUNCH_CHECK(ctx);
  unsigned long long h = 0;
  SVK_HIP(ctx, hipMemcpyAsync(&h, hits, 8, hipMemcpyDeviceToHost, st));
  SVK_HIP(ctx, hipStreamSynchronize(st));
  *h_correct = (int64_t)h;
  return SVK_OK;
}

size_t svk_roc_dcf_workspace_bytes(int64_t n) { return n >= 2 ? roc_layout((size_t)n).total : 0; }

}  // extern "C"

namespace {

// svk_roc_dcf, and svk_rocch with a hull request: the same checks in the same words, the same launches in front of the hull's
int roc_dcf_entry(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const double* h_ops, int32_t n_op,
                  void* d_workspace, size_t workspace_bytes, double* h_out, HullRequest* hull) {
  if (!ctx || !h_out) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 2, "need at least two (label, score) pairs");
  SVK_REQUIRE(ctx, n < ((int64_t)1 << 32), "at most 2^32 - 1 pairs");
  SVK_REQUIRE(ctx, n_op >= 0 && n_op <= DCF_MAX_OPS, "0 to 8 operating points");
  SVK_REQUIRE(ctx, d_scores && d_labels && d_workspace && (h_ops || n_op == 0), "NULL buffer");
  DcfRequest req;
  req.ops.n = n_op;
  for (int o = 0; o < DCF_MAX_OPS; ++o) req.ops.a[o] = req.ops.b[o] = 0.0;
  for (int o = 0; o < n_op; ++o) {
    const double p = h_ops[3 * o], c_miss = h_ops[3 * o + 1], c_fa = h_ops[3 * o + 2];
    if (!(p > 0.0 && p < 1.0 && c_miss > 0.0 && c_miss < INFINITY && c_fa > 0.0 && c_fa < INFINITY))
      return svk_fail(ctx, SVK_ERR_BAD_ARG, "bad argument: operating point %d = (%g, %g, %g): need 0 < p_target < 1 and finite "
                      "c_miss, c_fa > 0", o, p, c_miss, c_fa);
    req.ops.a[o] = c_miss * p;
    req.ops.b[o] = c_fa * (1.0 - p);
  }
  const RocLayout l = roc_layout((size_t)n);
  if (hull) {
    SVK_REQUIRE(ctx, hull->vf && hull->vt && hull->vscore, "NULL buffer");
    SVK_REQUIRE(ctx, hull->capacity >= 1, "capacity < 1");
    SVK_REQUIRE(ctx, workspace_bytes >= l.total_hull, "workspace smaller than svk_rocch_workspace_bytes(n)");
  } else {
    SVK_REQUIRE(ctx, workspace_bytes >= l.total, "workspace smaller than svk_roc_dcf_workspace_bytes(n)");
  }
  double h4[4];
  if (int rc = roc_split(ctx, d_scores, d_labels, (size_t)n, reinterpret_cast<char*>(d_workspace), l, true, 0, false, nullptr,
                         nullptr, h4, &req, hull))
    return rc;
  const double P = h4[2], N = (double)n - P;
  for (int i = 0; i < 4; ++i) h_out[i] = h4[i];
  h_out[4] = req.fin[0];
  for (int o = 0; o < n_op; ++o) {
    const double* f = req.fin + 1 + 4 * o;
    double* r = h_out + 5 + 4 * o;
    r[0] = f[0] / std::min(req.ops.a[o], req.ops.b[o]);
    r[1] = (double)req.thr[o];
    r[2] = 1.0 - f[3] / P;
    r[3] = f[2] / N;
  }
  if (hull) h_out[5 + 4 * n_op] = (double)hull->count;
  return SVK_OK;
}

}  // namespace

extern "C" {

int svk_roc_dcf(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const double* h_ops, int32_t n_op,
                void* d_workspace, size_t workspace_bytes, double* h_out) {
  return roc_dcf_entry(ctx, d_scores, d_labels, n, h_ops, n_op, d_workspace, workspace_bytes, h_out, nullptr);
}

size_t svk_rocch_workspace_bytes(int64_t n) { return n >= 2 ? roc_layout((size_t)n).total_hull : 0; }

size_t svk_rocch_level_counts_offset(int64_t n) { return n >= 2 ? roc_layout((size_t)n).hcount : 0; }

int64_t svk_rocch_max_vertices(int64_t n) {
  if (n < 1) return 0;
  // S = the smallest integer with S (S + 1) (S + 2) / 3 >= m (include/svk.h, at svk_rocch_max_vertices).  m = n, held to the
  // 2^32 - 1 trials svk_rocch takes (a larger n gets that bound's S: the K <= n term no longer binds there): S <= 2 345 and
  // every product is below 2^34
  const int64_t m = std::min<int64_t>(n, ((int64_t)1 << 32) - 1);
  int64_t s = 1;
  while (s * (s + 1) * (s + 2) / 3 < m) ++s;
  return std::min(s * (s + 3) / 2, n) + 1;
}

int svk_rocch(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const double* h_ops, int32_t n_op,
              void* d_workspace, size_t workspace_bytes, uint32_t* d_vf, uint32_t* d_vt, float* d_vscore, int64_t capacity,
              double* h_out) {
  HullRequest hull{d_vf, d_vt, d_vscore, capacity, 0};
  return roc_dcf_entry(ctx, d_scores, d_labels, n, h_ops, n_op, d_workspace, workspace_bytes, h_out, &hull);
}

int svk_pav_apply(svk_ctx* ctx, const float* d_scores, int64_t n, const float* d_edges, const float* d_llr, int32_t n_bins,
                  float* d_out) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 0, "negative size");
  SVK_REQUIRE(ctx, n_bins >= 1, "n_bins < 1");
  SVK_REQUIRE(ctx, d_edges && d_llr, "NULL table");
  if (n == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_scores && d_out, "NULL buffer");
  const uintptr_t ps = reinterpret_cast<uintptr_t>(d_scores), po = reinterpret_cast<uintptr_t>(d_out);
  SVK_REQUIRE(ctx, ((ps | po | reinterpret_cast<uintptr_t>(d_edges) | reinterpret_cast<uintptr_t>(d_llr)) & 3) == 0,
              "scores, table and output must be 4-byte aligned");
  const bool vec = (ps & 15) == (po & 15);
  const size_t head = vec ? std::min<size_t>((size_t)n, ((16 - (ps & 15)) & 15) / 4) : 0;
  const size_t quads = ((size_t)n - head + 3) / 4;
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((quads + RT - 1) / RT, (size_t)ctx->num_cu * 8));
  const bool lds = n_bins <= PAV_LDS_BINS;
  auto kern = lds ? (vec ? pav_apply_kernel<true, true> : pav_apply_kernel<true, false>)
                  : (vec ? pav_apply_kernel<false, true> : pav_apply_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(RT), 0, ctx->stream, d_scores, (size_t)n, head, d_edges, d_llr, (int)n_bins, d_out);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

int svk_decision_counts(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const float* h_thresholds,
                        int32_t n_thr, int64_t* h_out) {
  if (!ctx || !h_out) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 0, "negative size");
  SVK_REQUIRE(ctx, n_thr >= 1 && n_thr <= DC_MAX_THR, "1 to 16 thresholds");
  SVK_REQUIRE(ctx, h_thresholds && ((d_scores && d_labels) || n == 0), "NULL buffer");
  SVK_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_scores) & 3) == 0, "scores must be 4-byte aligned");
  DcThr thr;
  for (int t = 0; t < DC_MAX_THR; ++t) thr.v[t] = t < n_thr ? h_thresholds[t] : __builtin_nanf("");
  for (int t = 0; t < n_thr; ++t) SVK_REQUIRE(ctx, thr.v[t] == thr.v[t], "NaN threshold");
  const int maxt = n_thr == 1 ? 1 : n_thr <= 4 ? 4 : DC_MAX_THR;
  unsigned long long h[2 * DC_MAX_THR + 1] = {};
  if (n > 0) {
    if (int rc = svk_ensure_work(ctx, sizeof(h))) return rc;
    auto* counts = static_cast<unsigned long long*>(ctx->work);
    hipStream_t st = ctx->stream;
    SVK_HIP(ctx, hipMemsetAsync(counts, 0, sizeof(h), st));
    const bool vec = (reinterpret_cast<uintptr_t>(d_scores) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_labels) & 3) == 0;
    const size_t quads = ((size_t)n + 3) / 4;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((quads + RT - 1) / RT, (size_t)ctx->num_cu * 8));
    auto kern = maxt == 1 ? (vec ? decision_counts_kernel<1, true> : decision_counts_kernel<1, false>)
              : maxt == 4 ? (vec ? decision_counts_kernel<4, true> : decision_counts_kernel<4, false>)
                          : (vec ? decision_counts_kernel<DC_MAX_THR, true> : decision_counts_kernel<DC_MAX_THR, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RT), 0, st, d_scores, d_labels, (size_t)n, thr, counts);
    SVK_LAUNCH_CHECK(ctx);
    SVK_HIP(ctx, hipMemcpyAsync(h, counts, sizeof(unsigned long long) * (2 * (size_t)maxt + 1), hipMemcpyDeviceToHost, st));
    SVK_HIP(ctx, hipStreamSynchronize(st));
  }
  for (int t = 0; t < 2 * n_thr; ++t) h_out[t] = (int64_t)h[t];
  h_out[2 * n_thr] = (int64_t)h[2 * maxt];
  h_out[2 * n_thr + 1] = n - (int64_t)h[2 * maxt];
  return SVK_OK;
}

}  // extern "C"
