// The ROC convex hull and the PAV map (include/svk.h, "the ROC convex hull"): device code of roc.hip, included there inside its namespace
// (it uses RT, TILE, WAVES and key_value).  The hull of the origin + the distinct-score points (pf, pt) by divide and conquer:
// hull_tile_kernel leaves one hull per tile of TILE points, hull_merge_kernel joins adjacent hulls pairwise, level by level.
// A hull stays anchored at the offset of its first point's tile in a buffer of one (f, t) pair per point, its length beside it:
// nothing is compacted between levels, so no level needs a scan, a readback or another workgroup's result.  All integers.
#pragma once

constexpr int HULL_LEAF = 8;                         // points of one thread's monotone chain
constexpr int HULL_LEAVES = TILE / HULL_LEAF;        // = RT: one leaf per thread
constexpr int HULL_LDS_LEVELS = 8;                   // log2(HULL_LEAVES)
constexpr int HULL_LDS_POINTS = TILE + TILE / HULL_LEAF;   // a tile in LDS, one pad pair behind every 8
constexpr int PAV_LDS_BINS = 4096;                   // the PAV table in LDS: 2 x 16 KiB
static_assert(HULL_LEAVES == RT && (1 << HULL_LDS_LEVELS) == HULL_LEAVES, "one leaf per thread, a power of two of them");

// (b - a) x (c - a) for a <= b <= c in the sequence's order: both products are below N P < 2^62
__device__ __forceinline__ long long hull_cross(uint2 a, uint2 b, uint2 c) {
  return (long long)(b.x - a.x) * (long long)(c.y - a.y) - (long long)(b.y - a.y) * (long long)(c.x - a.x);
}

// Where a hull lives.  LDS: 8-byte reads bank on (address / 4) % 64 per 32 lanes; a leaf is 8 pairs = 16 words, so lanes 4
// apart would share a bank while every thread walks its own leaf.  One pad pair per leaf makes the stride 18 words: the 32
// lanes of a half then start on 32 distinct even banks.  That is the READS of the chain.  LDS writes bank on (address / 4) % 32:
// at 18 words the chain's in-place writes are 2-way conflicted, and the merge levels' reads and
// writes follow the hulls' lengths, not a fixed stride.  No bank-conflict counter was collected; what the 2-way costs is not known.
__device__ __forceinline__ int hull_phys(int i) { return i + (i >> 3); }
struct LdsHull {
  const uint2* p;
  int base;
  __device__ uint2 operator()(int i) const { return p[hull_phys(base + i)]; }
};
struct GlobalHull {
  const uint2* p;
  __device__ uint2 operator()(int i) const { return p[i]; }
};

// Is A[u] the left end of the bridge between the adjacent hulls A (na > 0 vertices) and B (nb > 0, to its right)?  *v = the
// right end seen from A[u]: the first i with cross(A[u], B[i], B[i + 1]) < 0 -- the predicate is monotone along a hull -- or
// B's last index.  Exactly one u of [0, na) qualifies.
template <class HA, class HB>
__device__ __forceinline__ bool hull_bridge_at(const HA& A, int na, const HB& B, int nb, int u, int* v) {
  const uint2 a = A(u);
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (hull_cross(a, B(mid), B(mid + 1)) < 0) hi = mid;
    else lo = mid + 1;
  }
  *v = lo;
  const uint2 b = B(lo);
  const bool left = u == 0 || hull_cross(A(u - 1), a, b) < 0;
  const bool right = u == na - 1 || hull_cross(a, A(u + 1), b) >= 0;
  return left && right;
}

// One workgroup per tile of TILE consecutive points; point 0 is the origin, point i > 0 is (pf[i - 1], pt[i - 1]); `points` =
// M + 1.  hull[tile * TILE ..] and count[tile] get the tile's hull.
__global__ __launch_bounds__(RT) void hull_tile_kernel(const unsigned* __restrict__ pf, const unsigned* __restrict__ pt,
                                                       size_t points, uint2* __restrict__ hull, unsigned* __restrict__ count) {
  __shared__ uint2 buf[2][HULL_LDS_POINTS];
  __shared__ int cnt[2][HULL_LEAVES];
  __shared__ int bridge[HULL_LEAVES / 2][2];
  const int t = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * TILE;
  const int tn = (int)std::min<size_t>(TILE, points - first);
  for (int i = t; i < tn; i += RT) {
    const size_t g = first + i;
    buf[0][hull_phys(i)] = g == 0 ? make_uint2(0u, 0u) : make_uint2(pf[g - 1], pt[g - 1]);
  }
  __syncthreads();
  {  // the chain over this thread's leaf, in place: the stack never grows past the point being read
    const int lo = t * HULL_LEAF, len = std::max(0, std::min(HULL_LEAF, tn - lo));
    uint2* leaf = &buf[0][hull_phys(lo)];
    int top = 0;
    for (int k = 0; k < len; ++k) {
      const uint2 c = leaf[k];
      while (top >= 2 && hull_cross(leaf[top - 2], leaf[top - 1], c) >= 0) --top;
      leaf[top++] = c;
    }
    cnt[0][t] = top;
  }
  __syncthreads();
  int cur = 0;
  for (int level = 0; level < HULL_LDS_LEVELS; ++level) {
    const int sub = HULL_LEAF << level;      // points under each of the two hulls of a pair
    const int g = 2 << level;                // threads of a pair
    const int pair = t / g, r = t % g;
    const LdsHull A{buf[cur], 2 * pair * sub}, B{buf[cur], (2 * pair + 1) * sub};
    const int na = cnt[cur][2 * pair], nb = cnt[cur][2 * pair + 1];
    if (r == 0) {   // all of A and none of B: what an absent B leaves; else the one qualifying u below overwrites it
      bridge[pair][0] = na - 1;
      bridge[pair][1] = nb;
    }
    __syncthreads();
    if (nb > 0) {
      for (int u = r; u < na; u += g) {
        int v;
        if (hull_bridge_at(A, na, B, nb, u, &v)) {
          bridge[pair][0] = u;
          bridge[pair][1] = v;
        }
      }
    }
    __syncthreads();
    const int u = bridge[pair][0], v = bridge[pair][1];
    const int total = u + 1 + (nb - v);
    uint2* dst = buf[cur ^ 1];
    for (int i = r; i < total; i += g) dst[hull_phys(2 * pair * sub + i)] = i <= u ? A(i) : B(v + i - u - 1);
    if (r == 0) cnt[cur ^ 1][pair] = total;
    __syncthreads();
    cur ^= 1;
  }
  const int total = cnt[cur][0];
  for (int i = t; i < total; i += RT) hull[first + i] = buf[cur][hull_phys(i)];
  if (t == 0) count[blockIdx.x] = (unsigned)total;
}

// One workgroup per pair of adjacent hulls of `span` points each: src[2 p span ..] with csrc[2 p] vertices and its right
// neighbour (absent behind the last hull of an odd count: A is copied).  dst[2 p span ..] and cdst[p] get the joined hull.
__global__ __launch_bounds__(RT) void hull_merge_kernel(const uint2* __restrict__ src, const unsigned* __restrict__ csrc,
                                                        unsigned hulls, size_t span, uint2* __restrict__ dst,
                                                        unsigned* __restrict__ cdst) {
  __shared__ int bridge[2];
  const unsigned ia = 2 * blockIdx.x, ib = ia + 1;
  const GlobalHull A{src + (size_t)ia * span}, B{src + (size_t)ib * span};
  const int na = (int)csrc[ia], nb = ib < hulls ? (int)csrc[ib] : 0;
  if (threadIdx.x == 0) {   // all of A and none of B: what an absent B leaves; else the one qualifying u below overwrites it
    bridge[0] = na - 1;
    bridge[1] = nb;
  }
  __syncthreads();
  if (nb > 0) {
    for (int u = threadIdx.x; u < na; u += RT) {
      int v;
      if (hull_bridge_at(A, na, B, nb, u, &v)) {
        bridge[0] = u;
        bridge[1] = v;
      }
    }
  }
  __syncthreads();
  const int u = bridge[0], v = bridge[1];
  const int total = u + 1 + (nb - v);
  uint2* out = dst + (size_t)ia * span;
  for (int i = threadIdx.x; i < total; i += RT) out[i] = i <= u ? A(i) : B(v + i - u - 1);
  if (threadIdx.x == 0) cdst[blockIdx.x] = (unsigned)total;
}

// The caller's planes from the finished hull: the vertex's counts and its score, the sorted key of the last pair at or above
// it (element f + t - 1); the origin accepts nothing.
__global__ __launch_bounds__(RT) void hull_emit_kernel(const uint2* __restrict__ hull, unsigned count,
                                                       const unsigned* __restrict__ keys, unsigned* __restrict__ vf,
                                                       unsigned* __restrict__ vt, float* __restrict__ vscore) {
  const unsigned i = blockIdx.x * RT + threadIdx.x;
  if (i >= count) return;
  const uint2 q = hull[i];
  vf[i] = q.x;
  vt[i] = q.y;
  vscore[i] = i == 0 ? INFINITY : key_value(keys[(size_t)q.x + q.y - 1]);
}

// ---- the PAV map ------------------------------------------------------------------------------------------------------------
// The smallest k with s >= edges[k] (descending), the last bin below every edge; a NaN stays itself.
// That k is the number of edges above s among the first n_bins - 1.  The search halves a length that depends on n_bins alone, so
// the trip count is the same for every lane (no divergent loop) and a step is a read, a compare and a conditional add; the answer
// stays within [base, base + len].
__device__ __forceinline__ float pav_lookup(float s, const float* edges, const float* llr, int n_bins) {
  int base = 0, len = n_bins - 1;
  while (len > 1) {
    const int half = len >> 1;
    base += edges[base + half] > s ? half : 0;
    len -= half;
  }
  const int k = len > 0 ? base + (edges[base] > s ? 1 : 0) : 0;
  return s != s ? s : llr[k];
}

// out[0, head) and the elements behind the last whole quad one by one, the quads between as 16-byte loads and stores (VEC: sc
// + head and out + head are 16-byte aligned).  A thread reads what it writes before it writes it, and nobody else touches it:
// out may be sc.  LDS: the table is copied into LDS first (n_bins <= PAV_LDS_BINS).
template <bool LDS, bool VEC>
__global__ __launch_bounds__(RT) void pav_apply_kernel(const float* sc, size_t n, size_t head, const float* __restrict__ g_edges,
                                                       const float* __restrict__ g_llr, int n_bins, float* out) {
  __shared__ float tab[LDS ? 2 * PAV_LDS_BINS : 2];
  const float *edges = g_edges, *llr = g_llr;
  if (LDS) {
    for (int i = threadIdx.x; i < n_bins; i += RT) {
      tab[i] = g_edges[i];
      tab[PAV_LDS_BINS + i] = g_llr[i];
    }
    __syncthreads();
    edges = tab;
    llr = tab + PAV_LDS_BINS;
  }
  const size_t g = (size_t)blockIdx.x * RT + threadIdx.x;
  if (g < head) out[g] = pav_lookup(sc[g], edges, llr, n_bins);
  const size_t quads = (n - head + 3) / 4;
  for (size_t q = g; q < quads; q += (size_t)gridDim.x * RT) {
    const size_t i0 = head + 4 * q;
    if (VEC && i0 + 4 <= n) {
      const float4 s = *reinterpret_cast<const float4*>(sc + i0);
      float4 r;
      r.x = pav_lookup(s.x, edges, llr, n_bins);
      r.y = pav_lookup(s.y, edges, llr, n_bins);
      r.z = pav_lookup(s.z, edges, llr, n_bins);
      r.w = pav_lookup(s.w, edges, llr, n_bins);
      *reinterpret_cast<float4*>(out + i0) = r;
    } else {
      float s[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = i0 + e < n ? sc[i0 + e] : 0.0f;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < n) out[i0 + e] = pav_lookup(s[e], edges, llr, n_bins);
    }
  }
}
