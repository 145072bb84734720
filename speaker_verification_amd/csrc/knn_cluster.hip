// Corpus clustering from k-NN lists: svk_knn_cluster (the rule: include/svk.h, "shared-neighbour (Jarvis-Patrick)
// clustering of k-NN lists").  The kernels, the workspace layout, the launch sequence and, at the end, the two entries;
// everything here is int32 / uint32 arithmetic except one float32 comparison per slot.
//
// knn_edge_kernel    TWO rows per wave, one on each 32-lane half (k <= 32: a row's slots fit a half, and at k = 32 no lane
//                    idles).  Lane `slot` of a half holds slot `slot` of its row: it range-checks the index (a bad or empty slot
//                    becomes -1 and is never followed), finds duplicates by k - 1 half-wide broadcasts, and takes the forward
//                    arc from its own score.  Then, slot by slot, the half gathers that neighbour's list (one row of
//                    8 * list_stride bytes, its first k slots only), finds the reverse arc with a ballot (the FIRST slot of the
//                    neighbour that names this row is its valid one: a later one is a duplicate) and counts |N(i) & N(j)| by k
//                    broadcast compares (a duplicate in the neighbour's list changes no set, so the neighbour's list needs no
//                    duplicate pass).  A neighbour whose edge the forward arc already decides is not gathered.  Output: one
//                    uint32 mask per row, bit a = slot a's edge survives, and parent[i] = i.  No atomics but the n_bad count.
// knn_hook_kernel    lock-free union-find, one thread per row, over the row's surviving slots (mutual mode: from the larger
//                    endpoint only, the edge set is symmetric).  A hook links the LARGER root under the smaller with atomicCAS,
//                    so parent[x] <= x always, a parent only ever decreases (path halving goes through atomicMin), and a tree's
//                    root is its minimum whatever the interleaving.  Nothing waits for another thread: a failed CAS returns the
//                    smaller parent somebody else installed, and the hook goes on from there.  Reads of `parent` are relaxed
//                    agent-scope loads (the XCDs' L2s are not coherent); a stale value is still an ancestor, so it costs a
//                    retry, never the result.  Every loop is bounded: a find by n steps, a hook by n retries; an overrun sets
//                    counts[3] and the thread leaves.
// knn_flatten_kernel (next launch) root[i] = the top of i's chain, written over parent[i] in place -- a reader meanwhile sees
//                    the old parent or the root, both ancestors -- and size[root] += 1 (integer atomic).
// knn_part / knn_scan / knn_emit   roc.hip's part / scan / emit pattern restated on one flag per row (a root whose size is >=
//                    min_size): per-tile counts, one block's exclusive scan of the tile counts (the total is C), then every
//                    flagged root writes its cluster's size to sizes[label] and keeps the label in its size slot.
// knn_label_kernel   labels[i] = the label its root kept, the -1 rows counted (integer atomic), sizes[C ..] zeroed.
#include "svk_internal.h"

namespace {

constexpr int KC_THREADS = 256;
constexpr int KC_ITEMS = 8;                          // rows per thread of the part / emit kernels
constexpr int KC_TILE = KC_THREADS * KC_ITEMS;       // rows per tile of the scan
enum { KC_COUNT_CLUSTERS = 0, KC_COUNT_UNLABELLED = 1, KC_COUNT_BAD = 2, KC_COUNT_GAVE_UP = 3 };

struct KnnLayout {
  size_t mask, size, part, total;
};

inline KnnLayout knn_layout(size_t n) {
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  KnnLayout l;
  l.mask = 0;                                        // uint32 [n]  the surviving slots of every row
  l.size = l.mask + up(4 * n);                       // int32 [n]   a root's component size, then its label (-1: too small)
  l.part = l.size + up(4 * n);                       // int32 [tiles]  flagged roots per tile, then their exclusive scan
  l.total = l.part + up(4 * ((n + KC_TILE - 1) / KC_TILE));
  return l;
}

__device__ __forceinline__ unsigned kc_half_ballot(bool p, int half) { return (unsigned)(__ballot(p) >> (32 * half)); }

__global__ __launch_bounds__(KC_THREADS) void knn_edge_kernel(const float* __restrict__ score, const int64_t* __restrict__ index,
                                                              int64_t n, int k, int64_t stride, float thr, int test_score,
                                                              int min_shared, int mutual, uint32_t* __restrict__ mask,
                                                              int32_t* __restrict__ parent, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63, slot = lane & 31, half = lane >> 5;
  const int64_t row = ((int64_t)blockIdx.x * KC_THREADS + threadIdx.x) >> 5;
  const bool live = row < n;
  const int me = (int)row;
  int w = -1;                     // this slot's neighbour, -1 while empty or bad
  bool bad = false, fwd = false;
  if (live && slot < k) {
    const int64_t v = index[row * stride + slot];
    if (v != -1) {
      if (v < 0 || v >= n || v == row) {
        bad = true;
      } else {
        w = (int)v;
        fwd = !test_score || score[row * stride + slot] >= thr;
      }
    }
  }
  bool dup = false;
  for (int b = 0; b + 1 < k; ++b) {
    const int o = __shfl(w, b, 32);
    dup |= b < slot && w >= 0 && o == w;
  }
  if (dup) {
    bad = true;
    fwd = false;
    w = -1;
  }
  const int n_bad = __popcll(__ballot(bad));
  if (lane == 0 && n_bad) atomicAdd(&counts[KC_COUNT_BAD], n_bad);

  uint32_t m = 0;
  for (int a = 0; a < k; ++a) {
    const int j = __shfl(w, a, 32);
    const bool f = __shfl((int)fwd, a, 32) != 0;
    // mutual: no forward arc, no edge.  Either arc: the forward arc decides unless the shared-neighbour test is on.
    const bool gather = j >= 0 && (mutual ? f : (!f || min_shared > 0));
    if (__ballot(gather) == 0) {
      m |= (uint32_t)(j >= 0 && !mutual && f) << a;
      continue;
    }
    int wj = -1;
    bool names_me_ok = false;
    if (gather && slot < k) {
      const int64_t v = index[(int64_t)j * stride + slot];
      wj = (v >= 0 && v < n && v != j) ? (int)v : -1;
      if (wj == me) names_me_ok = !test_score || score[(int64_t)j * stride + slot] >= thr;
    }
    const unsigned names_me = kc_half_ballot(wj == me, half), ok = kc_half_ballot(names_me_ok, half);
    const bool rev = names_me != 0 && ((ok >> (__ffs(names_me) - 1)) & 1u);
    bool shared_ok = true;
    if (min_shared > 0) {
      bool in = false;
      for (int b = 0; b < k; ++b) in |= __shfl(wj, b, 32) == w;
      shared_ok = __popc(kc_half_ballot(in && w >= 0, half)) >= min_shared;
    }
    const bool edge = j >= 0 && (gather ? shared_ok && (mutual ? f && rev : f || rev) : !mutual && f);
    m |= (uint32_t)edge << a;
  }
  if (live && slot == 0) {
    mask[row] = m;
    parent[row] = me;
  }
}

__device__ __forceinline__ int kc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree, halving the path on the way; -1 after n steps (gave_up).
__device__ int kc_find(int32_t* parent, int x, int64_t n, int32_t* counts) {
  for (int64_t step = 0; step <= n; ++step) {
    const int p = kc_load(parent + x);
    if (p == x) return x;
    const int g = kc_load(parent + p);
    if (g != p) atomicMin(parent + x, g);
    x = g;
  }
  counts[KC_COUNT_GAVE_UP] = 1;
  return -1;
}

__device__ void kc_unite(int32_t* parent, int u, int v, int64_t n, int32_t* counts) {
  for (int64_t tries = 0; tries <= n; ++tries) {
    u = kc_find(parent, u, n, counts);
    v = u < 0 ? -1 : kc_find(parent, v, n, counts);
    if (v < 0 || u == v) return;
    const int hi = max(u, v), lo = min(u, v);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    u = old;                    // hi was hooked meanwhile: its parent went down to `old`
    v = lo;
  }
  counts[KC_COUNT_GAVE_UP] = 1;
}

__global__ __launch_bounds__(KC_THREADS) void knn_hook_kernel(const int64_t* __restrict__ index, int64_t n, int64_t stride, int mutual,
                                                              const uint32_t* __restrict__ mask, int32_t* parent, int32_t* counts) {
  const int64_t row = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x;
  if (row >= n) return;
  const int me = (int)row;
  for (uint32_t m = mask[row]; m; m &= m - 1) {
    const int j = (int)index[row * stride + (__ffs(m) - 1)];       // a surviving slot: the edge kernel found it in [0, n)
    if (mutual && j > me) continue;
    kc_unite(parent, me, j, n, counts);
  }
}

__global__ __launch_bounds__(KC_THREADS) void knn_flatten_kernel(int64_t n, int32_t* root, int32_t* __restrict__ size, int32_t* counts) {
  const int64_t row = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x;
  if (row >= n) return;
  int r = (int)row;
  int64_t step = 0;
  for (; step <= n; ++step) {
    const int p = kc_load(root + r);
    if (p == r) break;
    r = p;
  }
  if (step > n) {
    counts[KC_COUNT_GAVE_UP] = 1;
    return;
  }
  __hip_atomic_store(root + row, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(&size[r], 1);
}

// Exclusive scan of one int per thread over the workgroup's KC_THREADS threads; *total = the sum.  lds: 4 ints.
__device__ __forceinline__ int kc_block_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int q = 0; q < KC_THREADS / 64; ++q) {
    base += q < wave ? lds[q] : 0;
    sum += lds[q];
  }
  __syncthreads();
  *total = sum;
  return base + inc - v;
}

__device__ __forceinline__ bool kc_flag(const int32_t* root, const int32_t* size, int64_t i, int64_t n, int min_size) {
  return i < n && root[i] == (int)i && size[i] >= min_size;
}

__global__ __launch_bounds__(KC_THREADS) void knn_part_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                              int64_t n, int min_size, int32_t* __restrict__ part) {
  __shared__ int lds[KC_THREADS / 64];
  const int64_t first = (int64_t)blockIdx.x * KC_TILE + (int64_t)threadIdx.x * KC_ITEMS;
  int c = 0;
#pragma unroll
  for (int e = 0; e < KC_ITEMS; ++e) c += kc_flag(root, size, first + e, n, min_size);
  int total;
  kc_block_scan(c, lds, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(KC_THREADS) void knn_scan_kernel(int32_t* __restrict__ part, int64_t tiles, int32_t* __restrict__ counts) {
  __shared__ int lds[KC_THREADS / 64];
  int carry = 0;
  for (int64_t base = 0; base < tiles; base += KC_THREADS) {
    const int64_t t = base + threadIdx.x;
    const int v = t < tiles ? part[t] : 0;
    int total;
    const int before = kc_block_scan(v, lds, &total);
    if (t < tiles) part[t] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) counts[KC_COUNT_CLUSTERS] = carry;
}

__global__ __launch_bounds__(KC_THREADS) void knn_emit_kernel(const int32_t* __restrict__ root, int32_t* __restrict__ size, int64_t n,
                                                              int min_size, const int32_t* __restrict__ part,
                                                              int32_t* __restrict__ sizes) {
  __shared__ int lds[KC_THREADS / 64];
  const int64_t first = (int64_t)blockIdx.x * KC_TILE + (int64_t)threadIdx.x * KC_ITEMS;
  int c = 0;
#pragma unroll
  for (int e = 0; e < KC_ITEMS; ++e) c += kc_flag(root, size, first + e, n, min_size);
  int total;
  int label = part[blockIdx.x] + kc_block_scan(c, lds, &total);
  for (int e = 0; e < KC_ITEMS; ++e) {
    const int64_t i = first + e;
    if (i >= n || root[i] != (int)i) continue;
    const int s = size[i];
    if (s >= min_size) {
      sizes[label] = s;           // label <= i: clusters are numbered in the order of their smallest member
      size[i] = label++;
    } else {
      size[i] = -1;
    }
  }
}

__global__ __launch_bounds__(KC_THREADS) void knn_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                               int64_t n, int32_t* __restrict__ labels, int32_t* __restrict__ sizes,
                                                               int32_t* counts) {
  const int64_t row = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x;
  int label = 0;
  if (row < n) {
    label = size[root[row]];
    labels[row] = label;
    if (row >= counts[KC_COUNT_CLUSTERS]) sizes[row] = 0;
  }
  const int unlabelled = __popcll(__ballot(label < 0));
  if ((threadIdx.x & 63) == 0 && unlabelled) atomicAdd(&counts[KC_COUNT_UNLABELLED], unlabelled);
}

// The launches of svk_knn_cluster, n >= 1, arguments checked.  d_root doubles as the union-find's parent array.
inline int knn_cluster_launch(svk_ctx* ctx, const float* d_score, const int64_t* d_index, int64_t n, int k, int64_t stride, float thr,
                              int min_shared, int min_size, int mutual, void* d_workspace, int32_t* d_labels, int32_t* d_root,
                              int32_t* d_sizes, int32_t* d_counts) {
  const KnnLayout l = knn_layout((size_t)n);
  char* ws = static_cast<char*>(d_workspace);
  uint32_t* mask = reinterpret_cast<uint32_t*>(ws + l.mask);
  int32_t* size = reinterpret_cast<int32_t*>(ws + l.size);
  int32_t* part = reinterpret_cast<int32_t*>(ws + l.part);
  const int64_t tiles = (n + KC_TILE - 1) / KC_TILE;
  const dim3 threads(KC_THREADS), per_row((unsigned)((n + KC_THREADS - 1) / KC_THREADS)), per_tile((unsigned)tiles);
  const int test_score = !(thr == -INFINITY);
  SVK_HIP(ctx, hipMemsetAsync(d_counts, 0, 4 * sizeof(int32_t), ctx->stream));
  SVK_HIP(ctx, hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)n, ctx->stream));
  hipLaunchKernelGGL(knn_edge_kernel, dim3((unsigned)((n + KC_THREADS / 32 - 1) / (KC_THREADS / 32))), threads, 0, ctx->stream, d_score,
                     d_index, n, k, stride, thr, test_score, min_shared, mutual, mask, d_root, d_counts);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(knn_hook_kernel, per_row, threads, 0, ctx->stream, d_index, n, stride, mutual, mask, d_root, d_counts);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(knn_flatten_kernel, per_row, threads, 0, ctx->stream, n, d_root, size, d_counts);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(knn_part_kernel, per_tile, threads, 0, ctx->stream, d_root, size, n, min_size, part);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(knn_scan_kernel, dim3(1), threads, 0, ctx->stream, part, tiles, d_counts);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(knn_emit_kernel, per_tile, threads, 0, ctx->stream, d_root, size, n, min_size, part, d_sizes);
  SVK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(knn_label_kernel, per_row, threads, 0, ctx->stream, d_root, size, n, d_labels, d_sizes, d_counts);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // namespace

extern "C" {

size_t svk_knn_cluster_workspace_bytes(int64_t n, int32_t k) {
  if (n <= 0 || n > INT32_MAX || k < 1 || k > 32) return 0;
  return knn_layout((size_t)n).total;
}

int svk_knn_cluster(svk_ctx* ctx, const float* d_nbr_score, const int64_t* d_nbr_index, int64_t n, int32_t k, int64_t list_stride,
                    float threshold, int32_t min_shared, int32_t min_size, int32_t flags, void* d_workspace, size_t workspace_bytes,
                    int32_t* d_labels, int32_t* d_root, int32_t* d_sizes, int32_t* d_counts) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n >= 0, "negative shape");
  SVK_REQUIRE(ctx, n <= INT32_MAX, "n above 2^31 - 1 (labels are int32)");
  SVK_REQUIRE(ctx, k >= 1 && k <= 32, "k outside [1, 32]");
  SVK_REQUIRE(ctx, list_stride >= k, "list_stride below k");
  SVK_REQUIRE(ctx, min_shared >= 0 && min_shared <= 32, "min_shared outside [0, 32]");
  SVK_REQUIRE(ctx, min_size >= 1, "min_size below 1");
  SVK_REQUIRE(ctx, threshold == threshold, "threshold is NaN");
  SVK_REQUIRE(ctx, (flags & ~SVK_KNN_CLUSTER_MUTUAL) == 0, "undefined flag bits");
  SVK_REQUIRE(ctx, d_counts && (n == 0 || (d_nbr_score && d_nbr_index && d_labels && d_root && d_sizes)), "NULL buffer");
  SVK_REQUIRE(ctx, !misaligned(d_nbr_index, 8) && !misaligned(d_nbr_score, 4) && !misaligned(d_labels, 4) && !misaligned(d_root, 4) &&
                       !misaligned(d_sizes, 4) && !misaligned(d_counts, 4), "misaligned buffer (int32 / f32: 4 bytes, int64: 8)");
  if (n == 0) {
    SVK_HIP(ctx, hipMemsetAsync(d_counts, 0, 4 * sizeof(int32_t), ctx->stream));
    return SVK_OK;
  }
  SVK_REQUIRE(ctx, d_workspace && workspace_bytes >= svk_knn_cluster_workspace_bytes(n, k),
              "workspace below svk_knn_cluster_workspace_bytes");
  SVK_REQUIRE(ctx, !misaligned(d_workspace, 16), "workspace must be 16-byte aligned");
  return knn_cluster_launch(ctx, d_nbr_score, d_nbr_index, n, k, list_stride, threshold, min_shared, min_size,
                            flags & SVK_KNN_CLUSTER_MUTUAL, d_workspace, d_labels, d_root, d_sizes, d_counts);
}

}  // extern "C"
