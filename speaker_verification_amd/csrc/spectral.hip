// Spectral clustering for diarization: from a recording's window affinities to the spectral embedding svk_ahc
// clusters, with the speaker count read off the eigengap and the graph's neighbour count chosen by the normalised maximum
// eigengap.  include/svk.h holds the definition; tests/spectral_f64_ref.py states it in NumPy.
//
// svk_spectral_embed    one workgroup of 256 threads per recording, no workgroup waits for another.  In order:
//   nodes       without groups node a is window a; with groups the members of every node are listed in ascending order in the
//               recording's workspace slot and thread (a, b), a < b, adds its |a| |b| affinities one at a time.  The node
//               matrix M sits where L will (the LDS matrix, rows an odd number of float64 apart)
//   ranks       rank[a][b] = how many c beat b in row a (larger M, then lower c): one byte per entry, 16 KiB at 128 nodes.
//               M is not needed afterwards: every candidate graph is `rank < p`, so L is rebuilt in place per candidate
//   Jacobi      cyclic, round-robin ordering: M2 = m rounded up to even, H = M2 / 2 disjoint pairs per round, M2 - 1 rounds per
//               sweep.  A round first computes the H rotations from the matrix as it stands, then applies J^T A J block by
//               block: the task (k, k'), k <= k', owns the 2 x 2 block rows (p_k, q_k) x columns (p_k', q_k'), rotates it from
//               both sides in registers and writes it AND its mirror image, so A stays symmetric bit for bit and every entry is
//               touched by one thread per round: two barriers per round.  A pair's own block takes the same two-sided
//               rotation and a zero for a_pq (the closed form a_pp - t a_pq of the textbooks was tried first: on graphs with
//               many equal eigenvalues it turned quadratic convergence into a linear crawl past 30 sweeps -- DESIGN 3.16).
//               With vectors (the winner only) V^T lives in the workspace slot, row p = eigenvector p, and a rotation mixes two
//               contiguous rows
//   decisions   every thread reads the sorted eigenvalues from LDS and takes the same (uniform) decisions: no broadcast step
// Contraction to FMA is allowed in this file (that is why it is not part of cluster.hip).
#include "svk_internal.h"

namespace {

constexpr int SP_THREADS = 256, SP_WAVES = SP_THREADS / 64;
constexpr int SP_MAX_NODES = 128, SP_MAX_STRIDE = 2048, SP_MAX_SPEAKERS = 16, SP_MAX_SWEEPS = 30;
constexpr double SP_EPS = 2.220446049250313e-16;   // 2^-52

struct SpParams {
  const float* aff;
  int32_t n_rec, stride;
  const int32_t* n_seg;
  const int32_t* group;
  int32_t node_stride, nb_lo, nb_step, nb_count, min_spk, max_spk;
  const int32_t* target;
  char* work;
  float* embed;
  int32_t* n_nodes;
  int32_t* n_speakers;
  int32_t* neighbours;
  double* eigval;
  double* eigvec;
  uint8_t* graph;
  double* ratio;
  int32_t* bad_count;
};

// rows of the LDS matrix and of V^T: node_stride rounded up to even (the round-robin wants an even count), at least 2
__host__ __device__ constexpr int sp_cap(int node_stride) { return std::max(2, (node_stride + 1) & ~1); }
// dynamic LDS: the matrix (cap rows, cap + 1 float64 apart), eigenvalues, the rotations of a round (c, s), then the int
// vectors (order, the pairs of a round, node sizes and starts), then the ranks
__host__ __device__ constexpr size_t sp_lds_bytes(int cap) {
  return sizeof(double) * ((size_t)cap * (cap + 1) + cap + 2 * (cap / 2)) + sizeof(int) * (size_t)(4 * cap) + (size_t)cap * cap;
}
// a recording's workspace slot: V^T (cap x cap float64), then the member list (int32 [seg_stride], rounded to 16 bytes)
__host__ __device__ constexpr size_t sp_slot_bytes(int cap, int stride) {
  return sizeof(double) * (size_t)cap * cap + sizeof(int32_t) * (size_t)((stride + 3) & ~3);
}

struct SpLds {
  double* A;      // [cap][ld]
  double* lam;    // [cap]   sorted eigenvalues (scratch while L is built)
  double* cs;     // [cap / 2]
  double* sn;
  int* ord;       // [cap]   ord[i] = the matrix index of the i-th smallest eigenvalue
  int* pp;        // [cap / 2]
  int* qq;
  int* nsize;     // [cap]
  int* nstart;    // [cap]
  uint8_t* rank;  // [cap][cap]
  int cap, ld;
};

__device__ __forceinline__ SpLds sp_carve(double* smem, int cap) {
  SpLds s;
  s.cap = cap, s.ld = cap + 1;
  s.A = smem;
  s.lam = s.A + (size_t)cap * s.ld;
  s.cs = s.lam + cap;
  s.sn = s.cs + cap / 2;
  s.ord = reinterpret_cast<int*>(s.sn + cap / 2);
  s.pp = s.ord + cap;
  s.qq = s.pp + cap / 2;
  s.nsize = s.qq + cap / 2;
  s.nstart = s.nsize + cap;
  s.rank = reinterpret_cast<uint8_t*>(s.nstart + cap);
  return s;
}

__device__ __forceinline__ bool sp_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }

// the largest value of the workgroup in every thread (red: SP_WAVES slots; the caller's next barrier frees them)
__device__ __forceinline__ double sp_block_max(double v, double* red) {
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) v = fmax(v, __shfl_xor(v, x, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int x = 1; x < SP_WAVES; ++x) v = fmax(v, red[x]);
  return v;
}

// L of the graph `rank < p` in place, then its spectrum: cyclic Jacobi until the largest off-diagonal magnitude is at or below
// 2^-52 ||L||_F, at most SP_MAX_SWEEPS sweeps.  Leaves the eigenvalues ascending in s.lam and their matrix indices in s.ord;
// with Vt != nullptr row i of Vt is the eigenvector of matrix index i.  Returns whether it converged (uniform).
__device__ bool sp_solve(const SpLds& s, int m, int p, double* Vt, double* red) {
  const int tid = threadIdx.x, ld = s.ld, cap = s.cap;
  const int M2 = (m + 1) & ~1, H = M2 / 2;
  double* A = s.A;
  __syncthreads();   // whoever read A or lam before is done
  for (int idx = tid; idx < M2 * M2; idx += SP_THREADS) {
    const int a = idx / M2, b = idx - a * M2;
    double v = 0.0;
    if (a < m && b < m && a != b) v = -0.5 * (double)((s.rank[a * cap + b] < p) + (s.rank[b * cap + a] < p));
    A[a * ld + b] = v;
  }
  if (Vt)
    for (int idx = tid; idx < m * m; idx += SP_THREADS) {
      const int a = idx / m, b = idx - a * m;
      Vt[(size_t)a * cap + b] = a == b ? 1.0 : 0.0;
    }
  __syncthreads();
  // degrees and ||L||_F^2: multiples of 1/2 and 1/4 far below 2^53, so every sum here is exact in any order
  for (int a = tid; a < m; a += SP_THREADS) {
    double d = 0.0, sq = 0.0;
    for (int b = 0; b < m; ++b) {
      const double v = A[a * ld + b];
      d -= v, sq += v * v;
    }
    A[a * ld + a] = d;
    s.lam[a] = sq + d * d;
  }
  __syncthreads();
  double fro2 = 0.0;
  for (int a = 0; a < m; ++a) fro2 += s.lam[a];
  const double tol = SP_EPS * sqrt(fro2);

  bool converged = false;
  for (int sweep = 0; sweep <= SP_MAX_SWEEPS; ++sweep) {
    double off = 0.0;
    for (int idx = tid; idx < m * m; idx += SP_THREADS) {
      const int a = idx / m, b = idx - a * m;
      if (a != b) off = fmax(off, fabs(A[a * ld + b]));
    }
    off = sp_block_max(off, red);
    if (off <= tol) {
      converged = true;
      break;
    }
    if (sweep == SP_MAX_SWEEPS) break;
    for (int r = 0; r < M2 - 1; ++r) {
      if (tid < H) {
        int a, b;
        if (tid == 0) a = M2 - 1, b = r;
        else a = (r + tid) % (M2 - 1), b = (r - tid + (M2 - 1)) % (M2 - 1);
        const int pi = min(a, b), qi = max(a, b);
        const double apq = A[pi * ld + qi];
        double c = 1.0, sv = 0.0;
        if (apq != 0.0) {
          const double theta = (A[qi * ld + qi] - A[pi * ld + pi]) / (2.0 * apq);
          const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          sv = t * c;
        }
        s.pp[tid] = pi, s.qq[tid] = qi, s.cs[tid] = c, s.sn[tid] = sv;
      }
      __syncthreads();
      // the blocks (k, k2), k <= k2: rows k and H - 1 - k of the triangle hold H + 1 of them together
      const int fold = (H + 1) / 2, per = H + 1;
      for (int idx = tid; idx < fold * per; idx += SP_THREADS) {
        const int kk = idx / per, cc = idx - kk * per;
        int k, k2;
        if (cc < H - kk) k = kk, k2 = kk + cc;
        else {
          k = H - 1 - kk;
          if (k == kk) continue;
          k2 = k + (cc - (H - kk));
        }
        const double c1 = s.cs[k], s1 = s.sn[k], c2 = s.cs[k2], s2 = s.sn[k2];
        if (s1 == 0.0 && s2 == 0.0) continue;   // two identities (a pair with the padding index is always one)
        const int p1 = s.pp[k], q1 = s.qq[k];
        const int p2 = s.pp[k2], q2 = s.qq[k2];
        const double x11 = A[p1 * ld + p2], x12 = A[p1 * ld + q2], x21 = A[q1 * ld + p2], x22 = A[q1 * ld + q2];
        const double y11 = c2 * x11 - s2 * x12, y12 = s2 * x11 + c2 * x12;
        const double y21 = c2 * x21 - s2 * x22, y22 = s2 * x21 + c2 * x22;
        const double z11 = c1 * y11 - s1 * y21, z21 = s1 * y11 + c1 * y21;
        const double z12 = c1 * y12 - s1 * y22, z22 = s1 * y12 + c1 * y22;
        if (k == k2) {   // the pair's own block: the rotation annihilates a_pq, which is set to zero outright
          A[p1 * ld + p1] = z11, A[q1 * ld + q1] = z22;
          A[p1 * ld + q1] = 0.0, A[q1 * ld + p1] = 0.0;
          continue;
        }
        A[p1 * ld + p2] = z11, A[p2 * ld + p1] = z11;
        A[p1 * ld + q2] = z12, A[q2 * ld + p1] = z12;
        A[q1 * ld + p2] = z21, A[p2 * ld + q1] = z21;
        A[q1 * ld + q2] = z22, A[q2 * ld + q1] = z22;
      }
      if (Vt)
        for (int idx = tid; idx < H * m; idx += SP_THREADS) {
          const int k = idx / m, i = idx - k * m;
          const double c1 = s.cs[k], s1 = s.sn[k];
          if (s1 == 0.0) continue;
          double* vp = Vt + (size_t)s.pp[k] * cap;
          double* vq = Vt + (size_t)s.qq[k] * cap;
          const double x = vp[i], y = vq[i];
          vp[i] = c1 * x - s1 * y;
          vq[i] = s1 * x + c1 * y;
        }
      __syncthreads();
    }
  }
  // ascending, equal values in the order of their matrix index
  for (int a = tid; a < m; a += SP_THREADS) {
    const double d = A[a * ld + a];
    int pos = 0;
    for (int b = 0; b < m; ++b) {
      const double e = A[b * ld + b];
      pos += e < d || (e == d && b < a);
    }
    s.lam[pos] = d, s.ord[pos] = a;
  }
  __syncthreads();
  return converged;
}

// the largest gap among g_i = lam_{i+1} - lam_i, i = 1 .. min(max_spk, m - 1), and the first i that has it (m >= 2)
__device__ __forceinline__ void sp_gap(const double* lam, int m, int max_spk, double* gap, int* at) {
  double g = lam[1] - lam[0];
  int k = 1;
  const int last = min(max_spk, m - 1);
  for (int i = 2; i <= last; ++i) {
    const double gi = lam[i] - lam[i - 1];
    if (gi > g) g = gi, k = i;
  }
  *gap = g, *at = k;
}

__device__ void sp_reject(const SpParams& p, int rec) {
  const int ns = p.node_stride;
  float* emb = p.embed + (size_t)rec * ns * p.max_spk;
  for (int idx = threadIdx.x; idx < ns * p.max_spk; idx += SP_THREADS) emb[idx] = 0.f;
  if (p.ratio)
    for (int c = threadIdx.x; c < p.nb_count; c += SP_THREADS) p.ratio[(size_t)rec * p.nb_count + c] = __builtin_nan("");
  if (threadIdx.x == 0) {
    p.n_nodes[rec] = p.n_speakers[rec] = p.neighbours[rec] = -1;
    if (p.bad_count) atomicAdd(p.bad_count, 1);
  }
}

__global__ __launch_bounds__(SP_THREADS) void spectral_embed_kernel(const SpParams p) {
  extern __shared__ double sp_smem[];
  __shared__ double red[SP_WAVES];
  __shared__ double sgn[SP_MAX_SPEAKERS];
  __shared__ int m_sh;
  const int tid = threadIdx.x, rec = blockIdx.x, stride = p.stride, ns = p.node_stride;
  const int cap = sp_cap(ns);
  const SpLds s = sp_carve(sp_smem, cap);
  const int ld = s.ld;
  const int n = p.n_seg[rec];
  if (n < 0 || n > stride) {
    sp_reject(p, rec);
    return;
  }
  const float* aff = p.aff + (size_t)rec * stride * stride;
  char* slot = p.work + (size_t)rec * sp_slot_bytes(cap, stride);
  double* Vt = reinterpret_cast<double*>(slot);
  int32_t* members = reinterpret_cast<int32_t*>(slot + sizeof(double) * (size_t)cap * cap);
  double* ratio = p.ratio ? p.ratio + (size_t)rec * p.nb_count : nullptr;

  // ---- nodes: M in the matrix
  int m = n, flag = 0;
  if (p.group) {
    const int32_t* grp = p.group + (size_t)rec * stride;
    if (tid == 0) m_sh = 0;
    for (int a = tid; a < cap; a += SP_THREADS) s.nsize[a] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += SP_THREADS) {
      const int g = grp[i];
      if (g < 0 || g >= ns) flag = 1;
      else atomicAdd(&s.nsize[g], 1), atomicMax(&m_sh, g + 1);   // (integer LDS atomics: counts and a maximum)
    }
    if (__syncthreads_or(flag)) {
      sp_reject(p, rec);
      return;
    }
    m = m_sh;
    for (int a = tid; a < m; a += SP_THREADS) flag |= s.nsize[a] == 0;
    if (__syncthreads_or(flag)) {
      sp_reject(p, rec);
      return;
    }
    if (tid == 0) {
      int at = 0;
      for (int a = 0; a < m; ++a) s.nstart[a] = at, at += s.nsize[a];
    }
    __syncthreads();
    for (int a = tid; a < m; a += SP_THREADS) {   // node a's members in ascending order
      int at = s.nstart[a];
      for (int i = 0; i < n; ++i)
        if (grp[i] == a) members[at++] = i;
    }
    __syncthreads();
    for (int idx = tid; idx < m * m; idx += SP_THREADS) {
      const int a = idx / m, b = idx - a * m;
      if (a == b) s.A[a * ld + a] = 0.0;
      if (a >= b) continue;
      const int na = s.nsize[a], nb = s.nsize[b];
      const int32_t* ma = members + s.nstart[a];
      const int32_t* mb = members + s.nstart[b];
      double acc = 0.0;
      for (int x = 0; x < na; ++x) {
        const int i = ma[x];
        for (int y = 0; y < nb; ++y) {
          const int j = mb[y];
          const double v = (double)aff[(size_t)min(i, j) * stride + max(i, j)];
          flag |= !sp_finite(v);
          acc += v;
        }
      }
      const double mean = acc / (double)(na * nb);
      s.A[a * ld + b] = mean, s.A[b * ld + a] = mean;
    }
  } else {
    for (int idx = tid; idx < m * m; idx += SP_THREADS) {
      const int a = idx / m, b = idx - a * m;
      double v = 0.0;
      if (a != b) {
        v = (double)aff[(size_t)min(a, b) * stride + max(a, b)];
        flag |= !sp_finite(v);
      }
      s.A[a * ld + b] = v;
    }
  }
  if (__syncthreads_or(flag)) {
    sp_reject(p, rec);
    return;
  }

  const int K = p.max_spk;
  float* emb = p.embed + (size_t)rec * ns * K;
  if (ratio)
    for (int c = tid; c < p.nb_count; c += SP_THREADS) ratio[c] = __builtin_nan("");
  if (m <= 1) {
    if (tid == 0) {
      p.n_nodes[rec] = p.n_speakers[rec] = m, p.neighbours[rec] = 0;
      if (m == 1) {
        if (p.eigval) p.eigval[(size_t)rec * ns] = 0.0;
        if (p.eigvec) p.eigvec[(size_t)rec * K * ns] = 1.0;
        if (p.graph) p.graph[(size_t)rec * ns * ns] = 0;
      }
    }
    if (m == 1)
      for (int j = tid; j < K; j += SP_THREADS) emb[j] = j == 0 ? 1.f : 0.f;
    return;
  }

  // ---- ranks: how many c beat b in row a (larger value, then lower c)
  for (int idx = tid; idx < m * m; idx += SP_THREADS) {
    const int a = idx / m, b = idx - a * m;
    int cnt = 255;
    if (a != b) {
      const double v = s.A[a * ld + b];
      cnt = 0;
      for (int c = 0; c < m; ++c) {
        const double w = s.A[a * ld + c];
        cnt += c != a && (w > v || (w == v && c < b));
      }
    }
    s.rank[a * cap + b] = (uint8_t)cnt;
  }
  // (sp_solve opens with a barrier)

  // ---- the neighbour sweep: eigenvalues only, unless there is one candidate
  const bool single = p.nb_count == 1 || p.nb_lo >= m - 1;
  double best_r = 0.0;
  int best_p = -1, last_p = -1;
  bool ok = true;
  for (int c = 0; c < p.nb_count; ++c) {
    const int cand = (int)std::min<int64_t>((int64_t)p.nb_lo + (int64_t)c * p.nb_step, m - 1);
    if (cand == last_p) break;   // clamped to m - 1 a second time: so is every later one
    last_p = cand;
    ok = sp_solve(s, m, cand, single ? Vt : nullptr, red);
    if (!ok) break;
    double gap;
    int at;
    sp_gap(s.lam, m, K, &gap, &at);
    const double r = gap > 0.0 ? (double)cand * s.lam[m - 1] / gap : __builtin_inf();
    if (ratio && tid == 0) ratio[c] = r;
    if (best_p < 0 || r < best_r) best_r = r, best_p = cand;
  }
  if (ok && !single) ok = sp_solve(s, m, best_p, Vt, red);
  if (!ok) {
    __syncthreads();   // thread 0's ratios before the NaNs
    sp_reject(p, rec);
    return;
  }
  double gap;
  int k;
  sp_gap(s.lam, m, K, &gap, &k);
  k = min(max(k, p.min_spk), m);
  if (p.target && p.target[rec] >= 1) k = min(p.target[rec], m);
  k = min(k, K);   // (a target above max_speakers: the embedding has max_speakers columns)

  // ---- outputs
  if (tid < k) {   // the sign: the entry of largest magnitude, the lowest index among equals, is positive
    const double* v = Vt + (size_t)s.ord[tid] * cap;
    double big = -1.0, sg = 1.0;
    for (int a = 0; a < m; ++a)
      if (fabs(v[a]) > big) big = fabs(v[a]), sg = v[a] < 0.0 ? -1.0 : 1.0;
    sgn[tid] = sg;
  }
  __syncthreads();
  for (int idx = tid; idx < m * K; idx += SP_THREADS) {
    const int a = idx / K, j = idx - a * K;
    emb[idx] = j < k ? (float)(sgn[j] * Vt[(size_t)s.ord[j] * cap + a]) : 0.f;
  }
  if (p.eigvec)
    for (int idx = tid; idx < k * m; idx += SP_THREADS) {
      const int j = idx / m, a = idx - j * m;
      p.eigvec[((size_t)rec * K + j) * ns + a] = sgn[j] * Vt[(size_t)s.ord[j] * cap + a];
    }
  if (p.eigval)
    for (int a = tid; a < m; a += SP_THREADS) p.eigval[(size_t)rec * ns + a] = s.lam[a];
  if (p.graph)
    for (int idx = tid; idx < m * m; idx += SP_THREADS) {
      const int a = idx / m, b = idx - a * m;
      p.graph[((size_t)rec * ns + a) * ns + b] =
          a == b ? 0 : (uint8_t)((s.rank[a * cap + b] < best_p) + (s.rank[b * cap + a] < best_p));
    }
  if (tid == 0) p.n_nodes[rec] = m, p.n_speakers[rec] = k, p.neighbours[rec] = best_p;
}

}  // namespace

extern "C" {

int svk_spectral_limits(int32_t out[3]) {
  if (!out) return SVK_ERR_BAD_ARG;
  out[0] = SP_MAX_NODES;
  out[1] = SP_MAX_STRIDE;
  out[2] = SP_MAX_SPEAKERS;
  return SVK_OK;
}

size_t svk_spectral_workspace_bytes(int32_t n_rec, int32_t seg_stride, int32_t node_stride) {
  if (n_rec <= 0 || seg_stride < 0 || seg_stride > SP_MAX_STRIDE || node_stride < 0 || node_stride > SP_MAX_NODES) return 0;
  return (size_t)n_rec * sp_slot_bytes(sp_cap(node_stride), seg_stride);
}

int svk_spectral_embed(svk_ctx* ctx, const float* d_aff, int32_t n_rec, int32_t seg_stride, const int32_t* d_n_seg,
                       const int32_t* d_group, int32_t node_stride, int32_t nb_lo, int32_t nb_step, int32_t nb_count,
                       int32_t min_speakers, int32_t max_speakers, const int32_t* d_target, void* d_workspace,
                       size_t workspace_bytes, float* d_embed, int32_t* d_n_nodes, int32_t* d_n_speakers, int32_t* d_neighbours,
                       double* d_eigval, double* d_eigvec, uint8_t* d_graph, double* d_ratio, int32_t* d_bad_count) {
  if (!ctx) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, n_rec >= 0 && seg_stride >= 0 && node_stride >= 0, "negative shape");
  SVK_REQUIRE(ctx, seg_stride <= SP_MAX_STRIDE, "seg_stride above svk_spectral_limits()[1]");
  SVK_REQUIRE(ctx, node_stride <= SP_MAX_NODES, "node_stride above svk_spectral_limits()[0]");
  SVK_REQUIRE(ctx, nb_lo >= 1 && nb_step >= 1 && nb_count >= 1, "neighbour candidates need nb_lo, nb_step and nb_count of at least 1");
  SVK_REQUIRE(ctx, min_speakers >= 1 && max_speakers >= min_speakers && max_speakers <= SP_MAX_SPEAKERS,
              "speaker bounds need 1 <= min_speakers <= max_speakers <= svk_spectral_limits()[2]");
  if (n_rec == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_group || seg_stride <= node_stride, "without groups every window is a node: seg_stride must not exceed node_stride");
  SVK_REQUIRE(ctx, d_n_seg && d_n_nodes && d_n_speakers && d_neighbours && (d_aff || seg_stride == 0) && (d_embed || node_stride == 0),
              "NULL buffer");
  SVK_REQUIRE(ctx, !misaligned(d_aff, 4) && !misaligned(d_n_seg, 4) && !misaligned(d_group, 4) && !misaligned(d_target, 4) &&
                       !misaligned(d_embed, 4) && !misaligned(d_n_nodes, 4) && !misaligned(d_n_speakers, 4) &&
                       !misaligned(d_neighbours, 4) && !misaligned(d_bad_count, 4) && !misaligned(d_eigval, 8) &&
                       !misaligned(d_eigvec, 8) && !misaligned(d_ratio, 8),
              "misaligned buffer (int32 / f32: 4 bytes, float64: 8)");
  const size_t need = svk_spectral_workspace_bytes(n_rec, seg_stride, node_stride);
  SVK_REQUIRE(ctx, d_workspace && workspace_bytes >= need, "workspace below svk_spectral_workspace_bytes");
  SVK_REQUIRE(ctx, !misaligned(d_workspace, 16), "workspace must be 16-byte aligned");
  const size_t lds = sp_lds_bytes(sp_cap(node_stride));
  if (lds + 256 > (size_t)ctx->lds_per_cu)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "svk_spectral_embed needs %zu bytes of LDS per workgroup (device: %d)", lds, ctx->lds_per_cu);
  SVK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(spectral_embed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const SpParams p{d_aff, n_rec, seg_stride, d_n_seg, d_group, node_stride, nb_lo, nb_step, nb_count, min_speakers, max_speakers,
                   d_target, static_cast<char*>(d_workspace), d_embed, d_n_nodes, d_n_speakers, d_neighbours, d_eigval, d_eigvec,
                   d_graph, d_ratio, d_bad_count};
  hipLaunchKernelGGL(spectral_embed_kernel, dim3((unsigned)n_rec), dim3(SP_THREADS), lds, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
