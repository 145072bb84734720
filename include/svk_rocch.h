/*
 * svk_rocch.h -- C-ABI of libsvk.so, continued: the ROC convex hull (ROCCH) on the device and the PAV map.  Everything svk.h
 * says under "Conventions" holds here (device pointers d_*, host pointers h_*, caller-allocated buffers, svk_status returns,
 * svk_last_error, the context's stream, the memory contract: tests/test_memory_contract_rocch.py holds the entries below to it
 * on guarded buffers).  speaker_verification_amd/_lib.py binds this header's entries in ROCCH_SIGNATURES;
 * tests/test_rocch_host.py checks the two against each other and against the built library.  SVK_VERSION keeps its number.
 */
#ifndef SVK_ROCCH_H
#define SVK_ROCCH_H

#include "svk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the ROC convex hull ---------------------------------------------------------
 * minCllr, the ROCCH-EER and the PAV (isotonic) calibration of a trial set are one object: the upper convex hull of its ROC.
 * PAV's bins are the hull's edges, its posteriors their slopes, minCllr a sum over the edges.
 *
 * The points.  With the n trials sorted by descending score (-0.0 equals +0.0) and every group of equal scores pooled,
 *     Q_0 = (0, 0),   Q_j = (fps_j, tps_j), j = 1 .. M: non-targets / targets with a score at or above the j-th distinct score,
 *     Q_M = (N, P).
 * These are svk_roc_dcf's points (its "points" output is M).  Along the sequence f never decreases and t rises where f stands
 * still: it is lexicographically sorted.
 *
 * The hull.  cross(a, b, c) = (b.f - a.f) (c.t - a.t) - (b.t - a.t) (c.f - a.f).  The hull is the subsequence
 * V_0 = Q_0, ..., V_K = Q_M in which every interior vertex makes a STRICT right turn, cross(V_k-1, V_k, V_k+1) < 0; collinear
 * points are not vertices.  It is what Andrew's monotone chain leaves when it pops while cross >= 0.  n < 2^32 gives
 * N P < 2^62: every cross product is exact in int64, and no floating point takes part in deciding a vertex.  The result is a
 * function of the multiset of (score, label) pairs alone: the stored order of the trials changes nothing, nor does a rerun.
 *
 * Per edge k (V_k-1 -> V_k), dt_k targets and df_k non-targets lie in it:
 *     PAV posterior  dt_k / (dt_k + df_k)
 *     llr_k        = log(dt_k / df_k) - log(P / N)          (+inf for df_k = 0, -inf for dt_k = 0)
 *     e_k          = the score of V_k: the lowest score of the bin, a value of the input
 *     minCllr      = [ (1/P) sum_k dt_k log1p(df_k P / (dt_k N)) + (1/N) sum_k df_k log1p(dt_k N / (df_k P)) ] / (2 ln 2),
 *                    an edge with dt_k = 0 or df_k = 0 contributing 0
 *     ROCCH-EER    : svk_roc_eer's rule on the hull's vertices: on the one edge with g_0 = 1 - f_0/N - t_0/P > 0 >= g_1,
 *                    eer = x_0 + (x_1 - x_0) g_0 / (g_0 - g_1),  x = f / N
 * The library returns the integer vertices and their scores; the derived values are a few float64 operations per edge on the
 * host (speaker_verification_amd/calibration.py).
 *
 * svk_rocch is svk_roc_dcf plus the hull: the same kernels in the same order produce h_out[0 .. 5 + 4 n_op), bit for bit what
 * svk_roc_dcf writes there for the same arguments (see svk.h), and behind svk_roc_dcf's last kernel the hull passes run:
 *   tile pass     one workgroup per 2 048 consecutive points (the origin included), staged in LDS as (f, t) pairs; each thread
 *                 runs the monotone chain over its 8 points, then 8 levels in LDS merge adjacent hulls pairwise
 *   merge levels  ceil(log2(tiles)) kernels, one workgroup per pair of adjacent hulls A, B: the bridge (u, v) -- for a
 *                 candidate u, v(u) is the first i with cross(A[u], B[i], B[i+1]) < 0 (or B's last index), by binary search;
 *                 u is the bridge's left end iff (u == 0 or cross(A[u-1], A[u], B[v]) < 0) and (u == last or
 *                 cross(A[u], A[u+1], B[v]) >= 0); exactly one u qualifies -- and the copy A[0..u] ++ B[v..].  A hull
 *                 stays anchored at the offset of its first point's tile, so no level needs a scan of the counts.
 * Integers only; no atomic, no workgroup waits on another; the number of levels depends on M alone.
 *
 * n, d_scores, d_labels, h_ops, n_op : as for svk_roc_dcf
 * d_workspace  : svk_rocch_workspace_bytes(n) bytes (more than svk_roc_dcf's: two hull buffers of 8 bytes per point)
 * d_vf, d_vt   : [capacity] uint32: fps and tps of the K + 1 vertices, the origin first; elements from K + 1 on are untouched
 * d_vscore     : [capacity] float: the score at each vertex (the threshold "accept when score >= it" that reaches the vertex),
 *                bit for bit a score of the input with -0.0 read as +0.0; the origin gets +inf
 * capacity     : elements of each plane.  svk_rocch_max_vertices(n) always suffices
 * h_out        : [5 + 4 n_op + 1] doubles: svk_roc_dcf's values, then the vertex count K + 1
 *
 * Refusals: everything svk_roc_dcf refuses, in the same words (n < 2, n >= 2^32, more than 8 or malformed operating points,
 * NULL buffers, a non-finite score, a single class, a workspace smaller than svk_rocch_workspace_bytes(n)); NULL planes,
 * capacity < 1; and a capacity below the vertex count: SVK_ERR_BAD_ARG with the count in the message, nothing written to
 * the planes or to h_out.  Synchronous like svk_roc_dcf up to the last kernel, which writes the planes in stream order.
 *
 * Diagnostics.  After a call the workspace holds, from byte svk_rocch_level_counts_offset(n) on (host arithmetic only; 0 for
 * n < 2), uint32 vertex counts: one per tile of the M + 1 points (ceil((M + 1) / 2048) of them), then one per hull of every
 * merge level in turn (half as many each level, rounded up), the last being K + 1.  Their sums per level are the points that
 * survive it (tools/time_rocch.py reports them).  This is for measurement only: where the counts lie is the library's to
 * change between builds, which is why the offset is asked of the library and not derived by the caller.
 *
 * svk_rocch_max_vertices(n) (host arithmetic only, any int64 n; svk_rocch itself takes n < 2^32) is an integer bound on
 * K + 1.  Edges have pairwise distinct slopes, so pairwise distinct vectors (df, dt); at most s + 1 vectors have df + dt = s; the edge vectors sum to (N, P), df + dt over
 * them to n.  The most edges a budget of n buys takes every vector of weight 1, 2, ... in turn: all weights up to S cost
 * T(S) = S (S + 1) (S + 2) / 3 and give C(S) = S (S + 3) / 2 edges.  With S the smallest integer with T(S) >= n,
 * K <= C(S) (~ 1.04 n^(2/3) + 2.2 n^(1/3)), and K <= n trivially: the bound is min(C(S), n) + 1; 0 for n < 1.  For n >= 2^32,
 * which svk_rocch refuses, S is the one of 2^32 - 1.
 */
size_t svk_rocch_workspace_bytes(int64_t n);
size_t svk_rocch_level_counts_offset(int64_t n);
int64_t svk_rocch_max_vertices(int64_t n);
int svk_rocch(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const double* h_ops, int32_t n_op,
              void* d_workspace, size_t workspace_bytes, uint32_t* d_vf, uint32_t* d_vt, float* d_vscore, int64_t capacity,
              double* h_out);

/* ---- the PAV map -----------------------------------------------------------------
 * d_out[p] = d_llr[k] for the smallest k with d_scores[p] >= d_edges[k], the last bin when the score is below every edge:
 * a step function; a score in the gap between two bins goes to the lower bin.  A NaN score stays that NaN.
 * d_edges : [n_bins] float, descending (the e_k above), no NaN; n_bins >= 1
 * d_llr   : [n_bins] float, any values
 * d_out   : [n] float; may be d_scores itself (in place; no other overlap)
 * One binary search per score.  The table sits in LDS for n_bins <= 4096 (32 KiB) and is read from global memory above that.
 * 16-byte loads and stores where d_scores and d_out are equally placed within 16 bytes (an aligned body between a scalar head
 * and tail), scalar ones otherwise; both pointers 4-byte aligned.  Asynchronous on the context's stream.  n == 0 launches
 * nothing.  Refusals: n < 0, n_bins < 1, NULL d_edges / d_llr, NULL d_scores / d_out with n > 0, a misaligned pointer.
 */
int svk_pav_apply(svk_ctx* ctx, const float* d_scores, int64_t n, const float* d_edges, const float* d_llr, int32_t n_bins,
                  float* d_out);

#ifdef __cplusplus
}
#endif

#endif /* SVK_ROCCH_H */
