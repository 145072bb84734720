/*
 * svk_cluster.h -- C-ABI of libsvk.so, continued: corpus clustering from k-NN lists.  Everything svk.h says under
 * "Conventions" holds here (device pointers d_*, caller-allocated buffers, svk_status returns, svk_last_error, the context's
 * stream, the memory contract: tests/test_memory_contract_cluster.py holds the entry below to it on guarded buffers).
 * speaker_verification_amd/_lib.py binds this header's entries in CLUSTER_SIGNATURES; tests/test_knn_cluster_host.py checks the
 * two against each other and against the built library.  SVK_VERSION keeps its number.
 */
#ifndef SVK_CLUSTER_H
#define SVK_CLUSTER_H

#include "svk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- shared-neighbour (Jarvis-Patrick) clustering of k-NN lists -------------------
 * svk_knn_cluster labels the n rows of a corpus by the connected components of a graph whose edges are read off the rows'
 * k-nearest-neighbour lists, as svk_cosine_topk writes them for a self-search (d_exclude = the row itself).  No [n x n]
 * matrix and no host round trip; every output is defined in integers, so it is a function of the inputs alone and the same
 * bytes on every run.  tests/knn_cluster_ref.py restates the rule below in plain Python.
 *
 * Input.  d_nbr_index int64 [n][list_stride], d_nbr_score f32 [n][list_stride], best first.  Only the first k slots of a row
 * are read, 1 <= k <= 32, k <= list_stride: k < list_stride gives what a search with that smaller k gives.
 *
 * Slots.  A slot of row i is EMPTY if its index is -1.  It is BAD if its index is < -1 or >= n, equals i, or repeats the
 * index of an earlier slot of the same row.  A bad slot is counted once in n_bad, treated as empty and never followed: no
 * index is dereferenced before it is known to lie in [0, n).  N(i) is the set of indices in row i's valid (neither empty nor
 * bad) slots, whatever their scores.
 *
 * Arcs.  The arc i -> j holds iff j is in N(i) and that slot's score s satisfies  s >= threshold  as an IEEE float32
 * comparison: a NaN score fails, -0 >= +0 holds.  threshold = -inf switches the test off: every valid slot is an arc, a NaN
 * score included.  A NaN threshold is SVK_ERR_BAD_ARG.
 *
 * Edges.  flags & 1 ("mutual"): {i, j} is an edge iff i -> j AND j -> i, each arc by its own list's score (the two scores of
 * a pair need not be the same bits).  Bit 0 clear: iff i -> j OR j -> i.  In both modes  |N(i) & N(j)| >= min_shared  is
 * required as well; min_shared in [0, 32], 0 disables the test.  Every other bit of flags must be 0.
 *
 * Outputs, all int32 on the device.
 * d_root   : [n]  the smallest row index of row i's connected component
 * d_labels : [n]  components of at least min_size rows (min_size >= 1) are numbered 0 .. C-1 in increasing order of their
 *                 smallest member; d_labels[i] is that number, -1 for the rows of smaller components
 * d_sizes  : [n]  the sizes of clusters 0 .. C-1, then zeros
 * d_counts : [4]  {C, rows labelled -1, n_bad, gave_up}.  gave_up is 0 unless a bounded loop of the union-find ran out (a
 *                 find is given n steps, a hook n retries; neither is reached); when it is 1 the other outputs are undefined
 * n <= 2^31 - 1.  n == 0 launches nothing and writes d_counts = 0; the other buffers are then not touched and may be NULL.
 *
 * d_workspace: at least svk_knn_cluster_workspace_bytes(n, k) bytes, 16-byte aligned (NULL allowed where that is 0); the size
 * depends on the shape alone and is 0 for arguments the entry refuses (host arithmetic only).  d_nbr_index 8-byte aligned,
 * every other buffer 4-byte aligned.
 * SVK_ERR_BAD_ARG: NULL context or buffer, negative n or n above 2^31 - 1, k outside [1, 32], list_stride < k, min_shared
 * outside [0, 32], min_size < 1, NaN threshold, undefined flag bits, misalignment, short workspace.
 * Asynchronous on the context's stream.
 */
#define SVK_KNN_CLUSTER_MUTUAL 1

size_t svk_knn_cluster_workspace_bytes(int64_t n, int32_t k);
int svk_knn_cluster(svk_ctx* ctx, const float* d_nbr_score, const int64_t* d_nbr_index, int64_t n, int32_t k,
                    int64_t list_stride, float threshold, int32_t min_shared, int32_t min_size, int32_t flags,
                    void* d_workspace, size_t workspace_bytes, int32_t* d_labels, int32_t* d_root, int32_t* d_sizes,
                    int32_t* d_counts);

#ifdef __cplusplus
}
#endif

#endif /* SVK_CLUSTER_H */
