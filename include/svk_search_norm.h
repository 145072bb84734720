/*
 * svk_search_norm.h -- C-ABI of libsvk.so, continued: the speaker search ranked by normalised scores.  Everything svk.h says
 * under "Conventions" holds here (device pointers d_*, caller-allocated buffers, svk_status returns, svk_last_error, the
 * context's stream, the memory contract: tests/test_memory_contract_search_norm.py holds the entry below to it on guarded
 * buffers).  speaker_verification_amd/_lib.py binds this header's entries in SEARCH_NORM_SIGNATURES;
 * tests/test_search_norm_host.py checks the two against each other and against the built library.  SVK_VERSION keeps its number.
 */
#ifndef SVK_SEARCH_NORM_H
#define SVK_SEARCH_NORM_H

#include "svk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- top-k search on normalised scores -------------------------------------------
 * svk_cosine_topk_norm is svk_cosine_topk (svk.h) in every respect except that it selects, merges and accumulates NORMALISED
 * scores: the Z- / T- / S-norm of svk_score_norm sits inside the selection, and the [n_query x n_gallery] matrix is never
 * written.  For a fixed query the normalised score is no monotone function of the raw score across gallery rows (every row
 * has its own mean and deviation), so this ranking cannot be recovered from svk_cosine_topk's lists.
 *
 * The raw score s of (query row, gallery row) has exactly the bits svk_cosine_topk gives that pair: the same K order and
 * the same acc * 1/|q| * 1/|g|.
 *
 * The ranked and returned score is svk_score_norm's expression on s, bit for bit:
 *     both tables   f32(0.5 * ((s - mu_q) / sd_q + (s - mu_g) / sd_g))
 *     one table     f32((s - mu) / sd)
 * Each difference, quotient, sum and product is float64 and rounded on its own, in the order written, with no contraction.
 * A zero, negative or NaN sd, or a NaN moment, gives what IEEE arithmetic gives; nothing is clamped.
 *
 * The order is svk_cosine_topk's total order applied to the normalised value: higher first, NaN above every number,
 * -0 equal to +0, the lower index among equal normalised scores, empty slots (-inf, -1) last.  The order is total and a
 * score's bits depend on its two rows, their two moment pairs and dim alone, so the result is the same bytes for any split
 * into spans, chunks, k, batch or run.
 *
 * d_query_moments   : [n_query][2] float64 {mean, std} of the query rows (the T-norm side: svk_score_norm's row table), or NULL
 * d_gallery_moments : [n_gallery][2] float64 {mean, std} of THIS call's gallery rows (the Z-norm side: the column table), or
 *                     NULL.  Row j of the table belongs to row j of d_gallery, whatever index_base is
 * Both as svk_cohort_moments writes them; 8-byte aligned; read only in their [n][2] extent.  Both NULL is SVK_ERR_BAD_ARG:
 * svk_cosine_topk exists for that.  A table is GIVEN by its pointer: the table of an empty side (n_query or n_gallery of 0,
 * a chunk without rows) is never read, but only a non-NULL pointer says that it is there.
 * flags & 1 (accumulate): the lists already in the outputs are NORMALISED scores of earlier calls (other chunks of the
 *                     gallery under the same query table).  d_exclude and index_base are global, as in svk_cosine_topk.
 * Every other argument, the empty-query and empty-gallery cases, the refusals and the workspace rule are svk_cosine_topk's.
 * svk_cosine_topk_norm_workspace_bytes gives the workspace size (host arithmetic only; 0 for arguments the entry refuses).
 * Asynchronous on the context's stream.
 */
size_t svk_cosine_topk_norm_workspace_bytes(int32_t n_query, int32_t n_gallery, int32_t dim, int32_t k);
int svk_cosine_topk_norm(svk_ctx* ctx, const float* d_query, int32_t n_query, const float* d_gallery, int32_t n_gallery,
                         int32_t dim, int32_t k, int64_t index_base, const int64_t* d_exclude, int32_t flags,
                         const double* d_query_moments, const double* d_gallery_moments, void* d_workspace,
                         size_t workspace_bytes, float* d_top_score, int64_t* d_top_index);

#ifdef __cplusplus
}
#endif

#endif /* SVK_SEARCH_NORM_H */
