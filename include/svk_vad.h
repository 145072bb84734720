/*
 * svk_vad.h -- C-ABI of libsvk.so, continued: the level-adaptive VAD.  Everything svk.h says under "Conventions" holds here
 * (device pointers d_*, caller-allocated buffers, svk_status returns, svk_last_error, the context's stream, the memory
 * contract: tests/test_memory_contract_vad_adaptive.py holds the entry below to it on guarded buffers).
 * speaker_verification_amd/_lib.py binds this header's entries in EXT_SIGNATURES; tests/test_vad_adaptive_host.py checks the two
 * against each other and against the built library.
 */
#ifndef SVK_VAD_H
#define SVK_VAD_H

#include "svk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- level-adaptive energy VAD -------------------------------------------------
 * The reference's per-frame decision is webrtcvad.Vad(3) (vad.py:90,152), which adapts to the signal's level;
 * svk_vad_energy replaces it with ONE absolute threshold for every clip, so a quietly recorded clip loses all its frames.
 * This entry is the same framer (vad.py:44-57, Q12), the same ring-buffer hysteresis (vad.py:60-129, Q13), the same
 * compaction and index form as svk_vad_energy -- ring_len, ring_thresh, d_keep, d_seg, d_n_vad_frames, d_voiced,
 * d_voiced_len and d_src_frame mean exactly what they mean there -- with a threshold derived PER CLIP from two order
 * statistics of the clip's own frame energies.  All of it is integer arithmetic; no float is used anywhere.
 *
 * The rule.  A clip of L samples has nf = (2 L - 1) / (2 frame_samples) whole frames, capped at max_vad_frames (the samples
 * of the partial frame behind them are not read); E_f = sum of x^2 over frame f (int64; frame_samples <= 65536 keeps
 * E_f <= 2^46).
 *     rank(q) = (q * (nf - 1)) >> 16
 *     E_lo, E_hi = the rank(floor_q16)-th and the rank(peak_q16)-th smallest of the clip's E_f (0-based; ties are equal values)
 *     A = (E_lo * above_floor_q16) >> 16,   B = (E_hi * below_peak_q16) >> 16     (the products are formed in 128 bits)
 *     T = max(min(A, B), min_threshold * frame_samples)
 *     frame f is speech  iff  E_f > T                                             (strict, like the absolute rule)
 * A clip without a whole frame (nf == 0) has the levels {0, 0, min_threshold * frame_samples} and nothing else.
 *   - below_peak_q16 = 0 is the absolute rule with threshold = min_threshold: every output equals svk_vad_energy's.
 *   - with min_threshold = 0, multiplying every sample by 2^k (without clipping) changes no decision: E scales by 4^k exactly
 *     and the floor of the shift moves T by less than one unscaled unit.
 *   - a clip with no speech at all is kept whole unless min_threshold is set: the rule has only the clip's own levels.
 *     min_threshold is the caller's absolute floor and costs the exact invariance.
 *
 * floor_q16, peak_q16 : the two quantiles times 65536, in [0, 65536], floor_q16 <= peak_q16
 * above_floor_q16     : a linear power ratio times 65536, in [65536, 2^40]: T is at least this far above the floor level ...
 * below_peak_q16      : a linear power ratio times 65536, in [0, 65536]: ... but no higher than this far below the peak level
 * min_threshold       : >= 0, per sample like svk_vad_energy's threshold; min_threshold * frame_samples must fit 63 bits
 * d_levels            : [n_utt][3] int64 = {E_lo, E_hi, T} per clip, or NULL
 * d_energy            : [n_utt][max_vad_frames] int64, E_f of the clip's frames; entries from the clip's frame count on are
 *                       left untouched; or NULL
 *
 * Refusals, each with a message that names the parameter and with no output written: SVK_ERR_BAD_ARG for a quantile or a
 * ratio outside its domain, floor_q16 > peak_q16, a negative min_threshold or one whose product with frame_samples overflows,
 * NULL d_pcm / d_keep, d_voiced or d_src_frame without d_voiced_len, d_voiced == d_pcm; SVK_ERR_UNSUPPORTED for
 * frame_samples > 65536 and for max_vad_frames > 8192.  n_utt == 0 launches nothing.
 *
 * Asynchronous on the context's stream, no host round trip; workspaces come from the handle.  Routes (SVK_VAD_SPLIT = 0 / 1 / 2
 * forces them as for svk_vad_energy: 1 the long-clip route, 2 the general one, 0 never the long-clip route):
 *   short clips   frame_samples a multiple of 8 and <= 512, max_vad_frames <= 512: one kernel per clip; the energies stay in
 *                 LDS, the order statistics come from rank counting
 *   long clips    same frame geometry, max_vad_frames > 512: frame energies over frame chunks of the whole grid, then one
 *                 workgroup per clip selects both order statistics exactly (radix select over the 8-bit digits of the 48-bit
 *                 energies) and writes levels and flags, then svk_vad_energy's own walk and copy kernels
 *   general       any other frame_samples: the same energy and select kernels with a frame loop for any length and
 *                 alignment, then svk_vad_energy's general kernel for the walk and the copy
 * On the last two the energies go through d_energy when it is given and through the handle's workspace otherwise.
 */
int svk_vad_adaptive(svk_ctx* ctx, const int16_t* d_pcm, const int64_t* d_offsets, const int32_t* d_lengths,
                     int64_t clip_stride, int32_t clip_len, int32_t n_utt, int32_t frame_samples,
                     int32_t ring_len, int32_t ring_thresh,
                     int32_t floor_q16, int32_t peak_q16, int64_t above_floor_q16, int64_t below_peak_q16,
                     int64_t min_threshold, int32_t max_vad_frames,
                     uint8_t* d_keep, int32_t* d_seg, int32_t* d_n_vad_frames, int16_t* d_voiced,
                     int32_t* d_voiced_len, int32_t* d_src_frame, int64_t* d_levels, int64_t* d_energy);

#ifdef __cplusplus
}
#endif

#endif /* SVK_VAD_H */
