/*
 * svk.h -- C-ABI of libsvk.so: the MI355X (gfx950) speaker-verification hot path.
 *
 * The reference (MingmChen/Speaker_Verification) is 100 % Python and has no FFI
 * layer; its boundary for this path is the Python API of its vendored SpeechPy
 * plus vad.py / evaluation.py / siamese.py.  Each entry point below names the
 * reference function(s) (file:line under /root/reference) whose arithmetic it
 * replaces; `speaker_verification_amd/` binds them with ctypes and re-exposes the
 * reference's own Python signatures.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer named d_* is a DEVICE pointer
 *     (hipMalloc'd / a torch tensor's data_ptr()), every h_* a host pointer.
 *   - the caller allocates every input and output; the library owns only what it
 *     returns through svk_create / svk_*_plan_create and frees it in *_destroy.
 *   - every function returns SVK_OK (0) or a negative svk_status; no exceptions,
 *     no aborts.  svk_last_error(ctx) holds a message for the last failure.
 *   - launches go to the stream set by svk_set_stream (default: the null stream)
 *     and are asynchronous w.r.t. the host; svk_sync waits for that stream.
 *   - a context is bound to one device and is not thread-safe.
 *   - the memory contract (tests/memory_contract.py; tests/test_memory_contract_{scoring,backend,evaluation,diarization,
 *     frontend,stages,ingest,network,vad_adaptive,rocch,search_norm,cluster}.py hold every entry that touches device memory to it on guarded buffers, and
 *     tests/test_memory_contract_helper.py walks the sources so that none is left out):
 *       a call writes only the buffers it documents as outputs, and only the elements it documents -- nothing in front of a
 *       buffer, behind it, in the padding between strided rows or in elements an entry calls "not written";
 *       the contents of workspaces and outputs on entry change no result (a workspace of exactly svk_*_workspace_bytes
 *       bytes is enough, whatever it holds; lists an accumulate flag reads and counters "the caller zeroes" are inputs);
 *       bytes beyond an input's documented extent -- behind its last element, in stride padding, in rows or entries an
 *       entry calls "not read" -- change no result.
 */
#ifndef SVK_H
#define SVK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVK_VERSION 114 /* 0.1.12; what each version added: History, at the end of this header */

typedef enum svk_status {
  SVK_OK = 0,
  SVK_ERR_BAD_ARG = -1,      /* NULL pointer, negative size, inconsistent shape   */
  SVK_ERR_UNSUPPORTED = -2,  /* a parameter combination the kernels do not cover  */
  SVK_ERR_HIP = -3,          /* a HIP runtime call failed (message has the code)  */
  SVK_ERR_NO_DEVICE = -4,    /* no usable gfx950 device                           */
  SVK_ERR_OOM = -5,
  SVK_ERR_RCCL = -6          /* RCCL could not be loaded or a collective failed   */
} svk_status;

typedef struct svk_ctx svk_ctx;
typedef struct svk_frontend_plan svk_frontend_plan;

/* ---- context, stream, memory --------------------------------------------- */
int svk_version(void);
int svk_create(int device_id, svk_ctx** out);
void svk_destroy(svk_ctx* ctx);
const char* svk_last_error(const svk_ctx* ctx);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream), NULL = null stream */
int svk_set_stream(svk_ctx* ctx, void* hip_stream);
int svk_sync(svk_ctx* ctx);
/* so that a host without torch can drive the library */
int svk_malloc(svk_ctx* ctx, size_t bytes, void** d_out);
int svk_free(svk_ctx* ctx, void* d_ptr);
int svk_memcpy_h2d(svk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int svk_memcpy_d2h(svk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int svk_memset(svk_ctx* ctx, void* d_dst, int value, size_t bytes);
/* device facts for roofline reporting: [0]=CU count, [1]=max clock kHz, [2]=LDS bytes/CU, [3]=wavefront size */
int svk_device_info(svk_ctx* ctx, int64_t out[4]);

/* ---- fused front end -------------------------------------------------------
 * PCM -> [pre-emphasis] -> frames -> rFFT power spectrum -> frame energy ->
 * mel filterbank (f32 MFMA) -> [log] -> [DCT-II (f32 MFMA)] -> [c0 := log E]
 * Replaces speechpy/feature.py:102-153 (mfcc), :156-219 (mfe), :222-258 (lmfe)
 * and, when preemph != 0, speechpy/processing.py:45-58 applied to the whole
 * clip first (circular, Q5).  Framing is the no-padding branch of
 * processing.py:112-120 (Q3) with a rectangular window (Q4).
 */
typedef enum svk_out_kind { SVK_OUT_MFE = 0, SVK_OUT_LMFE = 1, SVK_OUT_MFCC = 2 } svk_out_kind;
typedef enum svk_pcm_dtype { SVK_PCM_I16 = 0, SVK_PCM_F32 = 1 } svk_pcm_dtype;

typedef struct svk_frontend_cfg {
  int32_t frame_len;      /* samples per frame  = int(round(fs * frame_length))  */
  int32_t frame_stride;   /* samples per hop    = round(fs * frame_stride)       */
  int32_t nfft;           /* 512 or 1024 (fft_length)                            */
  int32_t num_filters;    /* 1..64                                               */
  int32_t num_ceps;       /* MFCC only: 1..num_filters                           */
  int32_t out_kind;       /* svk_out_kind                                        */
  int32_t dc_elimination; /* MFCC only: column 0 := log(frame energy) (Q8)       */
  int32_t preemph;        /* 0 = none, 1 = y[n] = x[n] - cof * x[(n-shift) mod N] */
  int32_t preemph_shift;
  float preemph_cof;
  float input_scale;      /* amplitude factor applied to the PCM first; 0 = 1.  2^-15 reads int16 PCM as
                             librosa.load hands it to lmfe (utils.py:170-173, load_data.py:50-70)          */
} svk_frontend_cfg;

/* h_filterbank: num_filters x (nfft/2+1) float64, row-major -- the matrix of
 * speechpy/feature.py:33-99, built on the host (its bin edges hinge on float64
 * libm rounding, Q1/Q2, so the host language that owns parity builds it).   */
int svk_frontend_plan_create(svk_ctx* ctx, const svk_frontend_cfg* cfg, const double* h_filterbank,
                             svk_frontend_plan** out);
void svk_frontend_plan_destroy(svk_frontend_plan* plan);
/* number of frames of a clip of n_samples: floor((n - frame_len) / stride), >= 0 (Q3) */
int64_t svk_frontend_num_frames(const svk_frontend_cfg* cfg, int64_t n_samples);
/* columns of the feature matrix: num_filters (MFE/LMFE) or num_ceps (MFCC) */
int svk_frontend_num_cols(const svk_frontend_cfg* cfg);

/* d_pcm      : concatenated clips, int16 or float32 (pcm_dtype); only the samples [offset, offset + length) of each clip are
 *              read (pre-emphasis is circular over the clip: the neighbour of its first sample is its last), never the gaps
 *              between clips or what lies behind the last one
 * d_offsets  : [n_utt] int64 first sample of each clip in d_pcm, or NULL = i * clip_stride; any offset is allowed (a clip
 *              that starts on a 16-byte boundary is staged with 16-byte loads, any other sample by sample: same bits)
 * d_lengths  : [n_utt] int32 samples per clip, or NULL = clip_len for all
 * max_frames : row stride of the outputs (>= frames of the longest clip)
 * d_feat     : [n_utt][max_frames][num_cols] float32; rows >= n_frames are zeroed
 * d_energy   : [n_utt][max_frames] float32 frame energies (after zero handling), rows >= n_frames are zeroed; or NULL
 * d_n_frames : [n_utt] int32 frames produced per clip, or NULL
 * d_src_chunk: NULL, or GATHERED input (int16 PCM): clip u's signal is then the concatenation of chunks of chunk_samples
 *              samples of its PCM, chunk q = PCM chunk d_src_chunk[u * chunk_stride + q], d_lengths[u] samples of it in
 *              all (required) -- svk_vad_energy's d_src_frame with chunk_samples = frame_samples: the voiced frames of
 *              vad.py:135-168 feed the front end where they lie, without the pass that copies them to the front of a
 *              second buffer (same samples, bit-identical features).  chunk_samples a multiple of 8.  Of a clip's row of the
 *              table only the first ceil(d_lengths[u] / chunk_samples) entries are read, and of its PCM only the chunks they name.
 */
int svk_frontend_run(svk_ctx* ctx, const svk_frontend_plan* plan, const void* d_pcm, int pcm_dtype,
                     const int64_t* d_offsets, const int32_t* d_lengths, int64_t clip_stride,
                     int32_t clip_len, int32_t n_utt, int32_t max_frames, float* d_feat, float* d_energy,
                     int32_t* d_n_frames, const int32_t* d_src_chunk, int32_t chunk_samples, int32_t chunk_stride);

/* ---- stage-level entry points (one speechpy function each) ----------------- */
/* processing.py:45-58.  d_in int16/float32 [n]; d_out float32 [n]; circular. */
int svk_preemphasis(svk_ctx* ctx, const void* d_in, int pcm_dtype, int64_t n, int32_t shift, float cof,
                    float* d_out);
/* processing.py:61-139.  frame t = d_sig[t*stride .. +frame_len) (zeros past n: nothing is read there) times d_window
 * (NULL = rectangular).  d_out float32 [n_frames][frame_len].                 */
int svk_stack_frames(svk_ctx* ctx, const float* d_sig, int64_t n, int32_t frame_len, int32_t stride,
                     int32_t n_frames, const float* d_window, float* d_out);
/* processing.py:142-174.  d_frames float32 [n_frames][frame_len] -> d_out
 * [n_frames][nfft/2+1]; power = 0: |rfft| (fft_spectrum), 1: |rfft|^2/nfft (power_spectrum).
 * Frames longer than nfft are cropped, shorter are zero-padded (Q6).  Any nfft >= 2. */
int svk_spectrum(svk_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_len, int32_t nfft,
                 int32_t power, float* d_out);
/* processing.py:239-271 per clip: d_feat [n_utt][max_frames][n_cols], rows < n_frames[u]
 * (NULL = max_frames) are normalised in place; variance != 0 divides by (std + 2^-30).  Rows >= n_frames[u] are neither
 * read nor written (nor read by svk_cmvn_stats, svk_delta_cmvn_stats, svk_cmvnw and svk_delta_planes: what they hold reaches
 * no statistic).
 * ONE CLIP, ONE RESULT (svk_cmvn, svk_cmvn_stats, svk_delta_cmvn_stats): a clip's statistics, and with them its normalised
 * rows, are a function of its rows and its n_frames[u] -- not of max_frames, n_utt or the clip's place in the batch, to the
 * last bit (tests/test_cmvn_route_invariance.py).  The launch is chosen by max_frames (above 1 024: chunks of 256 frames on
 * separate workgroups, otherwise one workgroup per clip), the ORDER of the float64 sums by the clip's own frame count: up to
 * 1 024 frames row group tr adds rows tr, tr + R, .. (R = 256 / min(n_cols, 256)) of the whole clip and the R partial sums
 * are added in order; above that the same inside each chunk, and the chunks are added in order.  Two exceptions, neither on
 * a path the pipeline takes: SVK_CMVN_SPLIT=0 / 1 in the environment (read at every call) forces a launch for tests, and 0
 * sums a clip of more than 1 024 frames in the one-workgroup order; with more than 65 535 clips in one call the chunked
 * launch does not fit the grid and every clip is summed in the one-workgroup order, so a clip of more than 1 024 frames
 * then differs from itself in a smaller call in the last bits of 1 / (std + 2^-30). */
int svk_cmvn(svk_ctx* ctx, float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
             const int32_t* d_n_frames, int32_t variance);
/* The same statistics WITHOUT applying them: d_stats float64 [n_utt][2][n_cols], [u][0][c] = mean, [u][1][c] =
 * 1 / (std + 2^-30) (1 when variance == 0) over rows < n_frames[u]; clips with no rows are left untouched.  utils.py:382-397
 * (CMVN) feeds utils.py:351-379 (FeatureCube), which reads 20 x 80 rows of a clip: svk_cube_gather_cmvn below applies the
 * normalisation to just those rows on the way, instead of a pass over every row of a 145 s clip.  The statistics are
 * svk_cmvn's own, bit for bit, and depend on the clip alone (ONE CLIP, ONE RESULT above). */
int svk_cmvn_stats(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                   const int32_t* d_n_frames, int32_t variance, double* d_stats);

/* feature.py:202-217 and :146-153 on a power spectrum that is already on the device -- the general
 * (any fft_length, up to 1024 filters) counterpart of the fused front end, one workgroup per frame:
 * energy = sum of all bins (0 -> eps), mel = power x bank^T (0 -> eps), then by out_kind nothing /
 * log / log + DCT-II ortho (+ c0 := log energy).  d_bank [num_filters][n_bins] float32.
 * d_feat [n_frames][cols], cols = num_filters or num_ceps; d_energy [n_frames] or NULL. */
int svk_mel_features(svk_ctx* ctx, const float* d_power, int32_t n_frames, int32_t n_bins, const float* d_bank,
                     int32_t num_filters, int32_t out_kind, int32_t num_ceps, int32_t dc_elimination,
                     float* d_feat, float* d_energy);
/* processing.py:274-327 (cmvnw, Q10) per clip: sliding window of `win` (odd) rows, 'symmetric'
 * padding of (win-1)/2 rows; out = x - window mean; with variance != 0 a second pass divides by
 * (population std of the window over the MEAN-SUBTRACTED rows, padded the same way, + 2^-30).
 * d_in / d_out / d_tmp: [n_utt][max_frames][n_cols] float32, all distinct; d_tmp is a workspace, only needed
 * (and only written, in rows < n_frames[u] at most) when variance != 0: with variance == 0 it may be NULL and is left
 * untouched.  Rows >= n_frames[u] are left untouched in d_out.  The kernel is chosen by max_frames (up to 3 900: prefix sums,
 * above: a sliding sum), so a clip's result may depend on the launch in the last bits; svk_cmvnw is not on the embedding path. */
int svk_cmvnw(svk_ctx* ctx, const float* d_in, int32_t n_utt, int32_t max_frames, int32_t n_cols,
              const int32_t* d_n_frames, int32_t win, int32_t variance, float* d_tmp, float* d_out);
/* processing.py:201-236 (derivative_extraction) exactly as the reference computes it, Q11 included:
 * out[r][c] = sum_{k=1..delta} k * in[r][min(c + k, n_cols - 1)] / sum_{k} 2 k^2  (edge padding along
 * the FEATURE axis; the subtraction on processing.py:232 is a detached statement). */
int svk_derivative(svk_ctx* ctx, const float* d_in, int64_t n_rows, int32_t n_cols, int32_t delta, float* d_out);
/* processing.py:177-198 (log_power_spectrum) on a power spectrum already on the device: in place
 * p <- 10 log10(max(p, 1e-20)); normalize != 0 then subtracts the global maximum. */
int svk_log_power(svk_ctx* ctx, float* d_power, int64_t n, int32_t normalize);

/* ---- energy VAD ------------------------------------------------------------
 * vad.py:44-57 (framer, Q12) + vad.py:60-129 (ring-buffer hysteresis, Q13) with
 * the per-frame decision  sum(x^2) > threshold * frame_samples  (int64) in place of
 * webrtcvad (vad.py:90).  ring_len = int(padding_ms / frame_ms); ring_thresh =
 * floor(0.9 * ring_len) (trigger when voiced > ring_thresh, release when unvoiced >
 * ring_thresh).
 * A clip of L samples has (2 L - 1) / (2 frame_samples) whole frames (vad.py:54); the samples of the partial frame behind
 * them are not read.
 * d_keep       : [n_utt][max_vad_frames] uint8, 1 = frame is in some yielded segment; 0 from the clip's frame count on
 * d_seg        : [n_utt][max_vad_frames] int32 segment ordinal or -1 (also from the clip's frame count on), or NULL
 * d_n_vad_frames: [n_utt] int32, or NULL
 * d_voiced     : int16, same offsets as d_pcm: kept frames packed to the front (the rest of a
 *                clip's slot is left untouched), or NULL
 * d_voiced_len : [n_utt] int32 samples kept (required when d_voiced or d_src_frame != NULL)
 * d_src_frame  : [n_utt][max_vad_frames] int32 or NULL: the index form of the same compaction, d_src_frame[u][q] = the
 *                frame that is the q-th kept one (entries past the kept count are left untouched); svk_frontend_run reads
 *                the PCM through it (d_src_chunk) -- with d_voiced = NULL nothing is copied
 */
int svk_vad_energy(svk_ctx* ctx, const int16_t* d_pcm, const int64_t* d_offsets, const int32_t* d_lengths,
                   int64_t clip_stride, int32_t clip_len, int32_t n_utt, int32_t frame_samples,
                   int32_t ring_len, int32_t ring_thresh, int64_t threshold, int32_t max_vad_frames,
                   uint8_t* d_keep, int32_t* d_seg, int32_t* d_n_vad_frames, int16_t* d_voiced,
                   int32_t* d_voiced_len, int32_t* d_src_frame);

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

/* ---- feature cube ------------------------------------------------------------
 * utils.py:351-379 (FeatureCube): out[u][0][c][r][:] = feat[u][crop[u][c] + r][:].
 * d_out float32 [n_utt][1][n_crops][crop_frames][n_cols] (a torch tensor's data_ptr()).  A negative start or one at / past
 * max_frames gives a zero crop, a crop that runs past max_frames zero rows from there; rows of d_feat that no crop covers
 * are not read (the same for svk_cube_gather_cmvn and svk_cube_gather_delta). */
int svk_cube_gather(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                    const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, float* d_out);
/* utils.py:382-397 + :351-379 in one pass: the cube of svk_cmvn-normalised features from the RAW features and svk_cmvn_stats'
 * d_stats: out = (float)(((double)feat - mean[c]) * inv[c]), the expression svk_cmvn applies (bit-identical to svk_cmvn followed
 * by svk_cube_gather); too-short clips (crop -1) give zero cubes as there. */
int svk_cube_gather_cmvn(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                         const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const double* d_stats,
                         float* d_out);

/* ---- the three-channel input (constants.DERIVATIVE: static, delta, delta-delta) from STATIC features ------------
 * feature.py:261-282 (extract_derivative_feature) stacks the static features with processing.py:201-236 applied once and
 * twice; utils.py:382-397 (CMVN) then normalises each channel by itself (processing.py:239-271) and utils.py:325-348
 * (FeatureCube3C) crops all three.  The reference's derivative runs along the FEATURE axis (Q11, reproduced by
 * svk_derivative), so the three channels of a frame depend on that frame's static row alone: the entries below form the
 * delta values where they are needed instead of writing, re-reading and stacking delta planes.  Every delta value is
 * svk_derivative's (f32, the same expression and order, edge clamp min(c + k, n_cols - 1)); delta-delta is taken from the
 * F32 delta values.  `delta` >= 1 is both steps' window (the reference uses 2).  max_frames * n_cols must stay below 2^31.
 *
 * d_stats float64 [n_utt][3][2][n_cols]: for channel ch (0 static, 1 delta, 2 delta-delta)
 * [u][ch][0][c] = mean, [u][ch][1][c] = 1 / (std + 2^-30) (1 when variance == 0) over rows < n_frames[u]; clips with no
 * rows are left untouched.  ONE pass over d_feat [n_utt][max_frames][n_cols]; bit-identical to svk_cmvn_stats on plane ch
 * of svk_delta_planes (the same launch paths, SVK_CMVN_SPLIT included, the same summation order), and like them a function
 * of the clip's rows and n_frames[u] alone, whatever max_frames, n_utt and the clip's place (ONE CLIP, ONE RESULT at svk_cmvn). */
int svk_delta_cmvn_stats(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                         const int32_t* d_n_frames, int32_t delta, int32_t variance, double* d_stats);
/* d_out [n_utt][3][max_frames][n_cols] (svk_c3d2_stage1_c3's d_feat layout): plane 0 = d_feat, 1 = derivative(d_feat),
 * 2 = derivative(plane 1); with d_stats != NULL each value is (float)(((double)v - mean) * inv), svk_cmvn's expression.
 * Rows >= n_frames[u] (NULL = max_frames) are written as zeros in all three planes.  d_out must not alias d_feat. */
int svk_delta_planes(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                     const int32_t* d_n_frames, int32_t delta, const double* d_stats, float* d_out);
/* FeatureCube3C (utils.py:325-348) from STATIC features: d_out [n_utt][3][n_crops][crop_frames][n_cols],
 * out[u][ch][k][r][:] = channel ch of row crop[u][k] + r, normalised when d_stats != NULL; crop -1 / rows outside the
 * clip's max_frames rows -> zeros, as svk_cube_gather / svk_cube_gather_cmvn (like those, it does not know n_frames: crop
 * starts are expected to keep their rows below it, as svk_cube_draw_crops' do). */
int svk_cube_gather_delta(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                          const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, int32_t delta,
                          const double* d_stats, float* d_out);

/* Crop starts drawn ON THE DEVICE (no host round trip for the per-clip frame count):
 * crop[u][c] = floor(uniform(seed, u, c) * (n_frames[u] - crop_frames)), a counter-based
 * generator (splitmix64 of seed, g, c) with g = d_utt_index[u] when that array is given (clips of a
 * ragged corpus land in batches in any order) and first_utt + u otherwise, so a draw depends only on
 * the clip's global index.  utils.py:372 draws `np.random.randint(T - 80, size=20)` from the process-global
 * NumPy RNG instead; hosts that need that exact sequence pass their own d_crop_idx to
 * svk_cube_gather.  Clips with n_frames <= crop_frames get -1 (svk_cube_gather then emits zeros)
 * and are counted in *d_bad_count (int32, may be NULL; the caller zeroes it).
 * Several cubes per clip (svk_c3d2_stage1_multi) need nothing new here: n_crops = 20 K yields d_crop_idx [n_utt][K][20], still
 * keyed by (seed, clip, c), and its first 20 starts per clip are the one-cube draw.               */
int svk_cube_draw_crops(svk_ctx* ctx, const int32_t* d_n_frames, int32_t n_utt, int64_t first_utt,
                        const int64_t* d_utt_index, int32_t n_crops, int32_t crop_frames, uint64_t seed,
                        int32_t* d_crop_idx, int32_t* d_bad_count);

/* ---- audio ingest ----------------------------------------------------------
 * utils.py:170-173  `librosa.load(path, sr=16000, mono=True)`: down-mix (mean over
 * channels), scale int16 / 32768 and resample, for n_utt clips in one launch.
 * librosa is absent and its resampler unpinned, so the arithmetic is the published
 * polyphase windowed-sinc scheme of scipy.signal.resample_poly (zero-padded edges):
 *     y[m] = sum_j x[j] * taps[m * down + half - j * up],   half = (n_taps - 1) / 2
 * d_pcm    : [n_utt][in_stride][n_ch] interleaved int16 frames (vad.py:10-22 reads them)
 * d_in_len : [n_utt] int32 frames per clip, or NULL = clip_in; frames at or past a clip's count and the padding of in_stride
 *            are not read, the padding of out_stride is not written
 * d_taps   : [n_taps] float32 (odd count; the host builds them, see ingest.py)
 * d_out    : [n_utt][out_stride] float32 in [-1, 1) (SVK_PCM_F32) or int16 rounded back to the
 *            16-bit grid, saturating (SVK_PCM_I16); samples past a clip's end are written as 0
 * d_out_len: [n_utt] int32 = min(ceil(n_in * up / down), clip_out), or NULL; written for every
 *            clip also when clip_out == 0 (a batch without frames: all zero, nothing else is touched) */
int svk_ingest_resample(svk_ctx* ctx, const int16_t* d_pcm, int32_t n_ch, int64_t in_stride,
                        const int32_t* d_in_len, int32_t clip_in, int32_t n_utt, const float* d_taps,
                        int32_t n_taps, int32_t up, int32_t down, void* d_out, int32_t out_dtype,
                        int64_t out_stride, int32_t clip_out, int32_t* d_out_len);

/* ---- scoring ---------------------------------------------------------------
 * evaluation.py:67-84: cosine of every test row against every enrolled row,
 * float32, out [n_test][n_enroll]  (f32 MFMA).  dim <= 4096.
 * Accuracy: f32 products and f32 accumulation in a K order fixed by dim; every score lies within 1e-5 of the float64
 * cosine of the same float32 rows, on every kernel the call may pick (one wave per 16 test rows below 2^22 pairs or 64
 * enrolled rows, the tiled kernel above, either register budget), with 16-byte or -- dim % 4 != 0, or a matrix that is only
 * 4-byte aligned -- 4-byte loads (tests/test_scoring_float64.py; DESIGN.md 3.4 has the measured errors).  A zero norm
 * divides by 1 (sklearn's normalize): a zero row scores exactly 0 against everything, never NaN.  A NaN or Inf in a row
 * makes that row's scores NaN -- an infinite norm too: inf / inf and x * (1 / inf) with x = +-inf are NaN -- and stays
 * there: every other score has the bits it has without it.  Within one shape the bits of a score depend on its two rows
 * alone, not on their positions, and runs are bit-identical.
 * 1 <= dim <= 4096: dim > 4096 is SVK_ERR_UNSUPPORTED, dim < 1 or a negative count SVK_ERR_BAD_ARG; n_test == 0 or
 * n_enroll == 0 writes nothing, launches nothing and looks at no pointer.                                      */
int svk_cosine_scores(svk_ctx* ctx, const float* d_test, const float* d_enroll, int32_t n_test,
                      int32_t n_enroll, int32_t dim, float* d_out);
/* siamese.py:29-30: out[i] = || a[i] - b[i] ||_2, one wave per row, f32.
 * Accuracy: |out[i] - d| <= (dim / 2 + 3) 2^-24 d against the float64 distance d of the same float32 rows (one rounding in
 * a - b, a sum of dim non-negative squares in any order, a square root); equal rows give exactly 0.
 * dim == 0 is allowed: the rows are empty, out[i] = 0 for all n rows, and d_a, d_b are not looked at (they may be NULL, as
 * the pointer of an empty matrix is); d_out must not be NULL.  n == 0 launches nothing.  Negative n or dim:
 * SVK_ERR_BAD_ARG.                                                                                             */
int svk_l2_dist(svk_ctx* ctx, const float* d_a, const float* d_b, int32_t n, int32_t dim, float* d_out);

/* The mean over groups of embedding rows (csrc/pool.hip): the K cubes of a clip -> the clip's embedding, and the utterances of
 * a speaker -> the speaker's model (the mean the d-vector method describes; the reference itself keeps a speaker's LAST
 * utterance, model.py:374-388, Q17 -- pipeline.enroll_last_utterance).
 *   d_emb         [n_rows][dim] f32, 4-byte aligned (16-byte loads when dim % 4 == 0 and d_emb, d_out are 16-byte aligned: same bits)
 *   segments      d_seg_start == NULL: uniform, segment s = rows [s * rows_per_seg, (s + 1) * rows_per_seg), rows_per_seg >= 1,
 *                 n_seg * rows_per_seg <= n_rows;  else d_seg_start int64 [n_seg + 1], CSR offsets (rows_per_seg is ignored):
 *                 segment s = rows [start[s], start[s + 1]), non-decreasing and within [0, n_rows] -- the caller's duty, as for
 *                 the crop starts; offsets outside that are clamped, never followed
 *   d_row_index   NULL, or int64 [n_rows]: segment s's rows are d_emb[d_row_index[i]] for i in its range (either form) -- a
 *                 speaker's utterances lie anywhere in d_emb.  An index outside [0, n_rows) is the caller's error: it is not
 *                 read, and its segment comes out NaN
 *   flags         bit 0 (1): every row enters as x / ||x||, a row of norm zero as zeros;  bit 1 (2): the mean leaves divided
 *                 by its own norm, a zero mean stays zero;  every other bit must be 0
 *   d_out         [n_seg][dim] f32 = (float)(sum / count);  an EMPTY segment writes zeros and adds 1 to *d_empty_count (int32,
 *                 may be NULL; the caller zeroes it)
 * Sums, norms and divisions are float64; NaN propagates to its own segment and no other.  The order of additions in a segment
 * depends on that segment's length alone (rows in order inside blocks of 64 rows, the blocks' partial sums in order), not on
 * n_seg, the launch geometry or the other segments: runs are bit-identical, and a segment pooled alone gives the bits it gives
 * inside a batch.  One team of threads per segment, eight segments of dim 128 per workgroup: many short segments are the
 * case it is laid out for.  1 <= dim <= 4096; n_seg == 0 launches nothing.  SVK_ERR_BAD_ARG: NULL context or buffer, negative
 * size, dim outside [1, 4096], rows_per_seg < 1 or n_seg * rows_per_seg > n_rows (uniform form), misalignment, undefined flag bits. */
int svk_embedding_pool(svk_ctx* ctx, const float* d_emb, int64_t n_rows, int32_t dim, int64_t n_seg, int32_t rows_per_seg,
                       const int64_t* d_seg_start, const int64_t* d_row_index, int32_t flags, float* d_out,
                       int32_t* d_empty_count);

/* ---- embedding back end (csrc/backend.hip) ---------------------------------
 * The statistics a back end (centring, LDA, WCCN, whitening: backend.py) is fitted on: the float64 mean of every class and the
 * within-class scatter  S_w = sum_c sum_{i in c} (x_i - m_c)(x_i - m_c)^T  of labelled embedding rows.
 *   d_emb         [n_rows][dim] f32, 4-byte aligned
 *   segments      d_seg_start int64 [n_class + 1] and d_row_index (NULL or int64 [n_rows]) mean what they mean in
 *                 svk_embedding_pool: class c is rows d_row_index[start[c] : start[c + 1]]; offsets are clamped, never followed;
 *                 a row index outside [0, n_rows) is not read and makes its class NaN (its mean, and through it d_sw, unless
 *                 the class has fewer than two rows); rows outside every class are ignored
 *   flags         bit 0 (1): every row enters as x / ||x|| with a float64 norm, a zero row as zeros; every other bit must be 0
 *   d_class_mean  float64 [n_class][dim]: the mean of the class, rows added in order inside blocks of 64 rows and the blocks'
 *                 sums in order; an empty class gives zeros.  A class's mean has the bits it has when it is the only class
 *   d_sw          float64 [dim][dim], computed from the CENTRED rows (two-pass, not sum x x^T - n m m^T) on
 *                 v_mfma_f64_16x16x4_f64 with the rows as K.  A class of one row contributes exactly zero: classes of fewer
 *                 than two rows are left out, and their presence changes no bit of d_sw
 *   d_workspace   svk_class_scatter_workspace_bytes(n_rows, dim, n_class) bytes, 16-byte aligned (the row norms, the prefix sums
 *                 of the class sizes and the partial matrices); 0 for arguments the call rejects and for n_class == 0
 * Determinism: no floating-point atomics.  The rows of the classes with two or more rows, in class order, are cut into chunks
 * whose length depends on dim alone; each chunk's partial matrix is an MFMA chain in row order and the partial matrices are
 * added in chunk order.  The bits depend on the rows, the segments, dim and flags alone -- not on the launch geometry, a
 * counter or timing: runs are bit-identical, and d_sw[a][b] == d_sw[b][a] bit for bit (only the upper triangle is computed).
 * NaN: a NaN at column a of one row makes that class's mean NaN at column a, and row a and column a of d_sw (flag bit 0 set:
 * the row's norm is NaN and so is the whole row).  1 <= dim <= 512; n_class == 0 writes a zero d_sw and launches nothing else.
 * The global mean, S_b and S_t = S_w + S_b are n_class x dim numbers: the host forms them (backend.solve).  Asynchronous on the
 * context's stream.  SVK_ERR_BAD_ARG: NULL context or buffer, negative size, dim outside [1, 512], undefined flag bits,
 * misalignment (f32: 4 bytes; int64 / float64: 8; workspace: 16), a short workspace. */
size_t svk_class_scatter_workspace_bytes(int64_t n_rows, int32_t dim, int64_t n_class);
int svk_class_scatter(svk_ctx* ctx, const float* d_emb, int64_t n_rows, int32_t dim, const int64_t* d_seg_start,
                      const int64_t* d_row_index, int64_t n_class, int32_t flags, void* d_workspace, size_t workspace_bytes,
                      double* d_class_mean, double* d_sw);

/* The per-embedding half of the back end, one trip through HBM:  y = l2( (l2(x) - mu) W ).  ONE arithmetic for every shape:
 *   flags bit 0 (1)   x' = (float)(x / ||x||): the sum of squares, the square root and the division in float64, rounded once; a
 *                     zero row gives zeros.  Clear: x' = x
 *   c = x' - mu       in f32; d_mean NULL (mu = 0) or f32 [dim]
 *   y_j = sum_k c_k W_kj   f32 products, f32 accumulation on v_mfma_f32_16x16x4_f32; d_w f32 [dim][out_dim] row-major.  The order
 *                     of k is fixed by dim: super-steps of 16, inside one the k = 16 S + 4 g + e in the order (e, g)
 *   flags bit 1 (2)   y / ||y||: the sum of squares of the f32 y, the square root and the division in float64, rounded once; a
 *                     zero y stays zero.  The y that is normalised has the bits the call gives with the bit clear
 *   d_w NULL          the identity: out_dim must equal dim, y = c exactly, no matrix pipe
 *   d_out             f32 [n_rows][out_dim]; must not be d_emb
 * A wave owns 16 rows and all their output tiles; W is staged through LDS sixteen k at a time.  Loads of x and mu are 16-byte
 * when dim % 4 == 0 and both are 16-byte aligned, 4-byte otherwise: the same bits either way.  The bits of a row's output
 * depend on that row, mu, W, dim, out_dim and flags alone -- not on n_rows, the row's position or the geometry; NaN stays in
 * its own row.  1 <= out_dim <= dim <= 512; n_rows == 0 launches nothing.  SVK_ERR_BAD_ARG: NULL context or buffer, negative
 * size, dims out of range, NULL d_w with out_dim != dim, undefined flag bits, misalignment, d_out == d_emb. */
int svk_embedding_project(svk_ctx* ctx, const float* d_emb, int64_t n_rows, int32_t dim, const float* d_mean, const float* d_w,
                          int32_t out_dim, int32_t flags, float* d_out);

/* One score per TRIAL of a list (the `label utterance_a utterance_b` lines of the VoxCeleb1 protocols) instead of the whole
 * matrix of svk_cosine_scores or the row-i-against-row-i of svk_l2_dist; replaces the a[idx_a], b[idx_b] gathers and the
 * reduction a framework would do:  d_out[p] = score(d_a[d_idx_a[p]], d_b[d_idx_b[p]]).
 *   metric 0      cosine, x.y / (||x|| ||y||); a zero norm divides by 1 (svk_cosine_scores, sklearn's normalize)
 *   metric 1      -||x - y||_2: siamese.py:29-30 negated, so that a larger score means the same speaker (what the ROC expects)
 *   d_a, d_b      [n_a][dim], [n_b][dim] f32, 4-byte aligned; d_a == d_b is allowed.  16-byte loads when dim % 4 == 0 and both
 *                 are 16-byte aligned, 4-byte loads otherwise: the same bits either way
 *   d_idx_a/_b    int64 [n_pairs].  An index outside its matrix is the caller's error: the rows are not read, that trial's score
 *                 is NaN and *d_bad_count (int32, may be NULL, the caller zeroes it) goes up by one
 * The products, the sums, the square roots and the division are float64 and the result is rounded to float32 once: it lies
 * within 1 float32 ulp of the correctly rounded exact score.  The order of additions of a trial depends on dim alone (a team of
 * 16 lanes per trial, each lane its columns in order, then a butterfly), not on n_pairs, the launch geometry or the
 * neighbouring trials: a trial scored alone gives the bits it gives inside a list.  1 <= dim <= 4096; n_pairs == 0 launches
 * nothing.  SVK_ERR_BAD_ARG: NULL context or buffer, negative size, dim out of range, unknown metric, misalignment. */
int svk_pair_scores(svk_ctx* ctx, const float* d_a, int64_t n_a, const float* d_b, int64_t n_b, int32_t dim,
                    const int64_t* d_idx_a, const int64_t* d_idx_b, int64_t n_pairs, int32_t metric, float* d_out,
                    int32_t* d_bad_count);

/* ---- PLDA scoring (csrc/plda.hip) ------------------------------------------------------------
 * Log-likelihood ratios under the two-covariance PLDA model in the basis that diagonalises both covariances (plda.py fits it
 * from svk_class_scatter's statistics): a projected utterance is u = y + e with y ~ N(0, diag psi) for the speaker and
 * e ~ N(0, I) for the session.  An enrolled model is the mean u of n >= 1 projected utterances, a test utterance is v:
 *   llr(u, n, v) = sum_k [ alpha_k(n) u_k v_k - 1/2 beta_k(n) v_k^2 - 1/2 gamma_k(n) u_k^2 ] + c(n)
 *   alpha_k(n) = n psi_k / d1,  beta_k(n) = n psi_k^2 / (d1 d3),  gamma_k(n) = n^2 psi_k^2 / (d1 d2)
 *   d1 = (n + 1) psi_k + 1,  d2 = n psi_k + 1,  d3 = psi_k + 1
 *   c(n) = -1/2 sum_k log(d1 / (d2 d3)), each logarithm formed as log1p(-n psi_k^2 / (d2 d3))
 * A direction with psi_k = 0 contributes exactly 0.  d_psi: float64 [dim], finite and >= 0 (the caller's duty: anything else
 * gives NaN or nonsense in the scores, never a fault).  Both entries take PROJECTED rows [.][dim] f32, 1 <= dim <= 512 (the
 * back end's limit), and are asynchronous on the context's stream.
 *
 * svk_plda_scores: d_out[i][j] = llr(d_enroll[j], n_j, d_test[i]), f32 [n_test][n_enroll]; n_j = d_enroll_count[j] (int32), or 1
 * for every j when d_enroll_count is NULL.  A float64 pre-pass, then ONE product kernel on v_mfma_f32_16x16x4_f32:
 *   pre-pass      enrolled row j:  b_jk = f32(alpha_k(n_j) u_jk),  t_j = -1/2 sum_k gamma_k(n_j) u_jk^2 + c(n_j) kept as float64
 *                 counts NULL:   test row i:  s_i = -1/2 sum_k beta_k(1) v_ik^2 kept as float64;  a_ik = v_ik;  K = dim
 *                 counts given:  a_i,dim+k = f32(v_ik^2),  b_j,dim+k = f32(-1/2 beta_k(n_j)),  s_i = 0;  K = 2 dim
 *                 (float64 products, divisions and sums; lane l of a wave adds the columns l, l + 64, ... in order, then a butterfly)
 *   product       dot_ij = sum_k a_ik b_jk: f32 products, f32 accumulation, the order of k fixed by dim and the form (128-column
 *                 blocks in order, the second half after the first; inside a block super-steps of 16, inside one the
 *                 k = 16 S + 4 g + e in the order (e, g)).  The enrolled operand is staged through LDS 32 rows at a time; the
 *                 split is over output rows and columns, never over K
 *   epilogue      d_out[i][j] = f32(((double) dot_ij + s_i) + t_j), rounded once
 *   accuracy      with a, b the float64 values of the operands before their rounding and ref the float64 score,
 *                 |d_out - ref| <= (K + 4) 2^-24 sum_k |a_k b_k| + 2^-24 |ref|  (tests/test_plda_scores.py derives it)
 * Within a form (counts NULL / given) the bits of a score depend on its two rows, psi, the row's count and dim alone -- not on
 * n_test, n_enroll, the rows' positions or the launch geometry; runs are bit-identical.  The same bits with 16-byte loads
 * (dim % 4 == 0 and a 16-byte aligned d_test) and 4-byte loads.  A NaN or Inf in a test row stays in that row of d_out, one in
 * an enrolled row in that column; a count < 1 makes its column NaN.
 *   d_workspace   svk_plda_scores_workspace_bytes(n_test, n_enroll, dim, with_counts) bytes, 16-byte aligned (t, s, the enrolled
 *                 operand and, with counts, both second halves); with_counts: non-zero when d_enroll_count is given.  0 for
 *                 arguments the call rejects and for n_test == 0 or n_enroll == 0, which need none
 * n_test == 0 or n_enroll == 0 writes nothing, launches nothing and looks at no pointer.  SVK_ERR_BAD_ARG: NULL context or
 * buffer, negative size, dim outside [1, 512], misalignment (f32 / int32: 4 bytes; float64: 8; workspace: 16), a short workspace. */
size_t svk_plda_scores_workspace_bytes(int32_t n_test, int32_t n_enroll, int32_t dim, int32_t with_counts);
int svk_plda_scores(svk_ctx* ctx, const float* d_test, int32_t n_test, const float* d_enroll, int32_t n_enroll, int32_t dim,
                    const double* d_psi, const int32_t* d_enroll_count, void* d_workspace, size_t workspace_bytes,
                    float* d_out);

/* One LLR per TRIAL of a list, as svk_pair_scores gives one cosine:  d_out[p] = llr(d_b[d_idx_b[p]], n, d_a[d_idx_a[p]]) with
 * n = d_count_b[d_idx_b[p]] (int32 [n_b]), or 1 when d_count_b is NULL.  d_a is the TEST side, d_b the ENROLLED side; d_a == d_b
 * is allowed.
 *   d_a, d_b      [n_a][dim], [n_b][dim] f32 projected rows, 4-byte aligned.  16-byte loads when dim % 4 == 0 and both are
 *                 16-byte aligned, 4-byte loads otherwise: the same bits either way
 *   d_idx_a/_b    int64 [n_pairs].  An index outside its matrix is the caller's error: the rows are not read, that trial's score
 *                 is NaN and *d_bad_count (int32, may be NULL, the caller zeroes it) goes up by one.  A count < 1 gives NaN too
 *                 (and is not counted)
 * Every coefficient, product, division, logarithm and sum is float64 and the result is rounded to float32 once:
 * |d_out - ref| <= 2^-24 |ref| + (dim + 8) 2^-52 sum |terms| against a float64 evaluation of the formula above, the terms being
 * its 6 dim summands (tests/test_plda_pair_scores.py).  The order of additions of a trial depends on dim alone (a team of 16
 * lanes per trial, each lane its columns in order, then a butterfly), not on n_pairs, the launch geometry or the neighbouring
 * trials: a trial scored alone gives the bits it gives inside a list.  n_pairs == 0 launches nothing.  SVK_ERR_BAD_ARG: NULL
 * context or buffer, negative size, dim outside [1, 512], misalignment. */
int svk_plda_pair_scores(svk_ctx* ctx, const float* d_a, int64_t n_a, const float* d_b, int64_t n_b, int32_t dim,
                         const double* d_psi, const int32_t* d_count_b, const int64_t* d_idx_a, const int64_t* d_idx_b,
                         int64_t n_pairs, float* d_out, int32_t* d_bad_count);

/* Speaker SEARCH: the k best rows of a gallery for every query row by cosine score, without the [n_query][n_gallery] matrix
 * that svk_cosine_scores writes and svk_top1 / a framework's top-k reads back (148 642 x 1 211: 720 MB each way; a corpus
 * against itself or against 10^6 enrolled speakers: more than the card holds).  The product runs as in svk_cosine_scores'
 * tiled kernel; each wave keeps a sorted list of k entries per query row on chip, and a second kernel merges the lists of
 * the gallery spans.
 *   d_query, d_gallery   [n_query][dim], [n_gallery][dim] f32, 4-byte aligned.  16-byte loads when dim % 4 == 0 and both are
 *                 16-byte aligned, 4-byte loads otherwise: the same bits either way
 *   d_top_score   f32 [n_query][k], d_top_index int64 [n_query][k]: the k best gallery rows of query q, best first.  An index is
 *                 index_base + j for row j of THIS call's d_gallery (index_base >= 0); slots beyond the number of candidates
 *                 hold index -1 and score -inf
 *   order         ONE strict total order, in the selection, in the merge and in accumulation: the higher score first; a NaN
 *                 score above every number (as svk_top1 and svk_c3d2_head put it); among equal scores (-0 == +0, all NaNs
 *                 equal) the lower index first.  The order being total, the result does not depend on how the work was split
 *   flags         bit 0 (1), accumulate: on entry the outputs hold lists of that form from earlier calls (sorted, -1 / -inf in
 *                 the empty slots); the result is the k best of that list and this call's gallery together.  With index_base
 *                 this searches a gallery that is streamed in chunks or larger than device memory with one set of lists: the
 *                 result equals ONE call over the concatenated gallery bit for bit, for any chunking with disjoint index
 *                 ranges, presented in any order.  Every other bit must be 0
 *   d_exclude     NULL, or int64 [n_query]: the gallery row whose global index (index_base + j) equals d_exclude[q] is not a
 *                 candidate for query q -- a self-search, where query q is row q of the gallery.  A value outside this call's
 *                 range excludes nothing
 *   d_workspace   svk_cosine_topk_workspace_bytes(n_query, n_gallery, dim, k) bytes, 16-byte aligned (the 1 / norms of both
 *                 matrices and the partial lists, 8 k bytes per query and gallery span); the size depends on the shape alone
 *                 and is 0 for arguments the call rejects (and for n_query == 0 or n_gallery == 0, which need none)
 * The score is what svk_cosine_scores' tiled path computes: f32 products and f32 accumulation on v_mfma_f32_16x16x4_f32 in
 * a K order fixed by dim, times 1 / ||q|| and 1 / ||g||, each formed in f32 by a pre-pass over its matrix; a zero norm divides
 * by 1, so a zero row scores 0.  There is ONE arithmetic for every shape: the bits of a score depend on the two rows and dim
 * alone, not on n_query, n_gallery, the row's position, the launch geometry, the chunking or k; runs are bit-identical.
 * 1 <= dim <= 4096, 1 <= k <= 32.  n_query == 0 launches nothing; n_gallery == 0 leaves the lists as they are with the
 * accumulate flag and fills them with -1 / -inf without it.  SVK_ERR_BAD_ARG: NULL context or buffer, negative size, dim or k
 * out of range, undefined flag bits, a negative index_base, misalignment, a workspace below the size above.  Asynchronous on
 * the context's stream: no host round trip. */
size_t svk_cosine_topk_workspace_bytes(int32_t n_query, int32_t n_gallery, int32_t dim, int32_t k);
int svk_cosine_topk(svk_ctx* ctx, const float* d_query, int32_t n_query, const float* d_gallery, int32_t n_gallery,
                    int32_t dim, int32_t k, int64_t index_base, const int64_t* d_exclude, int32_t flags,
                    void* d_workspace, size_t workspace_bytes, float* d_top_score, int64_t* d_top_index);

/* ---- top-k search on normalised scores -------------------------------------------
 * svk_cosine_topk_norm is svk_cosine_topk (above) in every respect except that it selects, merges and accumulates NORMALISED
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

/* ---- speaker diarization (csrc/cluster.hip) ---------------------------------------------------
 * "Who spoke when" in recordings with several speakers: sliding windows over a recording's feature rows, one embedding per
 * window (svk_c3d2_stage1_multi with K = max_windows), the cosine of every pair of windows of a recording, and agglomerative
 * clustering of each recording's windows.  All three entries are asynchronous on the context's stream, make no host round trip,
 * use no floating-point atomics and let no workgroup wait for another; every device loop has a trip count fixed by its
 * arguments.  PADDED layout throughout: recording r owns slot r of every array, and d_n_seg[r] (d_n_windows[r]) of its
 * seg_stride (max_windows) rows are live.  n_rec == 0 launches nothing and looks at no pointer.
 *
 * svk_window_crops: per-recording frame counts -> the crop table svk_c3d2_stage1_multi takes.  Integer arithmetic only.  For a
 * recording of T = d_n_frames[r] frames (a negative count reads as 0):
 *   windows       T < crop_frames: none;  T < win_frames: one window [0, T);  else windows of win_frames frames starting at
 *                 w * hop_frames for w = 0 .. (T - win_frames) / hop_frames, and, when (T - win_frames) % hop_frames != 0, a last
 *                 window [T - win_frames, T)
 *   crops         crop c of a window [w0, w0 + len) starts at w0 + (c * (len - crop_frames)) / max(n_crops - 1, 1)
 *   d_crop_idx    int32 [n_rec][max_windows][n_crops]; -1 in unused windows (the first block reads zero rows there)
 *   d_n_windows   int32 [n_rec]: windows written, at most max_windows
 *   d_window_span NULL, or int32 [n_rec][max_windows][2]: (first frame, length) of every window, (-1, 0) in unused ones
 *   d_bad_count   a recording that needs more than max_windows windows keeps its first max_windows and adds 1 to *d_bad_count
 *                 (int32, may be NULL; the caller zeroes it)
 * SVK_ERR_BAD_ARG: NULL context or buffer, negative size, crop_frames < 1, win_frames < crop_frames, hop_frames < 1,
 * n_crops < 1, max_windows < 1, max_windows * n_crops or n_crops * win_frames at or above 2^31, misalignment. */
int svk_window_crops(svk_ctx* ctx, const int32_t* d_n_frames, int32_t n_rec, int32_t win_frames, int32_t hop_frames,
                     int32_t crop_frames, int32_t n_crops, int32_t max_windows, int32_t* d_crop_idx, int32_t* d_n_windows,
                     int32_t* d_window_span, int32_t* d_bad_count);

/* The cosine of every pair of live rows of every recording: the block-diagonal part of the corpus-wide matrix
 * svk_cosine_scores would write.
 *   d_emb         f32 [n_rec][seg_stride][dim], 4-byte aligned, 1 <= dim <= 512
 *   d_n_seg       int32 [n_rec]: live rows of each recording; a value outside [0, seg_stride] is clamped into it
 *   d_aff         f32 [n_rec][seg_stride][seg_stride]; entries with i or j >= d_n_seg[r] are NOT written
 * Arithmetic as svk_pair_scores' cosine: products, sums, square roots and the division in float64, a zero norm divides by 1 (a
 * zero row scores exactly 0), the result (float)(x.y / (||x|| ||y||)) rounded once.  The dot products run on
 * v_mfma_f64_16x16x4_f64, one wave per 16 x 16 tile of the upper triangle; k runs in super-steps of 16, inside one the
 * k = 16 S + 4 g + e in the order (e, g); the squared norms are summed per lane over its columns in order, then over g.  Since
 * sum |x_k y_k| <= ||x|| ||y||, the float64 value lies within (dim + 8) 2^-53 of the exact cosine: the output is float32(exact)
 * or, within that distance of a rounding boundary, its neighbour (tests/test_segment_affinity.py).
 *   symmetry      only entries with i <= j are computed; each is written to [i][j] and [j][i]: symmetric bit for bit
 *   bits          an entry depends on its two rows and dim alone -- not on n_rec, the slot, seg_stride, d_n_seg or the launch
 *                 geometry; runs are bit-identical.  16-byte loads (dim % 4 == 0 and a 16-byte aligned d_emb) and 4-byte loads
 *                 fill the same registers: the same bits
 *   NaN           a NaN (or Inf) row makes its own row and column NaN and touches nothing else
 * SVK_ERR_BAD_ARG: NULL context or buffer, negative size, dim outside [1, 512], misalignment, more tiles than one launch holds. */
int svk_segment_affinity(svk_ctx* ctx, const float* d_emb, int32_t n_rec, int32_t seg_stride, int32_t dim,
                         const int32_t* d_n_seg, float* d_aff);

/* Average-linkage agglomerative clustering of every recording on its SIMILARITY matrix (larger = closer: the cosines above, or
 * LLRs a caller writes there).  One workgroup per recording.  Definition (tests/ahc_f64_ref.py states it in NumPy and the kernel
 * reproduces it bit for bit), n = d_n_seg[r]:
 *   W             float64 [n][n], W[i][j] = W[j][i] = (double)d_aff[r][i][j] for i < j: only entries ABOVE the diagonal of live
 *                 rows are read; cluster sizes s = 1, k = n live clusters
 *   step          the live pair i < j with the largest W[i][j]; ties go to the lowest i, then the lowest j.  The step is taken
 *                 if k > max_clusters, or if k > min_clusters and W[i][j] >= threshold; otherwise clustering stops
 *   merge         j into i: for every other live m, W[m][i] = W[i][m] = (s_i W[m][i] + s_j W[m][j]) / (s_i + s_j) -- two products,
 *                 one sum, one quotient, each rounded once in float64, no fused multiply-add; then s_i += s_j, j is retired
 *   d_target      NULL, or int32 [n_rec]: a value >= 1 replaces BOTH min_clusters and max_clusters for that recording (a known
 *                 number of speakers); a target above n merges nothing
 *   d_labels      int32 [n_rec][seg_stride]: clusters numbered 0, 1, ... in the order of their lowest member; dead rows are not
 *                 written
 *   d_n_clusters  int32 [n_rec]
 *   d_merge_pair  NULL, or int32 [n_rec][seg_stride][2]: step t of a recording in slot t as (i, j); unused slots hold -1
 *   d_merge_sim   NULL, or float64 [n_rec][seg_stride]: W[i][j] of step t in slot t; unused slots hold NaN
 *   special       n == 0: 0 clusters;  n == 1: one cluster.  A recording with a non-finite live entry above the diagonal, or with
 *                 d_n_seg[r] outside [0, seg_stride], is NOT clustered: its labels are -1 (the live rows'; all seg_stride of
 *                 them when the count is out of range), its cluster count is -1, its merge slots are unused, and it adds 1 to
 *                 *d_bad_count (int32, may be NULL; the caller zeroes it).  Non-finite values below the diagonal or in dead
 *                 rows are never read
 *   instances     n <= svk_ahc_limits()[0] keeps W in LDS (128 rows, 129 float64 apart: 129 KiB of the 160); a larger recording works in
 *                 its slot of d_workspace.  Both run the same statements in the same order: the same bits
 *   d_workspace   svk_ahc_workspace_bytes(n_rec, seg_stride) bytes, 16-byte aligned: 0 (d_workspace may be NULL) when
 *                 seg_stride <= limits[0], else 8 seg_stride^2 bytes per recording; 0 for arguments the call rejects
 * The search keeps every row's best partner j > i and the global step is a reduction over rows: average linkage is reducible, so
 * a merge elsewhere changes a row's best only through the merged column, which is compared on the spot; the total order above
 * (ties included) is reproduced exactly.  The bits depend on the recording's matrix and the stop arguments alone: a recording
 * clustered alone gives the bits it gives in a batch, and runs are bit-identical.  At most n - 1 steps; no spin-waits.
 * svk_ahc_limits: out[0] = the largest n_seg that runs on the LDS instance, out[1] = the largest supported seg_stride (2 048).
 * SVK_ERR_BAD_ARG: NULL context or buffer, negative size, seg_stride above limits[1], min_clusters < 1, max_clusters <
 * min_clusters, a NaN threshold (+-infinity is allowed), misalignment, a short workspace. */
int svk_ahc_limits(int32_t out[2]);
size_t svk_ahc_workspace_bytes(int32_t n_rec, int32_t seg_stride);
int svk_ahc(svk_ctx* ctx, const float* d_aff, int32_t n_rec, int32_t seg_stride, const int32_t* d_n_seg, double threshold,
            int32_t min_clusters, int32_t max_clusters, const int32_t* d_target, void* d_workspace, size_t workspace_bytes,
            int32_t* d_labels, int32_t* d_n_clusters, int32_t* d_merge_pair, double* d_merge_sim, int32_t* d_bad_count);

/* Spectral embedding of every recording with the speaker count read off the eigengap (Ng-Jordan-Weiss; the neighbour count of
 * the graph chosen by the normalised maximum eigengap, Park et al. 2020) (csrc/spectral.hip).  svk_ahc on the cosines of the
 * embedding rows, with d_n_speakers as its target, gives the labels; svk_ahc's labels may also come first, as d_group, to reduce
 * a long recording to at most limits[0] nodes.  One workgroup per recording; asynchronous on the context's stream, no host round
 * trip, no floating-point atomics, no workgroup waits for another, every loop's trip count is bounded by the arguments.
 * Definition (tests/spectral_f64_ref.py states it in NumPy), n = d_n_seg[r]:
 *   nodes         d_group == NULL: node a is window a, m = n, M[a][b] = (double)d_aff[r][min(a, b)][max(a, b)].  Otherwise
 *                 d_group is int32 [n_rec][seg_stride] (svk_ahc's labels), m = 1 + the largest label of the live rows, and
 *                 M[a][b] = (sum over i in a, j in b of (double)d_aff[r][min(i, j)][max(i, j)]) / (double)(|a| |b|) for a != b
 *                 (the mean pairwise cosine: what average linkage holds).  ORDER OF ADDITIONS: one float64 accumulator from 0,
 *                 i over a's members ascending, inside it j over b's members ascending; one division.  Only entries ABOVE
 *                 the diagonal that join two live rows of DIFFERENT nodes are read; the diagonal of M is not used
 *   graph(p)      p clamped to m - 1.  Row a keeps its p largest M[a][b], b != a, ties to the lower b: B[a][b] = 1 there, else 0.
 *                 S = (B + B^T) / 2, D = diag(S 1), L = D - S: every entry a multiple of 1/2, exact in float64
 *   spectrum      all m eigenvalues of L by cyclic Jacobi, sorted ascending (equal values in the order of their index).
 *                 M2 = m rounded up to even (an index >= m is padding and pairs as an identity), H = M2 / 2.  A sweep is the
 *                 M2 - 1 rounds r = 0 .. M2 - 2 of the round-robin: pair 0 = {M2 - 1, r}, pair k = {(r + k) mod (M2 - 1),
 *                 (r - k) mod (M2 - 1)} for k = 1 .. H - 1, each written p < q.  A round takes every rotation from the matrix
 *                 as the round finds it: a_pq == 0 gives c = 1, s = 0, else theta = (a_qq - a_pp) / (2 a_pq),
 *                 t = copysign(1, theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c; then A <- J^T A J for
 *                 the product J of the round's rotations: x'_p = c x_p - s x_q, x'_q = s x_p + c x_q along columns, then along
 *                 rows, a pair's own a_pq (which the rotation annihilates) then set to zero outright; an entry and its
 *                 mirror image get the same bits.  Products may contract into fused multiply-adds.  Before every
 *                 sweep the largest off-diagonal magnitude is compared with 2^-52 ||L||_F: at or below it the diagonal is
 *                 the spectrum.  At most 30 sweeps, then one last comparison; a recording that fails it is bad
 *   count         g_i = lambda_(i+1) - lambda_i, i = 1 .. min(max_speakers, m - 1) (lambda_1 the smallest); k = the first i with
 *                 the largest g_i, raised to min_speakers, capped at m.  d_target: NULL, or int32 [n_rec]; a value >= 1
 *                 replaces k, capped at m and at max_speakers (the columns of d_embed); the ratio below is unaffected
 *   neighbours    candidates p_c = nb_lo + c nb_step, c = 0 .. nb_count - 1, clamped to m - 1; a candidate that clamps to the
 *                 p of the one before it is skipped (and so are all after it).  r(p) = p lambda_max / max_i g_i in float64,
 *                 +infinity when the largest gap is not positive; the smallest r wins, the first among equals.  Candidates
 *                 are solved for eigenvalues only; the winner again with vectors (the same eigenvalue bits)
 *   d_embed       f32 [n_rec][node_stride][max_speakers]: row a < m = (float)v_1[a] .. (float)v_k[a], then zeros; v_j is the
 *                 eigenvector of lambda_j of the chosen graph, its sign such that the entry of largest magnitude (the lowest
 *                 index among equals) is positive.  Rows a >= m are NOT written
 *   d_n_nodes, d_n_speakers, d_neighbours   int32 [n_rec]: m, k, the chosen (clamped) p
 *   d_eigval      NULL, or f64 [n_rec][node_stride]: the m eigenvalues of the chosen graph, ascending
 *   d_eigvec      NULL, or f64 [n_rec][max_speakers][node_stride]: v_1 .. v_k in float64 (rows j < k, entries a < m)
 *   d_graph       NULL, or u8 [n_rec][node_stride][node_stride]: 2 S of the chosen graph (the m x m block)
 *   d_ratio       NULL, or f64 [n_rec][nb_count]: r(p_c); NaN where the candidate was skipped
 *                 Of d_eigval, d_eigvec and d_graph only the elements named above are written (nothing past entry m, past
 *                 vector k or outside the m x m block, and nothing at all for a bad recording)
 *   special       m == 0: 0 nodes, 0 speakers, 0 neighbours.  m == 1: 1 node, 1 speaker, 0 neighbours, embedding row (1, 0, ...),
 *                 eigenvalue 0, eigenvector (1), graph (0).  Both leave d_ratio NaN
 *   bad           a non-finite affinity among the entries read; d_n_seg[r] outside [0, seg_stride]; a group label of a live row
 *                 outside [0, node_stride); a node below the largest label without a member; no convergence.  A bad recording
 *                 gets d_n_nodes = d_n_speakers = d_neighbours = -1, zeros in all node_stride rows of its d_embed slot, NaN in
 *                 its d_ratio slot, and adds 1 to *d_bad_count (int32, may be NULL; the caller zeroes it).  It touches no
 *                 other recording
 *   d_workspace   svk_spectral_workspace_bytes(n_rec, seg_stride, node_stride) bytes, 16-byte aligned: per recording 8 c^2 +
 *                 4 * (seg_stride rounded up to 4) bytes with c = max(2, node_stride rounded up to even) -- the eigenvectors
 *                 (transposed) and the member lists; 0 for arguments the call rejects
 *   LDS           sized by node_stride: L with c rows, c + 1 float64 apart, one byte per entry of the neighbour ranks and a few
 *                 vectors (150 KiB at 128 nodes, 39 KiB at 64)
 * The only rounding is inside the eigensolver.  The bits depend on the recording's live entries, its groups and the scalar
 * arguments alone -- not on n_rec, the slot or the launch geometry; a recording processed alone gives the bits it gives in a
 * batch, and runs are bit-identical.
 * svk_spectral_limits: out[0] = the largest node_stride (128), out[1] = the largest seg_stride (2 048), out[2] = the largest
 * max_speakers (16).
 * SVK_ERR_BAD_ARG: NULL context or required buffer, negative size, node_stride or seg_stride above the limits, d_group == NULL
 * with seg_stride > node_stride, nb_lo, nb_step or nb_count < 1, min_speakers < 1, max_speakers outside [min_speakers,
 * limits[2]], misalignment, a short workspace.  n_rec == 0 launches nothing and looks at no pointer. */
int svk_spectral_limits(int32_t out[3]);
size_t svk_spectral_workspace_bytes(int32_t n_rec, int32_t seg_stride, int32_t node_stride);
int svk_spectral_embed(svk_ctx* ctx, const float* d_aff, int32_t n_rec, int32_t seg_stride, const int32_t* d_n_seg,
                       const int32_t* d_group, int32_t node_stride, int32_t nb_lo, int32_t nb_step, int32_t nb_count,
                       int32_t min_speakers, int32_t max_speakers, const int32_t* d_target, void* d_workspace,
                       size_t workspace_bytes, float* d_embed, int32_t* d_n_nodes, int32_t* d_n_speakers, int32_t* d_neighbours,
                       double* d_eigval, double* d_eigvec, uint8_t* d_graph, double* d_ratio, int32_t* d_bad_count);

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

/* ---- ROC / EER / AUC on the device ------------------------------------------------------------
 * evaluation.py:47-52 (sklearn roc_curve + roc_auc_score + brentq on interp1d) for pair sets too
 * large for the host: LSD radix sort of the scores (descending, 8-bit digits, the label riding along;
 * -0.0 sorts as +0.0), scan of the labels, one point per distinct score, trapezoid AUC and the linear
 * root of 1 - fpr - tpr.  Every step is a reduce-then-scan over per-workgroup spans: no workgroup waits
 * on another.  d_labels: uint8, non-zero = positive.  n < 2^32.
 * d_workspace: svk_roc_workspace_bytes(n) bytes (about 18 B per pair).  h_out[4] (HOST) = {eer, auc,
 * positives, ROC points (distinct scores)}; the call synchronises the stream (its result is a host scalar). */
size_t svk_roc_workspace_bytes(int64_t n);
int svk_roc_eer(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, void* d_workspace,
                size_t workspace_bytes, double* h_out);

/* evaluation.py:11-33 (get_and_plot_k_eer_auc) in one call: with step = n / k, split s is the pairs
 * [s * step, (s + 1) * step); the last n - k * step pairs are ignored, as there.  Per split, as svk_roc_eer,
 * plus roc_curve(drop_intermediate=True) in counts: the distinct-score points, then (more than two of
 * them) only the first, the last and those where a second difference of fps or tps is non-zero, then the
 * prepended origin.  d_curve: NULL, or uint32 [2][k][step + 1] -- the fps plane, then the tps plane; fpr =
 * fps / fps[-1], tpr = tps / tps[-1] in float64 is sklearn's own arithmetic; entries of a split's rows at and
 * past its curve points are not written.  h_out (HOST) [k][4] = {eer, auc, positives, curve points}.
 * SVK_ERR_BAD_ARG (the message names the split) for a split with one class or a non-finite score, and for
 * k < 1 or step < 2.
 * d_workspace: svk_roc_k_workspace_bytes(n, k) bytes (0 for arguments svk_roc_k rejects); the splits run one
 * after another through it.  Synchronises the stream. */
size_t svk_roc_k_workspace_bytes(int64_t n, int32_t k);
int svk_roc_k(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, int32_t k, void* d_workspace,
              size_t workspace_bytes, uint32_t* d_curve, double* h_out);

/* svk_roc_eer plus the detection cost the VoxCeleb results are quoted with and the thresholds to decide with (the reference
 * has neither; on the host this is NumPy over sklearn's roc_curve(drop_intermediate=False): evaluation.get_min_dcf).  One sort
 * serves all of it.  h_ops (HOST) [n_op][3] = {p_target, c_miss, c_fa}, 0 <= n_op <= 8, 0 < p_target < 1, costs > 0.
 * h_out (HOST) [5 + 4 n_op] = {eer, auc, positives, points, eer_threshold}, then per operating point {min_dcf, threshold, p_miss,
 * p_fa}; the first four are svk_roc_eer's values for the same input, bit for bit (the same kernels in the same order).
 * The candidates are roc_curve's origin (reject everything: p_miss = 1, p_fa = 0, threshold +inf) and one point per distinct
 * score in descending order; the cost of a point is c_miss p (1 - tps / P) + c_fa (1 - p) fps / N in float64, min_dcf the
 * smallest cost / min(c_miss p, c_fa (1 - p)); among equal costs the FIRST point wins (the highest threshold).  threshold is
 * that point's score -- accept when score >= threshold -- and p_miss, p_fa the rates there.  eer_threshold is the score of the
 * first point where 1 - fpr - tpr <= 0 (the upper end of the segment the EER is interpolated on).  Strict like svk_roc_k: a
 * non-finite score or a single class is SVK_ERR_BAD_ARG, as are a bad operating point, n_op outside [0, 8], n < 2 or n >= 2^32
 * and a workspace below svk_roc_dcf_workspace_bytes(n) (0 for n < 2).  Synchronises the stream. */
size_t svk_roc_dcf_workspace_bytes(int64_t n);
int svk_roc_dcf(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const double* h_ops, int32_t n_op,
                void* d_workspace, size_t workspace_bytes, double* h_out);

/* Applies thresholds chosen on one set to another (actual DCF, false accepts / false rejects; replaces a comparison and a
 * masked sum per threshold in a framework): one streaming pass over UNSORTED scores.  h_thresholds (HOST) [n_thr] f32,
 * 1 <= n_thr <= 16, +-inf allowed, NaN not.  h_out (HOST) int64 [2 n_thr + 2]: [2 t] = targets (label != 0) with score >=
 * thr[t], [2 t + 1] = non-targets with score >= thr[t], [2 n_thr] = targets, [2 n_thr + 1] = non-targets.  A NaN score is never
 * accepted and counts only in its class total.  Integer counts, exact; n may exceed 2^32.  Synchronises the stream. */
int svk_decision_counts(svk_ctx* ctx, const float* d_scores, const uint8_t* d_labels, int64_t n, const float* h_thresholds,
                        int32_t n_thr, int64_t* h_out);

/* evaluation.py:112-134 (top-1 of each test utterance) in one streaming pass over d_scores [n_rows][n_cols]:
 * d_argmax[r] = np.argmax(row r) (the first maximum; a NaN is the maximum, the first NaN wins); d_true[r] = the
 * enrolled column of row r's speaker, -1 = not enrolled; d_labels: NULL, or uint8 [n_rows][n_cols], the one-hot
 * rows of d_true (all zeros for -1).  *h_correct (HOST) = rows with argmax == d_true.  Synchronises the stream. */
int svk_top1(svk_ctx* ctx, const float* d_scores, int64_t n_rows, int32_t n_cols, const int32_t* d_true,
             int32_t* d_argmax, uint8_t* d_labels, int64_t* h_correct);

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
 * svk_roc_dcf writes there for the same arguments (see above), and behind svk_roc_dcf's last kernel the hull passes run:
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

/* ---- score calibration and fusion (csrc/calibration.hip) ---------------------------------------
 * An affine map from the scores of n_sys systems to a calibrated log-likelihood ratio, llr = sum_d w_d s_d + b, fitted by
 * prior-weighted logistic regression on a development trial list (calibration.py runs the Newton iteration on the host; the
 * reference has no calibration).  svk_calibration_stats is the one pass over the trials an iteration needs, svk_calibration_apply
 * the map itself.  Both take the scores as planes: system d's score of trial p is d_scores[d * plane_stride + p], f32,
 * 0 <= d < n_sys, 0 <= p < n, with 1 <= n_sys <= 8, plane_stride >= n, d_scores 4-byte aligned.  16-byte loads when d_scores is
 * 16-byte aligned and (n_sys == 1 or plane_stride % 4 == 0) (and, for the statistics, d_labels is 4-byte aligned; for apply,
 * d_out 16-byte aligned), 4-byte loads otherwise: the same bits either way.  h_weights (HOST) float64 [n_sys + 1], the offset b
 * last; all finite.  Element indices and addresses are 64-bit; n may exceed 2^32 (not tested at that size).
 *
 * svk_calibration_stats: objective, gradient and Hessian of the regression at h_weights.  d_labels: uint8, non-zero = target.
 * With x_p = (s_0p, .., s_(n_sys-1)p, 1), c_p = h_class_weight[0] for a target and [1] for a non-target (HOST, float64, finite),
 * all in float64:
 *   z_p   = ((w_0 s_0p + w_1 s_1p) + ..) + b) + tau      each product and each sum rounded on its own, in that order
 *   e     = exp(-|z|),  lp = log1p(e),  q = 1 / (1 + e)      one exp, one log1p, one division per trial
 *   softplus(z) = max(z, 0) + lp;  sigma(z) = z >= 0 ? q : e q;  sigma(z) sigma(-z) = (e q) q
 *   L_tar = sum over targets of softplus(-z_p),  L_non = sum over non-targets of softplus(z_p)        (unweighted, nats)
 *   G     = sum_p c_p r_p x_p,  r_p = -sigma(-z_p) for a target, +sigma(z_p) for a non-target          (n_sys + 1 values)
 *   H     = sum_p c_p sigma(z_p) sigma(-z_p) x_p x_p^T, the upper triangle packed row by row   ((n_sys + 1)(n_sys + 2) / 2)
 * |z| of 745 and more gives e = 0 and the exact limits (softplus = max(z, 0), sigma = 0 or 1, H term 0), never NaN or Inf for
 * finite z.  h_out (HOST) float64 [2 + (n_sys + 1) + (n_sys + 1)(n_sys + 2) / 2] = {L_tar, L_non, G.., H..}; h_count (HOST)
 * int64 [3] = {targets, non-targets, skipped}.  A trial with a NaN or an infinite score in ANY system adds to no sum and to
 * neither class: it is counted in h_count[2].  With c = (p / N_tar, (1 - p) / N_non) and tau = log(p / (1 - p)),
 * c_0 L_tar + c_1 L_non is the prior-weighted objective and G, H its gradient and Hessian; with w = (1, 0), tau = 0,
 * Cllr = (L_tar / N_tar + L_non / N_non) / (2 ln 2).
 *   flags         bit 0 (1), value only: G and H are neither computed nor written (h_out holds 2 values), L_tar and L_non are
 *                 those of the full call bit for bit.  Every other bit must be 0
 *   order of additions   a function of n alone, the same for every output.  With Q = ceil(n / 4) quads of four consecutive
 *                 trials, S = ceil(ceil(Q / 256) / 2048) and W = ceil(Q / (256 S)) workgroups: workgroup g owns the quads
 *                 [256 S g, 256 S (g + 1)); thread t adds, from 0.0, the trials of its quads 256 S g + t + 256 k, k = 0, 1, ..,
 *                 in index order (at most 4 S additions); a 64-lane xor butterfly (32, 16, .., 1: 6 additions); the 4 wave
 *                 sums from 0.0 in wave order (4); then ONE workgroup adds the W rows: 16 groups of ceil(W / 16) consecutive
 *                 rows, each from 0.0 in index order, then the 16 group sums from 0.0 in order.  No floating-point atomics, no
 *                 workgroup waits on another: runs are bit-identical, on any device
 *   accuracy      every output is within (A + 8) 2^-52 sum_p |term_p| of the exact sum of its terms at the z_p above, A = 4 S +
 *                 6 + 4 + ceil(W / 16) + 16 the additions on the longest path and 8 covering exp, log1p, the division and the
 *                 products (tests/test_calibration_stats.py)
 *   d_workspace   svk_calibration_stats_workspace_bytes(n, n_sys) bytes, 16-byte aligned (the W rows of partial sums); 0 for
 *                 arguments the call rejects and for n == 0
 * n == 0 launches nothing, looks at no device pointer and returns zeros.  The call synchronises the stream (its results are
 * host scalars).  SVK_ERR_BAD_ARG: NULL context or buffer, negative n, n_sys outside [1, 8], plane_stride < n, misalignment
 * (scores: 4 bytes; workspace: 16), a non-finite weight, tau or class weight, undefined flag bits, a short workspace. */
size_t svk_calibration_stats_workspace_bytes(int64_t n, int32_t n_sys);
int svk_calibration_stats(svk_ctx* ctx, const float* d_scores, int32_t n_sys, int64_t plane_stride, const uint8_t* d_labels,
                          int64_t n, const double* h_weights, double tau, const double* h_class_weight, int32_t flags,
                          void* d_workspace, size_t workspace_bytes, double* h_out, int64_t* h_count);

/* d_out[p] = f32(((w_0 (double) s_0p + w_1 (double) s_1p) + ..) + b): float64 products and sums, each rounded on its own, in
 * the order d = 0, 1, .., then the offset; rounded to f32 once:  |d_out - ref| <= 2^-24 |ref| + (n_sys + 1) 2^-52 sum |terms|.
 * d_out: f32 [n], 4-byte aligned; it may be d_scores itself when n_sys == 1 (in place).  A non-finite score gives what IEEE
 * arithmetic gives; nothing is counted.  Asynchronous on the context's stream, no workspace; n == 0 launches nothing.
 * SVK_ERR_BAD_ARG: NULL context or buffer, negative n, n_sys outside [1, 8], plane_stride < n, misalignment, a non-finite
 * weight. */
int svk_calibration_apply(svk_ctx* ctx, const float* d_scores, int32_t n_sys, int64_t plane_stride, int64_t n,
                          const double* h_weights, float* d_out);

/* ---- score normalisation (csrc/snorm.hip) -------------------------------------------------------
 * The step between the raw score and the calibration: the shift and scale of a row's (an utterance's, a model's) impostor
 * scores, estimated on a cohort, are taken out of its trial scores (Z-, T-, S-norm; adaptive with top_k).  The reference has
 * no score normalisation.  All three entries are asynchronous on the context's stream and take no workspace.
 *
 * svk_cohort_moments: d_scores f32 [n_rows][row_stride], 4-byte aligned, the first n_cohort values of a row being that row's
 * scores against the cohort (svk_cosine_scores or svk_plda_scores: the caller's choice).  For every row:
 *   candidates    the finite scores; NaN and +-inf never are.  -0.0 counts as +0.0 and enters the sums as +0.0
 *   selection     m = min(top_k, candidates), top_k == 0 meaning all.  With v* the m-th largest candidate, the selected MULTISET
 *                 is every candidate strictly above v* and as many copies of v* as it takes to reach m: equal values are
 *                 interchangeable, no index order exists and none influences a bit.  v* is found exactly, by a radix select on
 *                 the order-preserving 32-bit key of the scores (four 8-bit digits over an LDS histogram); nothing is sorted
 *   d_moments     float64 [n_rows][2] = {mean, std}: mean = S / m, std = sqrt(sum (x - mean)^2 / m) (population form, two-pass,
 *                 from the centred values).  m == 0 gives {NaN, NaN}.  When all m selected values are equal (nothing lies
 *                 above v*) the mean is v* exactly and std is +0.0 exactly: a case of its own, no arithmetic runs
 *   d_used        int32 [n_rows] = m, or NULL;   d_kth  f32 [n_rows] = v* (NaN when m == 0), or NULL
 *   team          ONE team of T threads per row: T = 64 (a wave; four rows share a workgroup) for n_cohort <= 2048, T = 256 above
 *   order of additions   a function of n_cohort alone, the same for S and for the centred squares: lane l of the team adds,
 *                 from 0.0, the selected values above v* among its columns l, l + T, l + 2 T, .. in column order (a column
 *                 that is not selected contributes nothing: ceil(n_cohort / T) additions at most); a 64-lane xor butterfly (32,
 *                 16, .., 1: 6 additions); for T = 256 the 4 wave sums from 0.0 in wave order (4); then ONE term for the c
 *                 copies of v*, (double) c * v* (for the squares (double) c * ((v* - mean) * (v* - mean))).  Every product,
 *                 difference and sum is float64 and rounded on its own.  It does not depend on n_rows, the row's position, top_k
 *                 or the launch geometry; no floating-point atomics: a row computed alone gives the bits it gives inside a
 *                 batch, runs are bit-identical, and any top_k >= n_cohort gives the bits of top_k == 0
 *   residency     a row of up to 16 384 columns (ROW_LDS_MAX) is read from memory ONCE and kept in LDS (as keys, 64 KiB at
 *                 most: two workgroups to a CU) for the four select passes and the two moment passes; a longer row passes
 *                 through the same LDS buffer 16 384 columns at a time in each of the six passes (re-read through L2).  16-byte
 *                 loads when row_stride % 4 == 0 and d_scores is 16-byte aligned, 4-byte loads otherwise.  A lane owns the
 *                 same columns in the same order on every path: the same bits
 *   accuracy      with x the m selected values, d = x - (their exact mean), ref and ref_var their exact mean and variance, and
 *                 A = ceil(n_cohort / T) + 6 + (T == 256 ? 4 : 0) + 1 the additions on the longest path:
 *                   |mean - ref|      <= dm = (A + 2) 2^-52 sum |x| / m                 (+ 2: the product c v* and the division)
 *                   |std^2 - ref_var| <= (A + 4) 2^-52 sum d^2 / m + 2 dm sum |d| / m + dm^2 + 2^-51 ref_var
 *                 (+ 4: the difference, the square, the product with c and the division; the terms in dm: the centre is the
 *                 computed mean, not the exact one; 2^-51 ref_var: the square root, squared again by whoever compares.
 *                 tests/test_cohort_moments.py holds every row to it)
 * 1 <= n_cohort < 2^31; element offsets are 64-bit (n_rows * row_stride passes 2^31 at corpus size).  n_rows == 0 launches
 * nothing.  SVK_ERR_BAD_ARG: NULL context or buffer, negative n_rows, n_cohort < 1, top_k < 0, row_stride < n_cohort,
 * misalignment (f32 / int32: 4 bytes; float64: 8). */
int svk_cohort_moments(svk_ctx* ctx, const float* d_scores, int64_t n_rows, int32_t n_cohort, int64_t row_stride,
                       int32_t top_k, double* d_moments, int32_t* d_used, float* d_kth);

/* Z-, T- and S-norm of a score matrix from ONE expression.  d_scores f32 [n_rows][row_stride], n_cols scores per row; d_out f32
 * [n_rows][out_stride]; d_row_moments float64 [n_rows][2], d_col_moments float64 [n_cols][2] = {mean, std} as svk_cohort_moments
 * writes them, either may be NULL:
 *   both given    out = f32(0.5 * ((s - mu_r) / sd_r + (s - mu_c) / sd_c))                       (S-norm)
 *   one given     out = f32((s - mu) / sd) with that table: rows -> T-norm (the test side), columns -> Z-norm (the enrolled side)
 *   both NULL     SVK_ERR_BAD_ARG
 * All arithmetic is float64; each difference, quotient, sum and the product with 0.5 is rounded on its own, in the order
 * written, and the result is rounded to f32 once:  |out - ref| <= 2^-24 |ref| + 4 * 2^-52 (|t_r| + |t_c|), t the quotients.
 * A zero or NaN std and a non-finite score give what IEEE arithmetic gives; nothing is clamped, nothing is counted.
 * d_out may be d_scores itself, in place; out_stride must then equal row_stride (anything else is SVK_ERR_BAD_ARG).  16-byte loads and stores when both matrices are
 * 16-byte aligned and both strides are multiples of 4, 4-byte otherwise: the same bits.  n_rows == 0 or n_cols == 0 launches
 * nothing.  SVK_ERR_BAD_ARG: NULL context or buffer, negative size, n_cols >= 2^31, a stride below n_cols, misalignment (f32: 4
 * bytes; float64: 8). */
int svk_score_norm(svk_ctx* ctx, const float* d_scores, int64_t n_rows, int64_t n_cols, int64_t row_stride,
                   const double* d_row_moments, const double* d_col_moments, float* d_out, int64_t out_stride);

/* The same expression for a TRIAL LIST: d_out[p] is svk_score_norm's entry for the score d_scores[p] with the row moments
 * d_mom_a[d_idx_a[p]] and the column moments d_mom_b[d_idx_b[p]], bit for bit; the tables (float64 [n_a][2], [n_b][2]) are
 * indexed as svk_pair_scores indexes its matrices.  A table may be NULL (that side is left out, and only then may its index
 * list be NULL too); both NULL is SVK_ERR_BAD_ARG.  An index outside its table is the caller's error: nothing is read, that
 * trial's output is NaN and *d_bad_count (int32, may be NULL, the caller zeroes it) goes up by one.  d_out may be d_scores.
 * 16-byte loads and stores of the scores when d_scores and d_out are 16-byte aligned, 4-byte otherwise: the same bits.
 * n == 0 launches nothing.  SVK_ERR_BAD_ARG: NULL context or buffer, negative size, misalignment (f32 / int32: 4 bytes;
 * float64 / int64: 8). */
int svk_score_norm_pairs(svk_ctx* ctx, const float* d_scores, int64_t n, const double* d_mom_a, int64_t n_a,
                         const double* d_mom_b, int64_t n_b, const int64_t* d_idx_a, const int64_t* d_idx_b,
                         float* d_out, int32_t* d_bad_count);

/* ---- the embedding network --------------------------------------------------------------------------
 * Every entry of this section (svk_c3d2_stage1 .. svk_c3d2_fc5) writes its whole d_out (the first-block entries under flags bit
 * 5: all of it but pooled column 17, see there) and, beside it, only its workspace where
 * it has one: svk_c3d2_fc5's d_work, and svk_c3d2_stage2's d_act2 under SVK_C3D2_STAGE2_TWO_KERNELS.  The work-item counters
 * the persistent kernels draw tickets from live in the handle and are zeroed by every call: a result does not depend on what
 * ran on the handle before.
 *
 * ---- the first block ------------------------------------------------------------------------------
 * model.py:110-117 + :141-150 (C3D2): cube (utils.py:351-379) -> conv1_1 (1 -> 16, kernel (3,1,5)) -> BN -> PReLU
 * -> conv1_2 (16 -> 16, kernel (3,9,1), stride (1,2,1)) -> BN -> PReLU -> MaxPool3d((1,1,2)), eval mode, as ONE
 * kernel: conv1_1's output (3.3 MB per cube) lives only in LDS.  Since 0.1.8 on v_mfma_f32_16x16x32_f16 through TWO-PIECE
 * products: a value x travels as the halves h = f16(x), l = f16(x - h) (22 significant bits in four bytes) and
 * x w = h_x h_w + l_x h_w + h_x l_w, three f16 products, exact in the f32 they are accumulated in (measured on this network:
 * 1 - 5e-7 of the activation scale from the f64 convolution; the f32 direct form: 2 - 8e-7).  Direct form (the depth
 * transform's adds do not distribute over pieces), two taps per K = 32 block.  The host folds the BatchNorm statistics into
 * weights / biases, splits the weights and lays them out in the lane order of the MFMA's A operand (lane l = (co = l & 15,
 * kk = l >> 4), eight halves: K = 8 kk + e):
 *   d_w1blk [2][64][8 halves]: conv1_1, element e = tap t = 8 (kk & 1) + e (t = 5 kd + kw; t = 15 -> 0):
 *                        block 0 = H for every kk, block 1 = L for kk < 2 and 0 for kk >= 2;   d_bias1 [16]
 *   d_w2blk [14][2][64][8 halves]: conv1_2's tap pairs (a | b): pr < 12 -> a = (kd = pr / 4, kh = 2 (pr % 4)), b = (kd, kh + 1);
 *                        pr = 12 -> (0, 8) | (1, 8).  Element e = W2[co][ci = 8 (kk & 1) + e][tap a if kk < 2 else b];
 *                        block 0 = H pieces, block 1 = L pieces.  pr = 13 is the last tap (2, 8) ALONE, which the kernel reads
 *                        as one [h | l] fragment: block 0 = its H pieces at every kk, block 1 = its L pieces for kk < 2, 0 above;
 *                        d_bias2 [16];   d_slope1 / d_slope2 [16] PReLU slopes per channel
 * DOMAIN of the half-pair kernels (this one, svk_c3d2_stage2 / conv31 / conv32t / conv41): a value carries 22 significant bits
 * while |x| >= 2^-3, an absolute error floor of 2^-25 below that, and must stay under 65 504 (an f16's largest finite value; the
 * reference's features -- log mel energies, MFCCs, CMVN output -- are within +-100).  Weights have the same floor, which is why
 * the host fixes every channel's scale before it splits them (model.FusedEmbedder: activations of channel c are carried times
 * the power of two nearest 1 / (|gamma_c| + |beta_c|) of its BatchNorm, the next layer's weights take the inverse: exact, and
 * the tables no longer depend on how a checkpoint distributes a channel's scale between one layer and the next).
 * d_feat [n_utt][max_frames][40] f32, d_crop_idx [n_utt][20] as for svk_cube_gather (a start outside the clip -> zero rows, a
 * crop that runs off the clip -> zero rows from max_frames on; feature rows that no crop names are not read).
 * d_out: the activation after the pool, float32, channels last: [n_utt][16 d][36 h][18 w][16 c]
 * flags bit 1 (value 2) = the caller asserts every PReLU slope lies in [0, 1] (then prelu(v) = max(v, slope v): two
 * instructions per value instead of four).
 * flags bit 5 (value 32) = the 17-column form, on all four first-block entries (this one, svk_c3d2_stage1_c3 and the two *_multi):
 * The caller consumes the output through svk_c3d2_stage2 only.  Pooled column 17 (d_out[u][d][h][17][0..15]) is neither computed
 * nor written.  It keeps what it held on entry.  Columns 0 ... 16 are bit-identical to a call without the flag.  (Why column 17 is
 * dead: conv2_1 is 4 columns wide, so it has 15 output columns; conv2_2 is 1 wide and pool2 drops its 15th, so conv2_1's last
 * live column is 13, which reads pooled columns 13 ... 16.)  The launch then has 34 work items per cube instead of 36.
 * Every other bit must be 0: 1, 4, 8 and 16 are undefined and SVK_ERR_BAD_ARG, as is any bit above 5.
 * Geometry other than the 20 x 80 x 40 cube -> SVK_ERR_UNSUPPORTED (the torch module is the path for other models). */
size_t svk_c3d2_stage1_lds_bytes(void);
int svk_c3d2_stage1(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                    const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                    const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                    const float* d_slope2, int32_t flags, float* d_out);

/* The same first block for the three-channel model C3D2(n, 3) (constants.DERIVATIVE = True: train.py:197-205), replacing
 * utils.py:325-348 (FeatureCube3C: static, delta and delta-delta features cropped into a (3, 20, 80, 40) cube) and
 * model.py:110-117 + :141-150 with conv1_1 = Conv3d(3, 16, (3,1,5)).  Same arguments, checks and output as svk_c3d2_stage1 except:
 *   d_feat   [n_utt][3][max_frames][40] f32, channel-planar (channel 0 static, 1 delta, 2 delta-delta; FeatureCube3C's transpose).
 *            A (n, 3, 20, 80, 40) cube tensor is this layout with max_frames = 1 600 and crop starts 0, 80, ... 1 520.  The 20
 *            crop starts of a cube apply to all three channels; a start outside the clip -> zero rows, as for svk_c3d2_stage1
 *   d_w1blk  [3 ch][2][64][8 halves]: conv1_1 as three K = 32 blocks, one per input channel ch, each laid out as
 *            svk_c3d2_stage1's d_w1blk: tap t = 8 (kk & 1) + e of channel ch (t = 5 kd + kw; t = 15 is a zero pad), block 0 = H
 *            for every kk, block 1 = L for kk < 2 and 0 above.  (45 taps padded to 48: taps 16 ch + 15 are the pads)
 *   d_w2blk  as svk_c3d2_stage1 (conv1_2 is the same layer)
 * Half-pair domain as svk_c3d2_stage1: every feature value finite and below 65 504 in magnitude, an absolute floor of 2^-25.
 * Returns SVK_ERR_BAD_ARG (NULL buffer, misalignment, bad flags, negative size, too many cubes), SVK_ERR_UNSUPPORTED (geometry
 * other than 3 x 20 x 80 x 40, or a device with less LDS than svk_c3d2_stage1_c3_lds_bytes() + 64), SVK_ERR_HIP. */
size_t svk_c3d2_stage1_c3_lds_bytes(void);
int svk_c3d2_stage1_c3(svk_ctx* ctx, const float* d_feat, int32_t n_utt, int32_t max_frames, int32_t n_cols,
                       const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                       const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                       const float* d_slope2, int32_t flags, float* d_out);

/* K CUBES PER CLIP: the two first-block entries above with one more argument, cubes_per_clip = K >= 1.  A cube is 20 random
 * 0.8 s crops, so one cube stands for at most 16 s of a clip that may run to 145 s; K cubes of the same clip read the same
 * feature rows with K sets of crop starts, without those rows being copied K times:
 *   d_feat      [n_clips][max_frames][40] (svk_c3d2_stage1_multi) or [n_clips][3][max_frames][40] (svk_c3d2_stage1_c3_multi)
 *   d_crop_idx  [n_clips][K][20]: cube u = K clip + k reads clip u / K with the starts d_crop_idx[u][0 .. 19]
 *   d_out       [n_clips * K][16][36][18][16]: cube-major, what svk_c3d2_stage2 takes (cubes are independent from here on;
 *               svk_embedding_pool with rows_per_seg = K turns the K embeddings of a clip into one)
 * Everything else -- tables, flags, alignment, the half-pair domain, starts outside the clip -- as for the parent entry, and
 * every check of the parent applies to the cube count n_clips * K.  The output is bit-identical to the parent entry fed with
 * each clip's rows repeated K times (K = 1: to the parent entry itself); the parents' own kernels are untouched (the K-cube form
 * is a separate instance of the same kernel: it differs in where the feature-row base is formed, nothing else).
 * cubes_per_clip < 1 -> SVK_ERR_BAD_ARG. */
int svk_c3d2_stage1_multi(svk_ctx* ctx, const float* d_feat, int32_t n_clips, int32_t max_frames, int32_t n_cols,
                          const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                          const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                          const float* d_slope2, int32_t flags, float* d_out, int32_t cubes_per_clip);
int svk_c3d2_stage1_c3_multi(svk_ctx* ctx, const float* d_feat, int32_t n_clips, int32_t max_frames, int32_t n_cols,
                             const int32_t* d_crop_idx, int32_t n_crops, int32_t crop_frames, const void* d_w1blk,
                             const float* d_bias1, const float* d_slope1, const void* d_w2blk, const float* d_bias2,
                             const float* d_slope2, int32_t flags, float* d_out, int32_t cubes_per_clip);

/* The second block, model.py:119-124 + :151-158: conv2_1 (16 -> 32, kernel (3,1,4)) -> BN -> PReLU -> conv2_2
 * (32 -> 32, kernel (3,8,1), stride (1,2,1)) -> BN -> PReLU -> MaxPool3d((1,1,2)), ONE kernel on v_mfma_f32_16x16x32_f16
 * through two-piece products like svk_c3d2_stage1 (direct form; the weights of all taps sit in registers): conv2_1 is handed
 * to conv2_2 depth pair by depth pair through LDS, already split into (h, l) halves, so its activation never reaches memory;
 * epilogues carry bias, PReLU and the pool.
 *   d_in     [n_utt][16][36][18][16]  = svk_c3d2_stage1's output; pooled column 17 (d_in[u][d][h][17][.]) enters no product and
 *            may hold anything, NaNs included (svk_c3d2_stage1's flags bit 5 leaves it unwritten)
 *   d_w21blk [2 nt][6 pairs][2][64][8 halves]: conv2_1, lane l = (co = 16 nt + (l & 15), kk = l >> 4), element e =
 *            W[co][ci = 8 (kk & 1) + e][kd][kw + (kk >= 2)] of the tap pair 2 kd + kw / 2 (kw = 0, 2); block 0 = H, 1 = L
 *   d_w22blk [2 nt][24 taps][2][64][8 halves]: conv2_2, element e = W[co][ci = 8 kk + e][kd][kh], tap = 8 kd + kh; H | L
 *   d_bias / d_slope [32] per layer (BN folded; PReLU slope per channel)
 *   d_act2   may be NULL: it is never read or written.  Only with SVK_C3D2_STAGE2_TWO_KERNELS in the environment (read at every
 *            call: the two kernels this one replaced, kept as the reference its tests and A/B measurements run against, not as
 *            a second path to ship on) is it conv2_1's activation [n_utt][14][36][14][32] (scratch, f32; 14 of the layer's
 *            15 columns -- conv2_2 is one column wide and pool2 drops its 15th, so conv2_1's 15th is never computed), and NULL
 *            is SVK_ERR_BAD_ARG;
 *   d_out    [n_utt][12][15][7][32] (channels last)
 * flags bit 1 as for svk_c3d2_stage1; every other bit must be 0 (bit 5 belongs to the first-block entries alone). */
int svk_c3d2_stage2(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_w21blk, const float* d_bias21,
                    const float* d_slope21, const void* d_w22blk, const float* d_bias22, const float* d_slope22,
                    int32_t flags, float* d_act2, float* d_out);

/* conv3_1 (32 -> 64, kernel (3,1,3)) -> BN -> PReLU, model.py:126-128 + :159-161, one kernel on v_mfma_f32_16x16x32_f16
 * through two-piece products like svk_c3d2_stage1 (direct form, one tap per K = 32 block).
 *   d_in    [n_utt][12][15][7][32]   = svk_c3d2_stage2's output
 *   d_wblk  [4 nt][9 taps][2][64][8 halves]: lane (co = 16 nt + (l & 15), kk = l >> 4), e: W31[co][ci = 8 kk + e][kd][kw],
 *           tap 3 kd + kw (BatchNorm folded); block 0 = H = f16(w), block 1 = L = f16(w - H);  d_bias / d_slope [64]
 *   flags   bit 1: the caller asserts every PReLU slope lies in [0, 1]; every other bit must be 0
 *   d_out   [n_utt][10 d][8 chunks of 8 channels][5 w][15 h][8]: chunked and column-major, what svk_c3d2_conv32t stages from */
int svk_c3d2_conv31(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
                    const float* d_slope, int32_t flags, float* d_out);

/* conv3_2 (64 -> 64, kernel (3,7,1)) -> BN -> PReLU, model.py:129-131 + :162-164, one kernel on v_mfma_f32_16x16x32_f16
 * through two-piece products like svk_c3d2_stage1 (direct form; per (cube, column) work items; csrc/c3d2.hip):
 *   d_in    [n_utt][10][8][5][15][8] = svk_c3d2_conv31's output
 *   d_wblk  [4 nt][2 kb][21 taps][2][64][8 halves]: lane (co = 16 nt + (l & 15), kk = l >> 4), e: W32[co][ci = 32 kb + 8 kk + e][kd][kh],
 *           tap 7 kd + kh (BatchNorm folded); block 0 = H = f16(w), block 1 = L = f16(w - H);  d_bias / d_slope [64]
 *   d_out   [n_utt][8][8][45][8]     = what svk_c3d2_conv41 takes                                                       */
int svk_c3d2_conv32t(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
                     const float* d_slope, int32_t flags, float* d_out);
/* conv4_1 (64 -> 128, kernel (3,1,3)) -> BN -> PReLU, model.py:132-135 + :165-166, one kernel on v_mfma_f32_16x16x32_f16
 * through two-piece products like svk_c3d2_stage1 (direct form; one cube per work item, staged whole; csrc/c3d2.hip):
 *   d_in    [n_utt][8][8][45][8]     = svk_c3d2_conv32t's output
 *   d_wblk  [8 nt][9 taps][2 kb][2][64][8 halves]: lane (co = 16 nt + (l & 15), kk = l >> 4), e: W41[co][ci = 32 kb + 8 kk + e][kd][kw],
 *           tap 3 kd + kw (BatchNorm folded); block 0 = H = f16(w), block 1 = L = f16(w - H);  d_bias / d_slope [128]
 *   flags   bit 1: the caller asserts every PReLU slope lies in [0, 1]; every other bit must be 0
 *   d_out   [n_utt][6][16][27 = 9 h x 3 w][8]: chunked [cube][depth][channel / 8][pixel][channel % 8], what svk_c3d2_conv42 takes */
int svk_c3d2_conv41(svk_ctx* ctx, const float* d_in, int32_t n_utt, const void* d_wblk, const float* d_bias,
                    const float* d_slope, int32_t flags, float* d_out);
/* The end of the network, model.py:136-139 (definitions) + :167-170 (forward): conv4_2 (128 -> 128, kernel (3,7,1)) -> BN -> PReLU,
 * flatten, FC5 (4 608 -> 128) -- GEMMs over the BATCH on v_mfma_f32_16x16x4_f32 (csrc/c3d2_tail.hip): an M tile is one output
 * position of 16 cubes; conv4_2 runs through Winograd's F(2, 3) along depth with the input transform applied once while a
 * chunk is staged into LDS and the weight transform applied by the HOST.
 *   svk_c3d2_conv42  d_in  [n_utt][6][16][27][8] = svk_c3d2_conv41's output
 *                    d_wfrag [8 nt][16 chunks][7 kh][4 k][64][2]: lane (co = 16 nt + (l & 15), kk = l >> 4), e:
 *                            G_k[co][8 chunk + 2 kk + e][kh], G0 = g0, G1 = (g0 + g1 + g2) / 2, G2 = (g0 - g1 + g2) / 2,
 *                            G3 = g2 over the three depth taps g of the BN-folded weights;  d_bias / d_slope [128]
 *                    d_out [n_utt][4][16][9 = 3 h x 3 w][8]
 *   flags            bit 1: the caller asserts every PReLU slope lies in [0, 1]
 *   svk_c3d2_fc5     d_in  [n_utt][4 608] = svk_c3d2_conv42's output, K index ((d * 16 + chunk) * 9 + pixel) * 8 + channel % 8
 *                    d_wfrag [4 d][8 nt][72][64][4]: lane (j = 16 nt + (l & 15), kk = l >> 4), e: W5[j][column of K index
 *                            1 152 d + 16 step + 4 kk + e] (model.py:168 flattens NCDHW: column = channel * 36 + d * 9 + pixel)
 *                    d_bias [128];  d_work: svk_c3d2_fc5_workspace_floats(n_utt) floats (partial sums of the four K ranges,
 *                    added in a fixed order: bitwise repeatable);  d_out [n_utt][128]                                  */
int svk_c3d2_conv42(svk_ctx* ctx, const float* d_in, int32_t n_utt, const float* d_wfrag, const float* d_bias,
                    const float* d_slope, int32_t flags, float* d_out);
size_t svk_c3d2_fc5_workspace_floats(int32_t n_utt);
int svk_c3d2_fc5(svk_ctx* ctx, const float* d_in, int32_t n_utt, const float* d_wfrag, const float* d_bias, float* d_work,
                 float* d_out);

/* The classification head, model.py:170-174 (forward, development=True: F.softmax(FC6(PReLu5(x)))) and the accuracy pass of
 * train.py:104-119 (torch.max of that softmax, hits against the true labels), widened to top-k (csrc/head.hip):
 *   d_emb    [n][128] f32 (svk_c3d2_fc5's output), 16-byte aligned;  prelu_slope: PReLu5's one slope
 *   d_w6     [n_labels][128] f32, FC6.weight as stored (row-major, 16-byte aligned);  d_b6 [n_labels] f32
 *   d_probs  NULL, or [n][n_labels] f32 (64-bit offsets): the softmax
 *   d_topk   NULL, or [n][k] int32: label indices in descending order of p, ties to the lower index (1 <= k <= 8)
 *   d_true   NULL, or [n] int32 true labels; then h_hits (HOST) [k] int64: hits[r] = rows whose true label is among their
 *            first r + 1 (a label of -1 or outside [0, n_labels) never counts).  Synchronises the stream when d_true is given.
 * Arithmetic, per row:
 *   - z = PReLU5(x); l = FC6(z) in exact f32 on v_mfma_f32_16x16x4_f32: f32 products and accumulation in a fixed order
 *     (eight 16-product fma chains added pairwise, then the bias), no half pairs;
 *   - m = max l (NaN if a logit is NaN), e = exp(l - m), s = sum of e in f32 in a fixed order (compensated), p = e / s
 *     (IEEE division);
 *   - d_topk is the stable descending sort of the p the kernel writes (a NaN above every number, as torch.sort puts it), bit
 *     for bit, whether or not d_probs is asked for: a NaN row's top-1 is its first NaN, as torch.argmax and svk_top1 give;
 *   - a row's results depend on that row and the weights alone, not on n or the launch geometry; runs are bit-identical.
 * 1 <= n_labels <= 65 536, n >= 0 (0: no launch).  SVK_ERR_BAD_ARG for k < 1 or k > n_labels when d_topk or d_true is given,
 * NULL weights, d_true without h_hits; SVK_ERR_UNSUPPORTED for k > 8 or n_labels > 65 536.  No workspace: the hit counters
 * live in the context. */
int svk_c3d2_head(svk_ctx* ctx, const float* d_emb, int64_t n, int32_t n_labels, float prelu_slope, const float* d_w6,
                  const float* d_b6, float* d_probs, int32_t k, int32_t* d_topk, const int32_t* d_true, int64_t* h_hits);


/* ---- multi-GPU: the one exchange step of the path ------------------------------------------------
 * Utterances shard over the GPUs of a node with no data-path exchange until scoring; then every rank needs
 * the enrolled embeddings: ONE all-gather of the [rows_per_rank][dim] float32 shards over RCCL / xGMI
 * (the reference has no collective, only in-process DataParallel, train.py:40-41).  One process
 * per GPU, one context per process.  A torch host uses torch.distributed instead (distributed.py); these
 * entry points serve a host without torch.  RCCL is loaded at the first call (dlopen), not at link time.
 *   rank 0: svk_comm_unique_id(ctx, id)  -> ship the 128 bytes to the other ranks by any host channel
 *   all   : svk_comm_init(ctx, id, n_ranks, rank)            (collective: every rank must call it)
 *   all   : svk_allgather_f32(ctx, d_send, d_recv, count)    d_recv holds n_ranks x count floats, rank-major;
 *           asynchronous on the context's stream like every launch
 *   all   : svk_comm_destroy(ctx)                                                                          */
int svk_comm_unique_id(svk_ctx* ctx, char out[128]);
int svk_comm_init(svk_ctx* ctx, const char id[128], int32_t n_ranks, int32_t rank);
int svk_allgather_f32(svk_ctx* ctx, const float* d_send, float* d_recv, size_t count_per_rank);
int svk_comm_destroy(svk_ctx* ctx);
/* out[0] = ranks of the context's communicator (0 = none), out[1] = this rank */
int svk_comm_info(const svk_ctx* ctx, int32_t out[2]);

/* History -- one version or addition per line, newest first.  0.1.12 (SVK_VERSION 114) kept its number through every addition;
 * the ten entries of the first four lines came under it too, declared at first in headers of their own, since folded in here.
 * 0.1.12  + svk_knn_cluster, svk_knn_cluster_workspace_bytes (corpus clustering: shared-neighbour components of k-NN lists)
 * 0.1.12  + svk_cosine_topk_norm, svk_cosine_topk_norm_workspace_bytes (the speaker search ranked by normalised scores)
 * 0.1.12  + svk_rocch, svk_rocch_workspace_bytes, svk_rocch_level_counts_offset, svk_rocch_max_vertices, svk_pav_apply (the ROC convex hull: minCllr, ROCCH-EER, PAV)
 * 0.1.12  + svk_vad_adaptive (the level-adaptive VAD: per-clip thresholds from two quantiles of the frame energies)
 * 0.1.12  + svk_spectral_embed, svk_spectral_limits, svk_spectral_workspace_bytes (spectral clustering for diarization: batched Jacobi eigendecompositions of graph Laplacians, the speaker count from the eigengap, the neighbour count by the normalised maximum eigengap)
 * 0.1.12  + svk_window_crops, svk_segment_affinity, svk_ahc, svk_ahc_limits, svk_ahc_workspace_bytes (speaker diarization: sliding-window crop tables, the window-against-window cosines of every recording and average-linkage clustering, one workgroup per recording)
 * 0.1.12  + svk_cohort_moments, svk_score_norm, svk_score_norm_pairs (adaptive score normalisation: the top-K cohort moments of every row by an exact radix select, and Z- / T- / S-norm from them)
 * 0.1.12  + svk_calibration_stats, svk_calibration_stats_workspace_bytes, svk_calibration_apply (score calibration and fusion: the statistics of a prior-weighted logistic regression in one pass, and the affine map)
 * 0.1.12  + svk_plda_scores, svk_plda_scores_workspace_bytes, svk_plda_pair_scores (PLDA log-likelihood ratios: the score matrix on the f32 matrix pipe, trial lists in float64)
 * 0.1.12  svk_c3d2_stage2 runs as one kernel and no longer touches d_act2, which may be NULL (same results, bit for bit)
 * 0.1.12  + svk_class_scatter, svk_class_scatter_workspace_bytes, svk_embedding_project (the embedding back end: class statistics in float64 and centre / project / length-normalise in one pass)
 * 0.1.12  + svk_cosine_topk, svk_cosine_topk_workspace_bytes (the k best gallery rows of every query without the score matrix; chunked galleries through an accumulate flag)
 * 0.1.12  + svk_pair_scores (one score per trial of a list), svk_roc_dcf, svk_roc_dcf_workspace_bytes (minDCF and the EER / minDCF thresholds on the ROC sort), svk_decision_counts (accepts at given thresholds); the AUC of svk_roc_eer / svk_roc_k is summed in a fixed order (same bits on every run)
 * 0.1.12  + svk_c3d2_stage1_multi, svk_c3d2_stage1_c3_multi (K cubes per clip), svk_embedding_pool (the mean over groups of embedding rows)
 * 0.1.12  + svk_delta_cmvn_stats, svk_delta_planes, svk_cube_gather_delta (the three-channel input from static features in one statistics pass and one writing pass)
 * 0.1.12  + svk_c3d2_head (PReLU5 -> FC6 -> softmax, top-k and hits: the classification head); tests/test_identification.py pins the number
 * 0.1.11  + svk_roc_k, svk_roc_k_workspace_bytes (k-fold splits, roc_curve in counts), svk_top1; the ROC sort and scans are the library's own kernels (no hipCUB)
 * 0.1.10  + svk_c3d2_stage1_c3 (the three-channel first block, DERIVATIVE = True)
 * 0.1.9   conv1_2's last tap as ONE [h | l] fragment (d_w2blk pair 13 = [H | H], [L | 0]: 41 MFMAs per tile, not 42), conv2_1 leaves out the column pool2 makes dead (d_act2 [..][14][32]); half-pair domain stated
 * 0.1.8   svk_c3d2_stage1 / svk_c3d2_stage2 / svk_c3d2_conv31 / svk_c3d2_conv32t run on the f16 matrix pipe through two-piece products (new weight tables: half-pair blocks)
 * 0.1.7   gathered front-end input (svk_vad_energy d_src_frame -> svk_frontend_run d_src_chunk)
 * 0.1.6   one kernel per network layer (svk_c3d2_conv32, svk_bias_prelu, svk_cube_gather_windows and the direct-form flag bits are gone); + svk_cmvn_stats, svk_cube_gather_cmvn
 */

#ifdef __cplusplus
}
#endif
#endif /* SVK_H */
