// Fused front end for gfx950: PCM -> [pre-emphasis] -> frames -> rFFT power spectrum ->
// frame energy -> mel filterbank -> [log] -> [DCT-II] -> [c0 := log E].
//
// Replaces, per clip, /root/reference/speech_feature_extraction/speechpy/
//   processing.py:45-58 (preemphasis, circular)   processing.py:112-138 (framing, no padding)
//   processing.py:142-174 (|rfft|^2 / nfft)       feature.py:202-205 (frame energy, 0 -> eps)
//   feature.py:216-217 (mel projection, 0 -> eps) feature.py:146-153 (log, DCT-II ortho, c0 := log E)
//
// Work decomposition: one workgroup per CU, as many waves as LDS allows (up to 12); the
// workgroup copies the filterbank / DCT operand fragments into LDS once (they are re-read
// for every tile: fetching them from L2 per tile cost 4x the PCM traffic and its latency),
// then every wave works on its own: it owns a TILE of 8 (or 16) consecutive frames of one
// clip, a private LDS slice, and loops over tiles with no further workgroup barrier (the waves
// of a workgroup draw the workgroup's tiles from a counter in LDS).  The two standard
// configurations run instances with their framing and output shape fixed at compile time (Spec).
//   1. the tile's sample span is read from HBM once with 16-byte loads issued back to back and
//      parked in LDS -- int16 clips as raw int16 (pre-emphasis x[n] - c x[n-1] is applied when a
//      frame is read), float clips or an unusual pre-emphasis shift as pre-emphasised f32;
//   2. 512-point complex FFTs run across the wave, two per trip pipelined through one scratch:
//      8 points per lane, three radix-8 passes in registers on packed-f32 instructions
//      (fft_wave.h), two transposes through a padded (bank-conflict-free) LDS scratch.  nfft = 512 packs TWO real frames into one
//      complex FFT; nfft = 1024 packs the even/odd samples of ONE frame.  The untangle step
//      pairs bin k with bin N-k, which lives in lane 64-l: one wave shuffle per register, no
//      LDS, and only for the bins the mel filters read;
//   3. those power bins go to a [TILE x KP] LDS tile; the frame energy (all bins) comes from
//      Parseval's identity: per-lane partial sums, three DPP adds to 8 group sums parked behind the
//      frame's power bins, finished by two MFMAs against ones -- and only when something consumes it;
//   4. mel energies^T = filterbank x P^T on v_mfma_f32_16x16x4_f32 (exact f32), skipping
//      the 16-bin chunks where a 16-filter tile is identically zero (Q2: the bank is
//      ~97 % zeros);  log;  the accumulator layout of that product is exactly the B
//      operand layout of the next one, so cepstra^T = DCT x log(mel)^T follows with no
//      data movement;
//   5. results go straight to HBM.
// (v_mfma_f32_4x4x1_16b_f32, which could follow the bank's sparsity filter group by filter
// group, was measured at 15 cycles per instruction = half the MAC rate of 16x16x4:
// tools/probes/mfma4x4_probe.hip -- not worth it.)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "fft_wave.h"
#include "svk_internal.h"

using namespace svk_fft;

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int RAW_OFF = 8;    // int16 staging: samples start 16 bytes in, slot RAW_OFF-1 holds the sample before the span
constexpr int MAX_FT = 4;    // 16-filter tiles  (<= 64 filters)
constexpr int PT_PAD = 8;    // ptile row padding (floats): conflict-free ds_read_b128; also holds the frame's 8 energy group sums
constexpr float EPS64 = 2.220446049250313e-16f;  // np.finfo(float).eps, functions.py:62

// Phase-ablation switches for tuning: compiled in only with -DSVK_TUNING
// (`make TUNING=1`), selected at run time by SVK_FE_ABLATE = 1 skip staging | 2 skip the FFT loop |
// 4 skip mel..output | 8 skip the mel MFMAs | 16 skip the DCT | 32 skip log..output | 64 skip zero fill.
#ifdef SVK_TUNING
#define SVK_ABLATE(p, bit) (((p).ablate & (bit)) != 0)
#else
#define SVK_ABLATE(p, bit) false
#endif

struct FrontendParams {
  const void* pcm;
  const int64_t* offsets;
  const int32_t* lengths;
  int64_t clip_stride;
  int32_t clip_len;
  // Gathered input (int16 PCM only): a clip's signal is the concatenation of CHUNKS of `chunk` samples of its PCM, chunk q of
  // clip u = PCM chunk src_chunk[u * chunk_stride + q] -- the index form of svk_vad_energy's compaction (d_src_frame): the
  // kept frames are read where they lie instead of being copied to the front of a second buffer first.  NULL = plain clips.
  const int32_t* src_chunk;
  int32_t chunk, chunk_stride;
  float chunk_inv;   // 1 / chunk: sample index -> chunk without an integer division (indices stay below 2^24: exact in float)
  int32_t n_utt, max_frames, tiles_per_utt;
  int32_t flen, flen_eff, stride, nfilt, ncols, out_kind, dc_elim, preemph, pre_shift;
  float pre_cof;
  float escale;      // input_scale^2: applied to the frame energy (the mel path carries it in the bank weights)
  int32_t kp;        // power bins kept for the mel product, multiple of 16
  int32_t sig_bytes; // LDS bytes reserved for the staged samples (multiple of 16)
  int32_t n_ft, n_ct;
  int32_t chunk_lo[MAX_FT], chunk_hi[MAX_FT];
  const cplx* tw1;    // [8][64]  W512^(lane*r)
  const cplx* tw2;    // [8][64]  W64^((lane&7)*r)
  const cplx* tw3;    // [5][64]  W1024^(lane+64q), q<4; [4][0] = W1024^256
  const f32x4* fbfrag;  // [n_slots][64]: only the non-zero (filter tile, 16-bin chunk) blocks
  const float* dctfrag; // [n_ct][n_ft][4][64]
  int32_t n_slots, slot_base[MAX_FT];  // block (t, u) lives in slot slot_base[t] + u - chunk_lo[t]
  int32_t table_bytes, wave_bytes;     // LDS: shared tables, then one slice per wave
  int32_t need_energy; // frame energies are consumed (c0 := log E, or d_energy given)
  int32_t n_steps; // register steps a frame reaches: ceil(flen_eff / 64), or / 128 for nfft 1024
  int32_t ablate;  // tuning only (SVK_FE_ABLATE): 1 skip staging, 2 skip the FFT loop, 4 skip mel/DCT/output
  float* feat;
  float* energy;
  int32_t* n_frames;
};

template <typename PcmT>
__device__ __forceinline__ void stage_span(const FrontendParams& p, const PcmT* x, int64_t s0, int need,
                                           int len, float* sig, int lane) {
  constexpr int V = 16 / (int)sizeof(PcmT);
  typedef PcmT vec_t __attribute__((ext_vector_type(V)));
  const bool fast = (!p.preemph || p.pre_shift == 1) && ((reinterpret_cast<uintptr_t>(x + s0) & 15) == 0);
  for (int i = lane * V; i < need; i += 64 * V) {
    const int64_t idx = s0 + i;
    float v[V];
    float o[V];
    if (fast && idx + V <= len) {
      vec_t raw = *reinterpret_cast<const vec_t*>(x + idx);
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = (float)raw[e];
      if (p.preemph) {
        const float prev = (float)x[idx == 0 ? len - 1 : idx - 1];
        o[0] = v[0] - p.pre_cof * prev;
#pragma unroll
        for (int e = 1; e < V; ++e) o[e] = v[e] - p.pre_cof * v[e - 1];
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = v[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int64_t id = idx + e;
        float val = 0.f;
        if (id < len) {
          val = (float)x[id];
          if (p.preemph) {
            int64_t j = (id - p.pre_shift) % len;
            if (j < 0) j += len;
            val -= p.pre_cof * (float)x[j];
          }
        }
        o[e] = val;
      }
    }
#pragma unroll
    for (int e = 0; e < V; e += 4)
      *reinterpret_cast<f32x4*>(sig + i + e) = (f32x4){o[e], o[e + 1], o[e + 2], o[e + 3]};
  }
}

// int16 clips with no pre-emphasis or the usual shift of 1: park the RAW samples (2 bytes each,
// half the LDS of the f32 form) and pre-emphasise when a frame is read: x[n] - c * x[n-1] needs
// one extra sample in front of the span (the clip's LAST sample when the span starts the clip:
// np.roll wraps, Q5).
// `tab` (gathered input, FrontendParams::src_chunk): sample j of the clip's signal = x[tab[j / chunk] * chunk + j % chunk]; chunk is a
// multiple of 8 and every span starts on a multiple of 8, so a 16-byte vector never straddles two chunks.
// q = j / chunk from a float reciprocal, corrected by one step either way (an integer division is ~40 vector instructions, four
// of them per lane and tile were 8 % of this issue-bound kernel): j < 2^24 (the host checks), so (float)j is exact and the
// estimate is off by at most one.
__device__ __forceinline__ int64_t gathered_index(const int32_t* tab, int chunk, float chunk_inv, int64_t j) {
  const int ji = (int)j;
  int q = (int)((float)ji * chunk_inv);
  int r = ji - q * chunk;
  if (r < 0) { --q; r += chunk; }
  if (r >= chunk) { ++q; r -= chunk; }
  return (int64_t)tab[q] * chunk + r;
}

__device__ __forceinline__ void stage_raw16(bool pre, const int16_t* x, int64_t s0, int need, int len, int16_t* sigh,
                                            int lane, const int32_t* tab = nullptr, int chunk = 0, float chunk_inv = 0.f) {
  typedef short vec_t __attribute__((ext_vector_type(8)));
  constexpr int NV = 3;  // 16-byte loads in flight per lane: an 8-frame tile at a 160-sample hop is 3 x 512 samples
  if (lane == 0 && pre) {
    const int64_t jp = s0 == 0 ? (int64_t)len - 1 : s0 - 1;
    sigh[RAW_OFF - 1] = x[tab ? gathered_index(tab, chunk, chunk_inv, jp) : jp];
  }
  // wave-uniform: the span starts on a 16-byte boundary and its last vector ends inside the clip
  // (every tile of a clip but possibly the last one), so no load needs patching
  const bool whole = (tab ? (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (s0 & 7) == 0
                          : (reinterpret_cast<uintptr_t>(x + s0) & 15) == 0) && s0 + ((need + 7) & ~7) <= len;
  if (whole) {
    for (int base = 0; base < need; base += NV * 512) {
      vec_t raw[NV];
      // all loads first (a load per loop trip followed by its own wait cost one HBM round trip EACH) ...
      if (tab) {
        int64_t src[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int i = base + k * 512 + lane * 8;
          src[k] = gathered_index(tab, chunk, chunk_inv, s0 + (i < need ? i : 0));   // (the table entries first: dependent loads)
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) raw[k] = *reinterpret_cast<const vec_t*>(x + src[k]);
      } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int i = base + k * 512 + lane * 8;
          raw[k] = *reinterpret_cast<const vec_t*>(x + s0 + (i < need ? i : 0));  // clamped: always a valid aligned address
        }
      }
      // ... then the LDS writes
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = base + k * 512 + lane * 8;
        if (i < need) *reinterpret_cast<vec_t*>(sigh + RAW_OFF + i) = raw[k];
      }
    }
  } else {
    for (int i = lane * 8; i < need; i += 64 * 8) {
      vec_t raw;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t j = s0 + i + e;
        raw[e] = j < len ? x[tab ? gathered_index(tab, chunk, chunk_inv, j) : j] : (short)0;
      }
      *reinterpret_cast<vec_t*>(sigh + RAW_OFF + i) = raw;
    }
  }
}

// Sums of two values over each group of 8 consecutive lanes, DPP adds only: an inclusive scan inside
// the 16-lane rows (row_shr 1, 2, 4; lanes shifted in from outside the row read 0) leaves the sum of
// lanes 8 m .. 8 m + 7 in lane 8 m + 7.  Written as v_add_f32_dpp (add and lane move in ONE
// instruction; the update_dpp builtin costs a zero-init, a move and an add per step); a VALU result
// needs two wait states before a DPP read, which the other value's step plus one s_nop provide.
// The 8 group sums of a frame are finished by the matrix cores (see the energy MFMA below).
__device__ __forceinline__ void group8_sum2(float& a, float& b) {
  asm volatile(
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %1, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "s_nop 1"
      : "+v"(a), "+v"(b));
}

// Frame samples -> the 8 complex registers of a lane.  NSTEPS = how many of the 8 register steps
// the frame reaches (frame_len / 64, or / 128 for the even-odd packing, rounded up); steps
// before the last are read unconditionally, the last one clamps its address and masks, the
// rest are the zero padding up to nfft (Q6).  Straight-line code: per-lane `if (n < frame_len)`
// around every read cost 28 exec-mask branches and as many serialised LDS round trips per FFT.
typedef const volatile __attribute__((address_space(3))) int16_t* lds_i16p;  // volatile needs the LDS address space spelled out
typedef const volatile __attribute__((address_space(3))) int* lds_i32p;
template <bool SPLIT1024, bool RAW16>
struct FrameReader {
  const float* sig;
  const int16_t* sigh;
  int off_a, off_b, flen;
  float cof;
  bool hasb;
  int lane;

  // PRE is a template parameter, not a select: with the LDS read of x[n-1] inside a `pre ? :`
  // arm the compiler emitted a branch per sample, each read followed by its own s_waitcnt
  // (20 serialised LDS round trips per FFT); straight-line code batches the reads.  The raw
  // samples are read through a volatile pointer so that x[n-1], x[n] are NOT merged into one
  // 2-byte-misaligned ds_read_b32 (measured: the merged form made the nfft-1024 kernel 16 % slower).
  template <bool PRE>
  __device__ __forceinline__ float sample(int off, int idx) const {
    if constexpr (RAW16) {
      const lds_i16p s = (lds_i16p)(sigh + RAW_OFF + off + idx);
      const float x0 = (float)s[0];
      if constexpr (PRE) return x0 - cof * (float)s[-1];  // x[n] - c x[n-1] (shift 1), Q5
      return x0;
    } else {
      return sig[off + idx];
    }
  }

  // Samples idx, idx + 1 (idx even) of the even/odd packing.  ALIGNED: the pair sits on a 4-byte
  // boundary (even hop), one ds_read_b32; the sample before it is one more 2-byte read.
  template <bool PRE, bool ALIGNED>
  __device__ __forceinline__ cplx pair(int off, int idx) const {
    if constexpr (RAW16) {
      const lds_i16p s = (lds_i16p)(sigh + RAW_OFF + off + idx);
      float x0, x1;
      if constexpr (ALIGNED) {
        const int w = *(lds_i32p)s;
        x0 = (float)(short)w;
        x1 = (float)(w >> 16);
      } else {
        x0 = (float)s[0];
        x1 = (float)s[1];
      }
      if constexpr (PRE) return mk(x0 - cof * (float)s[-1], x1 - cof * x0);
      return mk(x0, x1);
    } else {
      return mk(sig[off + idx], sig[off + idx + 1]);
    }
  }

  template <int NSTEPS, bool PRE, bool ALIGNED>
  __device__ __forceinline__ void read(cplx (&v)[8]) const {
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const int first = SPLIT1024 ? 2 * (lane + 64 * a) : lane + 64 * a;
      if (a + 1 < NSTEPS) {
        if (SPLIT1024) {
          v[a] = pair<PRE, ALIGNED>(off_a, first);
        } else {
          const float yb = sample<PRE>(off_b, first);
          v[a] = mk(sample<PRE>(off_a, first), hasb ? yb : 0.f);
        }
      } else if (a + 1 == NSTEPS) {
        if (SPLIT1024) {
          const bool in0 = first < flen, in1 = first + 1 < flen;  // the sample after the frame is staged or slack: finite, masked
          const cplx y = pair<PRE, ALIGNED>(off_a, in0 ? first : 0);
          v[a] = mk(in0 ? y.x : 0.f, in1 ? y.y : 0.f);
        } else {
          const bool in = first < flen;
          const float xa = sample<PRE>(off_a, in ? first : 0), xb = sample<PRE>(off_b, in ? first : 0);
          v[a] = mk(in ? xa : 0.f, (in && hasb) ? xb : 0.f);
        }
      } else {
        v[a] = mk(0.f, 0.f);
      }
    }
  }

  template <bool PRE, bool ALIGNED>
  __device__ __forceinline__ void read_steps(int n_steps, cplx (&v)[8]) const {
    switch (n_steps) {  // wave-uniform; each case is straight-line code
      case 1: read<1, PRE, ALIGNED>(v); break;
      case 2: read<2, PRE, ALIGNED>(v); break;
      case 3: read<3, PRE, ALIGNED>(v); break;
      case 4: read<4, PRE, ALIGNED>(v); break;
      case 5: read<5, PRE, ALIGNED>(v); break;
      case 6: read<6, PRE, ALIGNED>(v); break;
      case 7: read<7, PRE, ALIGNED>(v); break;
      default: read<8, PRE, ALIGNED>(v); break;
    }
  }
};

// Natural log of a mel / frame energy.  With integer PCM an energy is either the eps that replaces
// an exact zero or at least ~1e-3 (one LSB), never a float32 denormal, so the bare v_log_f32
// (log2, 1 ulp) x ln 2 is safe: two instructions.  Float PCM can be arbitrarily quiet: keep the
// denormal-safe library expansion there.
template <bool INT_PCM>
__device__ __forceinline__ float fast_log(float x) {
  if constexpr (INT_PCM)
    return __builtin_amdgcn_logf(x) * 0.69314718055994530942f;
  else
    return __logf(x);
}

// Spec: configuration values fixed at compile time (>= 0) or read from the launch parameters (-1).
// The generic kernel (every field -1) serves any plan; the two standard front ends get an instance
// with their framing and output shape folded in, which removes the per-frame dispatch branches,
// most scalar bookkeeping and the scalar-register spills that came with it.
struct SpecGeneric {
  static constexpr int MAX_THREADS = 768;  // 12 waves: up to 168 VGPRs each
  static constexpr int STRIDE = -1, FLEN = -1, N_STEPS = -1, PRE = -1, KP = -1, NEED_ENERGY = -1, N_FT = -1, N_CT = -1,
                       OUT_KIND = -1, NFILT = -1, NCOLS = -1, DC_ELIM = -1;
};
// speechpy.feature.mfcc(fs 16 kHz, 20 ms / 10 ms, 40 filters, 13 cepstra, nfft 512), with or without
// the fused pre-emphasis (PRE stays a launch parameter: one wave-uniform branch per frame read)
struct SpecMfcc13 {
  static constexpr int MAX_THREADS = 1024;  // 16 waves of <= 128 VGPRs: this instance fits, and its LDS slice allows 15
  static constexpr int STRIDE = 160, FLEN = 320, N_STEPS = 5, PRE = -1, KP = 128, NEED_ENERGY = 1, N_FT = 3, N_CT = 1,
                       OUT_KIND = SVK_OUT_MFCC, NFILT = 40, NCOLS = 13, DC_ELIM = 1;
};
// the model's front end: lmfe(25 ms / 10 ms, 40 filters, nfft 1024) (load_data.py:64-70), with or without
// the fused pre-emphasis
struct SpecLmfe40 {
  static constexpr int MAX_THREADS = 768;
  static constexpr int STRIDE = 160, FLEN = 400, N_STEPS = 4, PRE = -1, KP = 256, NEED_ENERGY = 0, N_FT = 3, N_CT = 0,
                       OUT_KIND = SVK_OUT_LMFE, NFILT = 40, NCOLS = 40, DC_ELIM = 0;
};

// The configuration as every phase reads it: a field is a compile-time constant where the Spec fixes it
// (the select folds away) and the launch parameter otherwise.
template <typename Spec>
struct Cfg {
  static constexpr int FFT_STEPS = Spec::N_STEPS > 0 ? Spec::N_STEPS : 8;  // register steps the transform takes as non-zero
  int stride, flen, flen_eff, n_steps, preemph, kp, need_energy, n_ft, n_ct, out_kind, nfilt, ncols, dc_elim;
  static __device__ __forceinline__ int pick(int fixed, int launched) { return fixed >= 0 ? fixed : launched; }
  __device__ __forceinline__ explicit Cfg(const FrontendParams& p)
      : stride(pick(Spec::STRIDE, p.stride)), flen(pick(Spec::FLEN, p.flen)), flen_eff(pick(Spec::FLEN, p.flen_eff)),
        n_steps(pick(Spec::N_STEPS, p.n_steps)), preemph(pick(Spec::PRE, p.preemph)), kp(pick(Spec::KP, p.kp)),
        need_energy(pick(Spec::NEED_ENERGY, p.need_energy)), n_ft(pick(Spec::N_FT, p.n_ft)), n_ct(pick(Spec::N_CT, p.n_ct)),
        out_kind(pick(Spec::OUT_KIND, p.out_kind)), nfilt(pick(Spec::NFILT, p.nfilt)), ncols(pick(Spec::NCOLS, p.ncols)),
        dc_elim(pick(Spec::DC_ELIM, p.dc_elim)) {}
};

// 8-frame tiles: the FFT scratch lies over rows 4..7 of the power tile (and a little beyond); the
// spectra of frames 4..7 wait in registers (2-4 floats per lane and frame) until the tile's last FFT
// is done.  nfft 1024 (wide rows, KP = 256): 4.2 KB less LDS per wave, 8 -> 12 waves per CU for the
// model's front end; nfft 512: 2.2 KB less, 12 -> 15 waves for the MFCC instance.
constexpr bool alias_scr(int tile) { return tile == 8; }

// A wave's view of LDS: the workgroup's operand fragments, then its own slice [staged samples | power tile | FFT scratch]
struct WaveLds {
  const f32x4* fb;
  const float* dct;
  float* sig;      // the staged span as f32 ...
  int16_t* sigh;   // ... or as raw int16 (the same bytes)
  float* ptile;    // [TILE][prow]
  int prow;        // kp + PT_PAD
  cplx* scr;
};

struct Twiddles {
  cplx t1[8], t2[8], t3[5];
};

// One transform's input: the 8 complex registers of a lane (nfft 512: frame f in .x, frame f + 1 in .y; nfft 1024: the
// even / odd samples of one frame), the per-lane Parseval partial sums of the first / second frame, and
// za / zb: the first / second frame of a packed pair (nfft 512) is all zeros.  The untangling separates the two spectra
// only to rounding: a silent frame would inherit ~1e-14 of its partner's power where SpeechPy has an exact 0 (-> eps,
// feature.py:217), so its power bins are written as 0.  (nfft 1024 transforms one frame: no partner.)
struct Frames {
  cplx v[8];
  float ea, eb;
  bool za, zb;
};

// untangle hands its results to a sink, step by step: `step(j, pa, pb)` takes the power of the first / second frame
// at bin lane + 64 j (only for 64 j < kp), `energy(ea, eb)` their energy group sums (only when they are consumed).
// Step j = 4 (bins 256..287) exists only when the bank reaches bin 256 = nfft/4 of a 1024-point transform
// (kp = 288: SpeechPy's bank at any rate but 16 kHz, Q2).
//
// RowPower keeps them in registers (see alias_scr) ...
struct RowPower {
  float pa[5], pb[5], ea, eb;
  __device__ __forceinline__ void step(int j, float a, float b) { pa[j] = a, pb[j] = b; }
  __device__ __forceinline__ void energy(float a, float b) { ea = a, eb = b; }
};

// ... and TileRows, the one row writer, puts them into tile row f (nfft 512: the second frame into row f + 1; a lone
// last frame writes its zero partner into a row >= nvalid of the tile: masked at the output), the group sums into
// the 8 padding floats behind the row's power bins.
template <bool SPLIT1024, typename C>
struct TileRows {
  const C& c;
  float *rowa, *rowb;
  int lane;
  __device__ __forceinline__ TileRows(const C& c_, const WaveLds& w, int f, int lane_)
      : c(c_), rowa(w.ptile + f * w.prow), rowb(rowa + w.prow), lane(lane_) {}
  __device__ __forceinline__ void step(int j, float pa, float pb) const {
    const int k = lane + 64 * j;
    if (64 * (j + 1) <= c.kp) {  // wave-uniform: no exec masking
      rowa[k] = pa;
      if (!SPLIT1024) rowb[k] = pb;
    } else if (k < c.kp) {  // ragged last step only
      rowa[k] = pa;
      if (!SPLIT1024) rowb[k] = pb;
    }
  }
  __device__ __forceinline__ void energy(float ea, float eb) const {
    if ((lane & 7) == 7) {
      rowa[c.kp + (lane >> 3)] = ea;
      if (!SPLIT1024) rowb[c.kp + (lane >> 3)] = eb;
    }
  }
  __device__ __forceinline__ void put(const RowPower& r) const {  // a held row, once the scratch is dead
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (64 * j < c.kp) step(j, r.pa[j], r.pb[j]);
    if (c.need_energy) energy(r.ea, r.eb);
  }
};

template <bool SPLIT1024, bool RAW16, typename C>
__device__ __forceinline__ void load_frames(const C& c, const WaveLds& w, float pre_cof, int f, int nvalid, int lane,
                                            Frames& fr) {
  const bool pre = RAW16 && c.preemph != 0;
  const bool hasb = !SPLIT1024 && f + 1 < nvalid;
  const FrameReader<SPLIT1024, RAW16> rd{w.sig, w.sigh, f * c.stride, (hasb ? f + 1 : f) * c.stride, c.flen_eff,
                                         pre_cof, hasb, lane};
  if (SPLIT1024 && RAW16 && ((f * c.stride) & 1) == 0) {  // RAW_OFF is even: the pairs are 4-byte aligned
    if (pre) rd.template read_steps<true, true>(c.n_steps, fr.v);
    else rd.template read_steps<false, true>(c.n_steps, fr.v);
  } else {
    if (pre) rd.template read_steps<true, false>(c.n_steps, fr.v);
    else rd.template read_steps<false, false>(c.n_steps, fr.v);
  }
  fr.za = false, fr.zb = false;
  if constexpr (!SPLIT1024) {
    bool nza = false, nzb = false;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      nza |= fr.v[a].x != 0.f;
      nzb |= fr.v[a].y != 0.f;
    }
    fr.za = __builtin_amdgcn_ballot_w64(nza) == 0;  // wave-uniform
    fr.zb = __builtin_amdgcn_ballot_w64(nzb) == 0;
  }
  // Frame energy = sum over ALL nfft/2+1 power bins (feature.py:202).  By Parseval that is
  // sum(x^2)/2 + (X[0]^2 + X[nfft/2]^2) / (2 nfft), so only the bins the mel filters read
  // (k < kp) have to be untangled.
  // (skipped altogether when nobody reads the energy: log-mel output without d_energy)
  fr.ea = 0.f, fr.eb = 0.f;
  if (c.need_energy) {
    cplx e2 = mk(0.f, 0.f);  // (sum re^2, sum im^2): one packed fma per register
#pragma unroll
    for (int a = 0; a < 8; ++a) e2 = __builtin_elementwise_fma(fr.v[a], fr.v[a], e2);
    fr.ea = SPLIT1024 ? 0.5f * (e2.x + e2.y) : 0.5f * e2.x;
    fr.eb = 0.5f * e2.y;
  }
}

// The transformed registers -> the power bins the mel filters read (k < kp) and the energy group sums, into `out`.
template <bool SPLIT1024, typename C, typename Sink>
__device__ __forceinline__ void untangle(const C& c, const Frames& fr, const cplx (&t3)[5], int lane, Sink& out) {
  const cplx(&v)[8] = fr.v;
  const bool lane0 = lane == 0;
  const int mirror = (64 - lane) & 63;
  float ea = fr.ea, eb = fr.eb;
  if (lane0 && c.need_energy) {
    if (SPLIT1024) {  // X[0] = Re + Im, X[512] = Re - Im of Z[0]
      ea += (v[0].x * v[0].x + v[0].y * v[0].y) * (1.0f / 1024.0f);
    } else {          // X1[0], X1[256] = Re Z[0], Re Z[256];  X2: the imaginary parts
      ea += fr.za ? 0.f : (v[0].x * v[0].x + v[4].x * v[4].x) * (1.0f / 1024.0f);
      eb += fr.zb ? 0.f : (v[0].y * v[0].y + v[4].y * v[4].y) * (1.0f / 1024.0f);
    }
  }
  cplx carry = v[0];  // lane 0 pairs bin 64 j with bin 64 (8 - j): one register later
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (64 * j < c.kp) {
      const cplx sm = shfl2(v[7 - j], mirror);
      const cplx zk = v[j], zn = lane0 ? carry : sm;
      carry = sm;
      if (SPLIT1024) {
        // X[k] = E + W^k O  with  E = (Zk + conj Zn)/2,  O = (Zk - conj Zn)/(2i)
        // 2 E = Zk + conj Zn,  2 O = -i (Zk - conj Zn) = (zk.y + zn.y, -(zk.x - zn.x)); the 1/2's are folded into the filterbank weights
        const cplx E2 = add_conj(zk, zn), Ot = swap_add_conj(zk, zn);  // Ot = conj(2 O)
        cplx xp = E2 + cmul_conj(t3[j], Ot);
        xp *= xp;
        out.step(j, xp.x + xp.y, 0.f);  // 4 nfft |X[k]|^2
      } else {
        // 2 X1 = Zk + conj Zn,  2i X2 = Zk - conj Zn  (|.|^2 is what matters)
        cplx xa = add_conj(zk, zn), xb = swap_add_conj(zk, zn);
        xa *= xa;
        xb *= xb;
        out.step(j, fr.za ? 0.f : xa.x + xa.y, fr.zb ? 0.f : xb.x + xb.y);  // 4 nfft |X[k]|^2
      }
    }
  }
  if (c.need_energy) {
    // 64 per-lane partial sums -> 8 (one per 8 lanes); the mel stage adds them up with two more MFMAs
    // against a matrix of ones.
    group8_sum2(ea, eb);  // (eb is idle for nfft 1024: its slot still hides ea's DPP wait states)
    out.energy(ea, eb);
  }
}

// Two transforms per trip (4 frames at nfft 512, 2 at nfft 1024), pipelined through the one
// scratch (fft512_wave_x2).  A missing second transform (ragged last tile of a clip) redoes
// the first and drops the result: one code path.  The body both trip loops of power_tile share.
template <bool SPLIT1024, bool RAW16, typename C, typename Sink>
__device__ __forceinline__ void fft_trip(const C& c, const WaveLds& w, const Twiddles& tw, float pre_cof, int fa, int nvalid,
                                         int lane, Sink&& outa, Sink&& outb) {
  constexpr int FR_PER_FFT = SPLIT1024 ? 1 : 2;
  const bool two = fa + FR_PER_FFT < nvalid;  // wave-uniform
  Frames a, b;
  load_frames<SPLIT1024, RAW16>(c, w, pre_cof, fa, nvalid, lane, a);
  load_frames<SPLIT1024, RAW16>(c, w, pre_cof, two ? fa + FR_PER_FFT : fa, nvalid, lane, b);
  fft512_wave_x2<C::FFT_STEPS>(a.v, b.v, w.scr, lane, tw.t1, tw.t2);
  untangle<SPLIT1024>(c, a, tw.t3, lane, outa);
  if (two) untangle<SPLIT1024>(c, b, tw.t3, lane, outb);
}

// The tile's power rows.  `n` = nvalid, or 0 under SVK_ABLATE bit 2.
template <bool SPLIT1024, bool RAW16, int TILE, typename C>
__device__ __forceinline__ void power_tile(const C& c, const WaveLds& w, const Twiddles& tw, float pre_cof, int n, int lane) {
  constexpr int FR_PER_FFT = SPLIT1024 ? 1 : 2;
  typedef TileRows<SPLIT1024, C> Rows;
  if constexpr (alias_scr(TILE)) {
    // trips that fill rows 0..3 store directly, the later ones (rows 4..7, under the scratch) keep their
    // results in `held` -- unrolled so that `held` is indexed statically.  (Two loops: with both kinds of trip in one
    // body the generic int16 nfft-1024 instance grew past the full-unroll limit, the loop stayed rolled and `held`
    // went to scratch memory, 208 bytes per lane.)
    constexpr int TRIPS = 8 / (2 * FR_PER_FFT), DIRECT = TRIPS / 2, NHELD = 2 * (TRIPS - DIRECT);
    RowPower held[NHELD] = {};
#pragma unroll
    for (int t = 0; t < DIRECT; ++t) {
      const int fa = 2 * FR_PER_FFT * t;
      if (fa < n)  // wave-uniform
        fft_trip<SPLIT1024, RAW16>(c, w, tw, pre_cof, fa, n, lane, Rows(c, w, fa, lane), Rows(c, w, fa + FR_PER_FFT, lane));
    }
#pragma unroll
    for (int t = DIRECT; t < TRIPS; ++t) {
      const int fa = 2 * FR_PER_FFT * t;
      if (fa < n) fft_trip<SPLIT1024, RAW16>(c, w, tw, pre_cof, fa, n, lane, held[2 * (t - DIRECT)], held[2 * (t - DIRECT) + 1]);
    }
    wave_sync();  // the scratch is dead: rows 4..7 may be written
#pragma unroll
    for (int q = 0; q < NHELD; ++q) {
      const int f = 4 + FR_PER_FFT * q;  // first frame of held FFT q
      if (f < n) Rows(c, w, f, lane).put(held[q]);  // wave-uniform
    }
  } else {
    for (int fa = 0; fa < n; fa += 2 * FR_PER_FFT)
      fft_trip<SPLIT1024, RAW16>(c, w, tw, pre_cof, fa, n, lane, Rows(c, w, fa, lane), Rows(c, w, fa + FR_PER_FFT, lane));
  }
}

// mel^T = fb x P^T (f32 MFMA), block-sparse over 16-bin chunks: lane (jf, g) ends up with mel[filter 16 t + 4 g + reg][frame jf]
template <int TILE, typename C>
__device__ __forceinline__ void mel_product(const C& c, const FrontendParams& p, const WaveLds& w, int lane,
                                            f32x4 (&acc)[MAX_FT]) {
  const int jf = lane & 15, g = lane >> 4;
  const float* pb = w.ptile + (jf & (TILE - 1)) * w.prow + 4 * g;  // an 8-frame tile repeats its rows in N = 8..15
#pragma unroll
  for (int t = 0; t < MAX_FT; ++t) {
    // two accumulators per filter tile: back-to-back MFMAs never wait on their own result
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    if (t < c.n_ft && !SVK_ABLATE(p, 8)) {
      const f32x4* frag = w.fb + (p.slot_base[t] - p.chunk_lo[t]) * 64 + lane;
      for (int u = p.chunk_lo[t]; u < p.chunk_hi[t]; u += 2) {  // the plan makes every chunk range even
        const f32x4 a0 = frag[u * 64], a1 = frag[(u + 1) * 64];
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(pb + 16 * u);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(pb + 16 * (u + 1));
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0], b0[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[1], b0[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[2], b0[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[3], b0[3], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[0], b1[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[1], b1[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[2], b1[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[3], b1[3], acc1, 0, 0, 0);
      }
    }
    acc[t] = acc0 + acc1;
  }
}

// frame energy = ones x (the 8 group sums of the frame): every output row of the tile is that sum,
// so each lane ends up with the energy of ITS frame jf (feature.py:202-205); 0 when nothing consumes it
template <int TILE, typename C>
__device__ __forceinline__ float frame_energy(const C& c, const WaveLds& w, float escale, int lane) {
  if (!c.need_energy) return 0.f;
  const int jf = lane & 15, g = lane >> 4;
  const float* pe = w.ptile + (jf & (TILE - 1)) * w.prow + c.kp + g;
  f32x4 oe = (f32x4){0.f, 0.f, 0.f, 0.f};
  oe = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, pe[0], oe, 0, 0, 0);
  oe = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, pe[4], oe, 0, 0, 0);
  const float e = oe[0] * escale;
  return e == 0.f ? EPS64 : e;
}

// mel energies: 0 -> eps (feature.py:217); unless they are the output, their log, 0 in the rows past the last filter
template <bool INT_PCM, typename C>
__device__ __forceinline__ void log_mel(const C& c, int g, f32x4 (&acc)[MAX_FT]) {
#pragma unroll
  for (int t = 0; t < MAX_FT; ++t) {
    if (t < c.n_ft) {  // wave-uniform: an absent filter tile costs nothing
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = acc[t][r];
        m = m == 0.f ? EPS64 : m;  // feature.py:217
        if (c.out_kind != SVK_OUT_MFE) {
          m = fast_log<INT_PCM>(m);
          if (16 * t + 12 + 3 >= c.nfilt) m = (16 * t + 4 * g + r) < c.nfilt ? m : 0.f;  // only the ragged last tile
        }
        acc[t][r] = m;
      }
    }
  }
}

// MFE / LMFE: the lane's four filters of every filter tile to its frame's output row
template <typename C>
__device__ __forceinline__ void store_filters(const C& c, const f32x4 (&acc)[MAX_FT], float* orow, bool row_ok, int g) {
#pragma unroll
  for (int t = 0; t < MAX_FT; ++t) {
    const int filt = 16 * t + 4 * g;
    if (row_ok && t < c.n_ft) {
      if ((c.ncols & 3) == 0 && filt + 3 < c.nfilt) {
        *reinterpret_cast<f32x4*>(orow + filt) = acc[t];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (filt + r < c.nfilt) orow[filt + r] = acc[t][r];
      }
    }
  }
}

// cepstra^T = DCT x log(mel)^T: acc[t][r] is already the B operand; c0 := log E under dc_elimination
template <bool INT_PCM, typename C>
__device__ __forceinline__ void store_cepstra(const C& c, const FrontendParams& p, const WaveLds& w, const f32x4 (&acc)[MAX_FT],
                                              float e_frame, float* orow, bool row_ok, int lane) {
  const int g = lane >> 4;
  const float le = fast_log<INT_PCM>(e_frame);
  for (int ct = 0; ct < (SVK_ABLATE(p, 16) ? 0 : c.n_ct); ++ct) {  // runtime loop: keeps the table loads of one cepstral tile in flight, not four
    f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* dfrag = w.dct + ct * c.n_ft * 4 * 64 + lane;
#pragma unroll
    for (int t = 0; t < MAX_FT; ++t) {
      if (t < c.n_ft) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          o = __builtin_amdgcn_mfma_f32_16x16x4f32(dfrag[(t * 4 + r) * 64], acc[t][r], o, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cep = 16 * ct + 4 * g + r;
      if (row_ok && cep < c.ncols) orow[cep] = (cep == 0 && c.dc_elim) ? le : o[r];  // feature.py:151-152
    }
  }
}

// rows of this tile past the clip's last frame: defined (zero) output
template <int TILE, typename C>
__device__ __forceinline__ void zero_fill(const C& c, const FrontendParams& p, float* out_rows, int utt, int f0, int nvalid,
                                          int lane) {
  const int first_bad = nvalid > 0 ? nvalid : 0;
  int last = p.max_frames - f0;
  last = last > TILE ? TILE : last;
  for (int i = first_bad * c.ncols + lane; i < last * c.ncols; i += 64) out_rows[i] = 0.f;
  if (p.energy)
    for (int i = first_bad + lane; i < last; i += 64) p.energy[(int64_t)utt * p.max_frames + f0 + i] = 0.f;
}

// The driver: table copy and the one barrier, the ticket loop, a tile's clip geometry, the wave_syncs between the
// phases above and the SVK_ABLATE exits.
template <typename PcmT, bool SPLIT1024, int TILE, bool RAW16, typename Spec>
__global__ __launch_bounds__(Spec::MAX_THREADS) void frontend_kernel(const FrontendParams p) {
  const Cfg<Spec> c(p);
  constexpr bool INT_PCM = sizeof(PcmT) == 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // shared by the workgroup: mel and DCT operand fragments
  f32x4* fb_lds = reinterpret_cast<f32x4*>(smem);
  float* dct_lds = reinterpret_cast<float*>(smem + (size_t)p.n_slots * 64 * sizeof(f32x4));
  for (int i = threadIdx.x; i < p.n_slots * 64; i += blockDim.x) fb_lds[i] = p.fbfrag[i];
  for (int i = threadIdx.x; i < c.n_ct * c.n_ft * 4 * 64; i += blockDim.x) dct_lds[i] = p.dctfrag[i];
  int* tile_counter = reinterpret_cast<int*>(smem + p.table_bytes - 16);
  if (threadIdx.x == 0) *tile_counter = 0;
  __syncthreads();  // the only workgroup-wide barrier; from here on waves never wait for each other
  // private to this wave
  // the wave index is uniform: say so, or every per-tile index computation lands on the VALU
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = blockDim.x >> 6;
  char* mine = smem + p.table_bytes + (size_t)wave * p.wave_bytes;
  float* ptile = reinterpret_cast<float*>(mine + p.sig_bytes);
  const int prow = c.kp + PT_PAD;
  const WaveLds w{fb_lds, dct_lds, reinterpret_cast<float*>(mine), reinterpret_cast<int16_t*>(mine), ptile, prow,
                  reinterpret_cast<cplx*>(ptile + (alias_scr(TILE) ? 4 : TILE) * prow)};
  const int lane_id = threadIdx.x & 63;

  Twiddles tw;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    tw.t1[r] = p.tw1[r * 64 + lane_id];
    tw.t2[r] = p.tw2[r * 64 + lane_id];
  }
  if (SPLIT1024) {
#pragma unroll
    for (int q = 0; q < 5; ++q) tw.t3[q] = p.tw3[q * 64 + lane_id];
  }
  // The workgroup owns tiles {r * grid * n_waves + block * n_waves + w}: n_waves consecutive tiles per
  // round r (neighbours share the overlapping PCM in L1).  Its waves take them in that order from a
  // counter in LDS rather than by a fixed stride: tiles differ in cost (a clip's last tile, clips
  // shortened by the VAD), and with fixed shares the waves of a CU finished up to 17 % apart.
  const int tpu = p.tiles_per_utt;
  const unsigned total_tiles = (unsigned)p.n_utt * (unsigned)tpu;  // < 2^31: checked by svk_frontend_run
  const unsigned round_stride = gridDim.x * (unsigned)n_waves;
  for (;;) {
    int ticket = 0;
    if (lane_id == 0) ticket = atomicAdd(tile_counter, 1);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    const unsigned round = (unsigned)ticket / (unsigned)n_waves;
    const unsigned tile = round * round_stride + blockIdx.x * (unsigned)n_waves + ((unsigned)ticket - round * (unsigned)n_waves);
    if (round > total_tiles / round_stride || tile >= total_tiles) break;  // the counter only grows: every wave gets here
    const int utt = (int)(tile / (unsigned)tpu), ft = (int)(tile - (unsigned)utt * (unsigned)tpu);
    // An opaque per-tile copy of the lane id: without it the compiler hoists every lane-derived
    // address and predicate of the tile body out of this loop and pins ~40 VGPRs for the whole
    // kernel (172 -> 3 waves per SIMD become 2); recomputing them per tile is a few dozen VALU.
    int lane = lane_id;
    asm volatile("" : "+v"(lane));
    const int jf = lane & 15, g = lane >> 4;
    const int f0 = ft * TILE;
    int64_t off = (int64_t)utt * p.clip_stride;  // utt is wave-uniform: these are scalar loads
    if (p.offsets) off = p.offsets[utt];
    int len = p.clip_len;
    if (p.lengths) len = p.lengths[utt];
    const int T = len >= c.flen ? (len - c.flen) / c.stride : 0;  // processing.py:115-116 (Q3)
    if (f0 == 0 && lane == 0 && p.n_frames) p.n_frames[utt] = T < p.max_frames ? T : p.max_frames;
    int nvalid = T - f0;
    nvalid = nvalid > TILE ? TILE : nvalid;
    if (f0 + nvalid > p.max_frames) nvalid = p.max_frames - f0;
    float* out_rows = p.feat + ((int64_t)utt * p.max_frames + f0) * c.ncols;

    if (nvalid > 0) {
      const PcmT* x = reinterpret_cast<const PcmT*>(p.pcm) + off;
      const int need = (nvalid - 1) * c.stride + c.flen_eff;
      wave_sync();  // previous tile's readers of sig / ptile are done
      if (SVK_ABLATE(p, 1)) {
      } else if constexpr (RAW16)
        stage_raw16(c.preemph != 0, reinterpret_cast<const int16_t*>(x), (int64_t)f0 * c.stride, need, len, w.sigh, lane,
                    p.src_chunk ? p.src_chunk + (int64_t)utt * p.chunk_stride : nullptr, p.chunk, p.chunk_inv);
      else
        stage_span<PcmT>(p, x, (int64_t)f0 * c.stride, need, len, w.sig, lane);
      wave_sync();
      power_tile<SPLIT1024, RAW16, TILE>(c, w, tw, p.pre_cof, SVK_ABLATE(p, 2) ? 0 : nvalid, lane);
      wave_sync();

      if (SVK_ABLATE(p, 4)) continue;
      f32x4 acc[MAX_FT];
      mel_product<TILE>(c, p, w, lane, acc);
      const float e_frame = frame_energy<TILE>(c, w, p.escale, lane);
      if (SVK_ABLATE(p, 32)) continue;
      const bool row_ok = jf < nvalid;
      float* orow = out_rows + (int64_t)jf * c.ncols;
      log_mel<INT_PCM>(c, g, acc);
      if (c.out_kind != SVK_OUT_MFCC)
        store_filters(c, acc, orow, row_ok, g);
      else
        store_cepstra<INT_PCM>(c, p, w, acc, e_frame, orow, row_ok, lane);
      if (p.energy && row_ok && g == 0) p.energy[(int64_t)utt * p.max_frames + f0 + jf] = e_frame;
    }

    if (SVK_ABLATE(p, 64)) continue;
    zero_fill<TILE>(c, p, out_rows, utt, f0, nvalid, lane);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// plan: device tables derived on the host, once per configuration
// ---------------------------------------------------------------------------------
struct svk_frontend_plan {
  svk_frontend_cfg cfg;
  int device;
  int tile;        // frames per wave tile (8 or 16), chosen for residency
  void* d_tables;  // one allocation: tw1 | tw2 | tw3 | fbfrag | dctfrag
  // Every launch parameter that does not depend on the call (framing, kp, tiles of filters and cepstra, chunk ranges,
  // slots, table pointers and bytes, escale, n_steps, pre-emphasis), stated once; svk_frontend_run copies the record
  // and sets the rest.
  FrontendParams params;
};

namespace {

constexpr int GENERIC_WAVES = 12;  // 12 waves = 768 threads (SpecGeneric::MAX_THREADS): up to 168 VGPRs each

int env_int(const char* name, int fallback) {
  const char* v = getenv(name);
  return v ? atoi(v) : fallback;
}

// LDS carve: [shared tables] then per wave [staged samples | power tile [tile][kp + PT_PAD] | FFT scratch]
struct LdsLayout {
  int sig_bytes, wave_bytes, waves;
};
LdsLayout lds_layout(const FrontendParams& g, int tile, bool raw16, int lds_per_cu, int max_waves = GENERIC_WAVES) {
  const int span = (tile - 1) * g.stride + g.flen_eff;
  LdsLayout l;
  if (raw16)
    l.sig_bytes = (((RAW_OFF + span + 8) * 2 + 15) / 16) * 16;  // whole 16-byte groups per lane
  else
    l.sig_bytes = (((span + 8) * 4 + 15) / 16) * 16;
  const int prow = g.kp + PT_PAD;
  if (alias_scr(tile))  // scratch starts at row 4 of the power tile
    l.wave_bytes = l.sig_bytes + (int)sizeof(float) * std::max(tile * prow, 4 * prow + 2 * SCR);
  else
    l.wave_bytes = l.sig_bytes + (int)sizeof(float) * (tile * prow + 2 * SCR);
  l.wave_bytes = ((l.wave_bytes + 15) / 16) * 16;
  const int room = lds_per_cu - g.table_bytes;
  // an instance built for 1 024 threads (<= 128 VGPRs) may take 16 waves
  l.waves = room >= l.wave_bytes ? std::min(max_waves, room / l.wave_bytes) : 0;
  return l;
}

// The call-independent launch parameters but the table pointers, from the configuration and the filterbank alone
// (no HIP call).  -> the highest bin with a non-zero weight; above 256 the plan cannot be made and `g` is not complete.
int plan_geometry(const svk_frontend_cfg& cfg, const double* h_filterbank, FrontendParams& g) {
  const int nbins = cfg.nfft / 2 + 1;
  const int nf = cfg.num_filters;
  g.flen = cfg.frame_len;
  g.flen_eff = cfg.frame_len < cfg.nfft ? cfg.frame_len : cfg.nfft;
  g.stride = cfg.frame_stride;
  g.nfilt = nf;
  g.ncols = svk_frontend_num_cols(&cfg);
  g.out_kind = cfg.out_kind;
  g.dc_elim = cfg.dc_elimination;
  g.preemph = cfg.preemph;
  g.pre_shift = cfg.preemph_shift;
  g.pre_cof = cfg.preemph_cof;
  g.escale = cfg.input_scale != 0.f ? cfg.input_scale * cfg.input_scale : 1.0f;
  g.n_ft = (nf + 15) / 16;
  g.n_ct = cfg.out_kind == SVK_OUT_MFCC ? (cfg.num_ceps + 15) / 16 : 0;
  const int per = cfg.nfft == 1024 ? 128 : 64;
  g.n_steps = std::max(1, std::min(8, (g.flen_eff + per - 1) / per));

  // highest bin with a non-zero weight decides how many power bins are kept
  int kmax = -1;
  for (int i = 0; i < nf; ++i)
    for (int k = 0; k < nbins; ++k)
      if (h_filterbank[(size_t)i * nbins + k] != 0.0 && k > kmax) kmax = k;
  // bins 0..255 are the four 64-bin steps of the untangling; bin 256 (= nfft/4 of a 1024-point transform, where
  // SpeechPy's bank ends at every sampling rate but 16 kHz, Q2) costs a fifth, mostly idle step: kp = 288
  if (kmax > 256) return kmax;
  g.kp = ((kmax + 1 + 31) / 32) * 32;  // a multiple of 32 bins: the mel loop consumes chunks of 16 in pairs
  if (g.kp < 32) g.kp = 32;
  const int nchunks = g.kp / 16;
  g.n_slots = 0;
  for (int t = 0; t < MAX_FT; ++t) {
    int lo = nchunks, hi = 0;
    for (int i = 16 * t; i < 16 * t + 16 && i < nf; ++i)
      for (int k = 0; k < g.kp && k < nbins; ++k)
        if (h_filterbank[(size_t)i * nbins + k] != 0.0) {
          lo = std::min(lo, k / 16);
          hi = std::max(hi, k / 16 + 1);
        }
    if (hi <= lo) lo = hi = 0;
    if ((hi - lo) & 1) {  // pair up: take one more (all-zero) chunk on whichever side has room
      if (hi < nchunks) ++hi; else --lo;
    }
    g.chunk_lo[t] = lo;
    g.chunk_hi[t] = hi;
    g.slot_base[t] = g.n_slots;
    g.n_slots += hi - lo;
  }
  g.table_bytes = g.n_slots * 64 * (int)sizeof(f32x4) + g.n_ct * g.n_ft * 4 * 64 * (int)sizeof(float);
  g.table_bytes = ((g.table_bytes + 15) / 16) * 16 + 16;  // + the workgroup's tile counter
  return kmax;
}

// Tile size: 8 frames leave half of the MFMA N dimension idle but halve the per-wave LDS slice,
// i.e. double the waves a CU can hold.  SVK_FRONTEND_TILE=8|16 overrides (tuning).
int choose_tile(const FrontendParams& g, int lds_per_cu) {
  const int forced = env_int("SVK_FRONTEND_TILE", 0);
  if (forced == 8 || forced == 16) return forced;
  return lds_layout(g, 8, true, lds_per_cu).waves > lds_layout(g, 16, true, lds_per_cu).waves ? 8 : 16;
}

// Twiddles, filterbank fragments and DCT fragments (float64 maths, rounded once to f32) in one host vector:
// tw1 | tw2 | tw3 | fbfrag | dctfrag; off[] = where each starts, in floats.
std::vector<float> build_tables(const svk_frontend_cfg& cfg, const double* h_filterbank, const FrontendParams& g,
                                size_t (&off)[5]) {
  const int nbins = cfg.nfft / 2 + 1;
  const int nf = cfg.num_filters;
  const size_t n_tw = 2 * 8 * 64, n_tw3 = 2 * 5 * 64;
  const size_t n_fb = (size_t)std::max(g.n_slots, 1) * 64 * 4;
  const size_t n_dct = (size_t)std::max(g.n_ct, 1) * g.n_ft * 4 * 64;
  off[0] = 0, off[1] = n_tw, off[2] = 2 * n_tw, off[3] = 2 * n_tw + n_tw3, off[4] = off[3] + n_fb;
  std::vector<float> host(off[4] + n_dct, 0.f);
  float *h_tw1 = host.data() + off[0], *h_tw2 = host.data() + off[1], *h_tw3 = host.data() + off[2];
  float *h_fb = host.data() + off[3], *h_dct = host.data() + off[4];
  const double PI = 3.14159265358979323846;
  for (int r = 0; r < 8; ++r)
    for (int l = 0; l < 64; ++l) {
      double a1 = -2.0 * PI * (double)(l * r) / 512.0;
      double a2 = -2.0 * PI * (double)((l & 7) * r) / 64.0;
      h_tw1[2 * (r * 64 + l)] = (float)cos(a1);
      h_tw1[2 * (r * 64 + l) + 1] = (float)sin(a1);
      h_tw2[2 * (r * 64 + l)] = (float)cos(a2);
      h_tw2[2 * (r * 64 + l) + 1] = (float)sin(a2);
    }
  for (int q = 0; q < 5; ++q)
    for (int l = 0; l < 64; ++l) {
      double a = -2.0 * PI * (double)(l + 64 * q) / 1024.0;
      h_tw3[2 * (q * 64 + l)] = (float)cos(a);
      h_tw3[2 * (q * 64 + l) + 1] = (float)sin(a);
    }
  // input_scale (e.g. 2^-15: int16 PCM read the way librosa hands it to the reference's lmfe call,
  // load_data.py:50-70) enters every power as its square: folded into the weights, exact for powers of two
  const double in_scale = cfg.input_scale != 0.f ? (double)cfg.input_scale : 1.0;
  const double power_scale = (cfg.nfft == 1024 ? 1.0 / 4096.0 : 1.0 / 2048.0) * in_scale * in_scale;
  // A-operand fragments of the filterbank: lane l = (i = l & 15, kk = l >> 4), element e of
  // chunk u is fb[16 t + i][16 u + 4 kk + e]
  for (int t = 0; t < g.n_ft; ++t)
    for (int u = g.chunk_lo[t]; u < g.chunk_hi[t]; ++u)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) {
          const int filt = 16 * t + (l & 15), bin = 16 * u + 4 * (l >> 4) + e;
          double w = (filt < nf && bin < nbins) ? h_filterbank[(size_t)filt * nbins + bin] : 0.0;
          // the weights carry the spectrum's 1/nfft and the 1/4 of the untangling (powers of two: exact),
          // so the kernel stores raw |.|^2 sums in the power tile
          h_fb[(((size_t)g.slot_base[t] + (u - g.chunk_lo[t])) * 64 + l) * 4 + e] = (float)(w * power_scale);
        }
  // A-operand fragments of the DCT-II (ortho) matrix, k-step (t, r) <-> filter 16 t + 4 (l >> 4) + r
  // scipy.fftpack.dct(type=2, norm='ortho'): D[k][n] = sqrt(2/N) cos(pi k (2n+1) / 2N), D[0][n] = sqrt(1/N)
  for (int c = 0; c < g.n_ct; ++c)
    for (int t = 0; t < g.n_ft; ++t)
      for (int r = 0; r < 4; ++r)
        for (int l = 0; l < 64; ++l) {
          const int cep = 16 * c + (l & 15), filt = 16 * t + 4 * (l >> 4) + r;
          double d = 0.0;
          if (cep < cfg.num_ceps && filt < nf)
            d = cep == 0 ? sqrt(1.0 / nf) : sqrt(2.0 / nf) * cos(PI * cep * (2.0 * filt + 1.0) / (2.0 * nf));
          h_dct[(((size_t)c * g.n_ft + t) * 4 + r) * 64 + l] = (float)d;
        }
  return host;
}

typedef void (*frontend_fn)(const FrontendParams);

template <typename PcmT, bool RAW16>
frontend_fn pick_kernel(bool split, int tile) {
  if (split)
    return tile == 8 ? frontend_kernel<PcmT, true, 8, RAW16, SpecGeneric> : frontend_kernel<PcmT, true, 16, RAW16, SpecGeneric>;
  return tile == 8 ? frontend_kernel<PcmT, false, 8, RAW16, SpecGeneric> : frontend_kernel<PcmT, false, 16, RAW16, SpecGeneric>;
}

// Does the launch match every value a specialised instance has folded in?
template <typename Spec>
bool spec_matches(const FrontendParams& p) {
  return p.stride == Spec::STRIDE && p.flen == Spec::FLEN && p.flen_eff == Spec::FLEN && p.n_steps == Spec::N_STEPS &&
         (Spec::PRE < 0 || (p.preemph != 0) == (Spec::PRE != 0)) && (!p.preemph || p.pre_shift == 1) && p.kp == Spec::KP &&
         (p.need_energy != 0) == (Spec::NEED_ENERGY != 0) && p.n_ft == Spec::N_FT && p.n_ct == Spec::N_CT &&
         p.out_kind == Spec::OUT_KIND && p.nfilt == Spec::NFILT && p.ncols == Spec::NCOLS &&
         (Spec::OUT_KIND != SVK_OUT_MFCC || (p.dc_elim != 0) == (Spec::DC_ELIM != 0));
}

struct Instance {
  frontend_fn kernel;
  const char* name;  // what SVK_FE_DEBUG prints
  int wave_cap;      // waves per workgroup the instance is compiled for
};

// The instance for a launch: a specialised one when the tile is 8, the generic instance is not forced, the samples are
// staged the way it is built for (int16: raw) and the launch matches every folded value; else the generic one.
Instance pick_instance(const FrontendParams& p, bool f32_pcm, bool raw16, bool split, int tile, bool generic_only) {
  struct Specialised {
    bool f32_pcm, split;
    bool (*matches)(const FrontendParams&);
    Instance instance;
  };
  // float32 signals (what librosa hands the reference's lmfe call, load_data.py:50-70): the same two configurations.
  // Only the int16 MFCC instance is launched with the 1 024 threads it is compiled for (SpecMfcc13::MAX_THREADS).
  static const Specialised specialised[] = {
      {false, false, spec_matches<SpecMfcc13>,
       {frontend_kernel<int16_t, false, 8, true, SpecMfcc13>, "mfcc13", SpecMfcc13::MAX_THREADS / 64}},
      {false, true, spec_matches<SpecLmfe40>, {frontend_kernel<int16_t, true, 8, true, SpecLmfe40>, "lmfe40", GENERIC_WAVES}},
      {true, false, spec_matches<SpecMfcc13>, {frontend_kernel<float, false, 8, false, SpecMfcc13>, "mfcc13 (f32)", GENERIC_WAVES}},
      {true, true, spec_matches<SpecLmfe40>, {frontend_kernel<float, true, 8, false, SpecLmfe40>, "lmfe40 (f32)", GENERIC_WAVES}}};
  if (tile == 8 && !generic_only && (f32_pcm || raw16))
    for (const Specialised& s : specialised)
      if (s.f32_pcm == f32_pcm && s.split == split && s.matches(p)) return s.instance;
  const frontend_fn generic = f32_pcm ? pick_kernel<float, false>(split, tile)
                              : raw16 ? pick_kernel<int16_t, true>(split, tile)
                                      : pick_kernel<int16_t, false>(split, tile);
  return {generic, "generic", GENERIC_WAVES};
}

}  // namespace

extern "C" {

int64_t svk_frontend_num_frames(const svk_frontend_cfg* cfg, int64_t n_samples) {
  if (!cfg || cfg->frame_stride <= 0 || n_samples < cfg->frame_len) return 0;
  return (n_samples - cfg->frame_len) / cfg->frame_stride;
}

int svk_frontend_num_cols(const svk_frontend_cfg* cfg) {
  if (!cfg) return 0;
  return cfg->out_kind == SVK_OUT_MFCC ? cfg->num_ceps : cfg->num_filters;
}

int svk_frontend_plan_create(svk_ctx* ctx, const svk_frontend_cfg* cfg, const double* h_filterbank,
                             svk_frontend_plan** out) {
  if (!ctx || !cfg || !h_filterbank || !out) return SVK_ERR_BAD_ARG;
  *out = nullptr;
  SVK_REQUIRE(ctx, cfg->frame_len >= 1 && cfg->frame_stride >= 1, "frame_len / frame_stride must be >= 1");
  SVK_REQUIRE(ctx, cfg->num_filters >= 1, "num_filters must be >= 1");
  SVK_REQUIRE(ctx, cfg->out_kind >= SVK_OUT_MFE && cfg->out_kind <= SVK_OUT_MFCC, "out_kind");
  if (cfg->nfft != 512 && cfg->nfft != 1024)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "fused front end supports fft_length 512 or 1024, got %d", cfg->nfft);
  if (cfg->num_filters > 16 * MAX_FT)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "fused front end supports up to %d filters, got %d", 16 * MAX_FT,
                    cfg->num_filters);
  if (cfg->out_kind == SVK_OUT_MFCC)
    SVK_REQUIRE(ctx, cfg->num_ceps >= 1 && cfg->num_ceps <= cfg->num_filters, "1 <= num_ceps <= num_filters");

  // the one owner: every error exit below releases the plan and, once they exist, its device tables
  std::unique_ptr<svk_frontend_plan, void (*)(svk_frontend_plan*)> plan(new (std::nothrow) svk_frontend_plan(),
                                                                       svk_frontend_plan_destroy);
  if (!plan) return SVK_ERR_OOM;
  plan->cfg = *cfg;
  plan->device = ctx->device;
  FrontendParams& g = plan->params;
  const int kmax = plan_geometry(*cfg, h_filterbank, g);
  if (kmax > 256)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED,
                    "filterbank reaches bin %d; the fused kernel keeps bins <= 256 (the SpeechPy bank stops at "
                    "(nfft/2+2)/2, Q2)", kmax);
  plan->tile = choose_tile(g, ctx->lds_per_cu);
  if (lds_layout(g, plan->tile, false, ctx->lds_per_cu).waves < 1)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "frame stride %d / %d filters need more than %d bytes of LDS per CU",
                    cfg->frame_stride, cfg->num_filters, ctx->lds_per_cu);

  size_t off[5];
  const std::vector<float> host = build_tables(*cfg, h_filterbank, g, off);
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&plan->d_tables, host.size() * sizeof(float)) != hipSuccess)
    return svk_fail(ctx, SVK_ERR_HIP, "hipMalloc of front-end tables failed");
  if (hipMemcpy(plan->d_tables, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    return svk_fail(ctx, SVK_ERR_HIP, "upload of front-end tables failed");
  const float* d = reinterpret_cast<const float*>(plan->d_tables);
  g.tw1 = reinterpret_cast<const cplx*>(d + off[0]);
  g.tw2 = reinterpret_cast<const cplx*>(d + off[1]);
  g.tw3 = reinterpret_cast<const cplx*>(d + off[2]);
  g.fbfrag = reinterpret_cast<const f32x4*>(d + off[3]);
  g.dctfrag = d + off[4];
  *out = plan.release();
  return SVK_OK;
}

void svk_frontend_plan_destroy(svk_frontend_plan* plan) {
  if (!plan) return;
  if (plan->d_tables) (void)hipFree(plan->d_tables);
  delete plan;
}

int svk_frontend_run(svk_ctx* ctx, const svk_frontend_plan* plan, const void* d_pcm, int pcm_dtype,
                     const int64_t* d_offsets, const int32_t* d_lengths, int64_t clip_stride, int32_t clip_len,
                     int32_t n_utt, int32_t max_frames, float* d_feat, float* d_energy, int32_t* d_n_frames,
                     const int32_t* d_src_chunk, int32_t chunk_samples, int32_t chunk_stride) {
  if (!ctx || !plan) return SVK_ERR_BAD_ARG;
  SVK_REQUIRE(ctx, plan->device == ctx->device, "plan belongs to another device");
  SVK_REQUIRE(ctx, n_utt >= 0 && max_frames >= 0, "n_utt / max_frames negative");
  if (n_utt == 0 || max_frames == 0) return SVK_OK;
  SVK_REQUIRE(ctx, d_pcm && d_feat, "d_pcm / d_feat is NULL");
  SVK_REQUIRE(ctx, pcm_dtype == SVK_PCM_I16 || pcm_dtype == SVK_PCM_F32, "pcm_dtype");
  SVK_REQUIRE(ctx, d_offsets || clip_stride >= 0, "clip_stride negative");
  SVK_REQUIRE(ctx, d_lengths || clip_len >= 0, "clip_len negative");

  const bool raw16 = pcm_dtype == SVK_PCM_I16 && (!plan->cfg.preemph || plan->cfg.preemph_shift == 1) &&
                     !env_int("SVK_FE_F32STAGE", 0);
  if (d_src_chunk) {
    SVK_REQUIRE(ctx, (int64_t)chunk_samples * chunk_stride < ((int64_t)1 << 24), "gathered clips of at most 2^24 samples");
    SVK_REQUIRE(ctx, d_lengths, "gathered input needs d_lengths (the gathered length of every clip)");
    if (!raw16 || chunk_samples < 8 || (chunk_samples & 7) || chunk_stride < 0)
      return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "gathered input (d_src_chunk) is built for int16 PCM through the 16-bit staging path "
                      "and chunks of a multiple of 8 samples (got dtype %d, chunk %d)", pcm_dtype, chunk_samples);
  }
  FrontendParams p = plan->params;  // the plan's part; what follows is the call's
  p.pcm = d_pcm;
  p.offsets = d_offsets;
  p.lengths = d_lengths;
  p.clip_stride = clip_stride;
  p.clip_len = clip_len;
  p.src_chunk = d_src_chunk;
  p.chunk = chunk_samples;
  p.chunk_stride = chunk_stride;
  p.chunk_inv = chunk_samples > 0 ? 1.0f / (float)chunk_samples : 0.f;
  p.n_utt = n_utt;
  p.max_frames = max_frames;
  p.tiles_per_utt = (max_frames + plan->tile - 1) / plan->tile;
  p.feat = d_feat;
  p.energy = d_energy;
  p.n_frames = d_n_frames;
  p.need_energy = (d_energy != nullptr) || (plan->cfg.out_kind == SVK_OUT_MFCC && plan->cfg.dc_elimination);
  p.ablate = env_int("SVK_FE_ABLATE", 0);

  const int64_t total = (int64_t)n_utt * p.tiles_per_utt;
  if (total >= ((int64_t)1 << 31))
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "%lld frame tiles in one launch (limit 2^31): split the batch",
                    (long long)total);
  const bool generic_only = getenv("SVK_FE_GENERIC") != nullptr;  // tuning / tests: force the unspecialised instance
  const Instance inst = pick_instance(p, pcm_dtype == SVK_PCM_F32, raw16, plan->cfg.nfft == 1024, plan->tile, generic_only);
  const LdsLayout lds = lds_layout(p, plan->tile, raw16, ctx->lds_per_cu, inst.wave_cap);
  p.sig_bytes = lds.sig_bytes;
  p.wave_bytes = lds.wave_bytes;
  // one workgroup of that many waves per CU (it owns the CU's LDS); fewer when there is little work
  int waves = (int)std::max<int64_t>(1, std::min<int64_t>(lds.waves, (total + ctx->num_cu - 1) / ctx->num_cu));
  waves = std::max(1, std::min(waves, env_int("SVK_FE_WAVES", waves)));  // tuning only
  const int64_t grid = std::min<int64_t>((total + waves - 1) / waves, ctx->num_cu);
  const size_t lds_total = (size_t)p.table_bytes + (size_t)waves * lds.wave_bytes;
  if (getenv("SVK_FE_DEBUG"))
    fprintf(stderr, "svk_frontend_run: %s instance, %d waves/CU, grid %lld\n", inst.name, waves, (long long)grid);
  SVK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(inst.kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_total));
  hipLaunchKernelGGL(inst.kernel, dim3((unsigned)grid), dim3(64 * waves), lds_total, ctx->stream, p);
  SVK_LAUNCH_CHECK(ctx);
  return SVK_OK;
}

}  // extern "C"
