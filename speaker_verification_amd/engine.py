"""Device engine: the thin host layer between Python callers and libsvk.so.

One `Engine` per process and GPU.  torch supplies device memory and streams
(plumbing); every computation below is a hand-written gfx950 kernel reached
through the C-ABI.  Methods take torch CUDA tensors (zero-copy) or NumPy arrays
(uploaded) and return torch CUDA tensors; the drop-in modules
(`speechpy/`, `vad.py`, `evaluation.py`, `siamese.py`) convert to the
reference's NumPy return types.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import FrontendCfg, check


def _torch():
    import torch
    return torch


class FrontendSpec:
    """Hashable description of one front-end configuration (SURVEY.md section 5:
    'a small frozen FrontEndConfig')."""

    __slots__ = ("fs", "frame_len", "frame_stride", "nfft", "num_filters", "num_ceps", "out_kind",
                 "dc_elimination", "low_freq", "high_freq", "preemph", "preemph_shift", "preemph_cof",
                 "input_scale")

    def __init__(self, fs, frame_len, frame_stride, nfft, num_filters, num_ceps, out_kind,
                 dc_elimination=True, low_freq=0, high_freq=None, preemph=False, preemph_shift=1,
                 preemph_cof=0.98, input_scale=1.0):
        """input_scale: amplitude factor applied to the PCM before anything else (1/32768 reads int16
        PCM as the float signal librosa.load hands the reference's lmfe call, load_data.py:50-70)."""
        self.input_scale = float(input_scale)
        self.fs, self.frame_len, self.frame_stride, self.nfft = fs, int(frame_len), int(frame_stride), int(nfft)
        self.num_filters, self.num_ceps, self.out_kind = int(num_filters), int(num_ceps), int(out_kind)
        self.dc_elimination, self.low_freq, self.high_freq = bool(dc_elimination), low_freq, high_freq
        self.preemph, self.preemph_shift, self.preemph_cof = bool(preemph), int(preemph_shift), float(preemph_cof)

    def key(self):
        return tuple(getattr(self, s) for s in self.__slots__)

    @property
    def num_cols(self):
        return self.num_ceps if self.out_kind == _lib.OUT_MFCC else self.num_filters

    def num_frames(self, n_samples):
        """floor((L - flen) / stride), never negative (processing.py:115-116, Q3)."""
        return max(0, int(math.floor((n_samples - self.frame_len) / float(self.frame_stride)))) \
            if n_samples >= self.frame_len else 0

    def c_struct(self):
        return FrontendCfg(self.frame_len, self.frame_stride, self.nfft, self.num_filters,
                           max(1, self.num_ceps), self.out_kind, int(self.dc_elimination), int(self.preemph),
                           self.preemph_shift, self.preemph_cof, self.input_scale)


def spec_from_seconds(fs, frame_length, frame_stride, nfft, num_filters, num_ceps, out_kind, **kw):
    """frame sizes as the reference derives them (processing.py:94-98)."""
    flen = int(np.round(fs * frame_length))
    stride = int(float(np.round(fs * frame_stride)))
    return FrontendSpec(fs, flen, stride, nfft, num_filters, num_ceps, out_kind, **kw)


def split_step(n, k):
    """Pairs per split of get_and_plot_k_eer_auc (evaluation.py:13, `int(n / float(k))`): n // k, the same number for
    every n < 2^53 (svk_roc_k computes it so); the last n - k * step pairs belong to no split."""
    return int(n) // int(k)


class Engine:
    def __init__(self, device=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("speaker_verification_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        handle = C.c_void_p()
        check(self.lib.svk_create(self.device_index, C.byref(handle)))
        self.ctx = handle
        self._plans = {}
        info = (C.c_int64 * 4)()
        check(self.lib.svk_device_info(self.ctx, info), self.ctx)
        self.num_cu, self.clock_khz, self.lds_per_cu, self.wave = (int(v) for v in info)

    def __del__(self):
        try:
            for hit in self._plans.values():
                if not isinstance(hit, str):
                    self.lib.svk_frontend_plan_destroy(hit[0])
            if self.ctx:
                self.lib.svk_destroy(self.ctx)
        except Exception:
            pass

    # ---- plumbing -----------------------------------------------------------
    def _stream(self):
        torch = _torch()
        stream = torch.cuda.current_stream(self.device)
        check(self.lib.svk_set_stream(self.ctx, C.c_void_p(stream.cuda_stream)), self.ctx)

    def to_device(self, x, dtype=None):
        """torch CUDA tensor (contiguous) from a NumPy array / tensor."""
        torch = _torch()
        if isinstance(x, torch.Tensor):
            t = x.to(self.device)
        else:
            x = np.ascontiguousarray(x)
            if not x.flags.writeable:            # e.g. np.frombuffer views: torch wants a writable array
                x = x.copy()
            t = torch.from_numpy(x).to(self.device)
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.contiguous()

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    # ---- argument rules, each stated once ------------------------------------------------------------------------
    def _frames(self, n_frames):
        """Per-clip counts (frames, samples) as int32 on the device, or None."""
        return self.to_device(n_frames, _torch().int32) if n_frames is not None else None

    def _workspace(self, nbytes):
        """A workspace sized by the library (svk_*_workspace_bytes): a torch allocation of at least 16 bytes, so that its
        pointer is never NULL; every entry accepts a larger workspace than it asks for."""
        return _torch().empty((max(16, int(nbytes)),), dtype=_torch().uint8, device=self.device)

    def _given_out(self, out, shape, dtype, what):
        """A caller-supplied output: a contiguous device tensor of that dtype and shape (an int: that many elements)."""
        ok = isinstance(out, _torch().Tensor) and out.is_cuda and out.dtype == dtype and out.is_contiguous() and \
            (out.numel() == shape if isinstance(shape, int) else tuple(out.shape) == tuple(shape))
        if not ok:
            raise ValueError(what)

    def _labels01(self, labels, n):
        """0/1 labels as uint8 [n] on the device (anything non-zero is a target)."""
        torch = _torch()
        lb = self.to_device(labels).reshape(-1)
        lb = (lb != 0).to(torch.uint8) if lb.dtype != torch.uint8 else lb
        if lb.numel() != n:
            raise ValueError("scores and labels differ in length")
        return lb

    def _scores_labels(self, scores, labels):
        sc = self.to_device(scores, _torch().float32).reshape(-1)
        return sc, self._labels01(labels, sc.numel())

    def _two_matrices(self, a, b, who):
        """Two float32 matrices (Na, D) and (Nb, D) on the device; `b is a` stays one tensor."""
        f32 = _torch().float32
        x = self.to_device(a, f32)
        y = x if b is a else self.to_device(b, f32)
        if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
            raise ValueError("%s wants (Na, D) and (Nb, D)" % who)
        return x, y

    def _counter(self, t, name):
        """An optional int32 device counter (the caller zeroes it)."""
        torch = _torch()
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() >= 1):
            raise ValueError("%s must be an int32 device tensor" % name)
        return t

    def _trials(self, idx_a, idx_b, bad_count):
        """The two index lists of a trial list as int64 on the device, and its bad-index counter."""
        i64 = _torch().int64
        ia, ib = self.to_device(idx_a, i64).reshape(-1), self.to_device(idx_b, i64).reshape(-1)
        if ia.numel() != ib.numel():
            raise ValueError("idx_a and idx_b differ in length")
        return ia, ib, self._counter(bad_count, "bad_count")

    def _row_index(self, row_index, n_rows):
        """The optional row permutation of the grouped entries as int64 [n_rows] on the device."""
        if row_index is None:
            return None
        index = self.to_device(row_index, _torch().int64).reshape(-1)
        if index.numel() != n_rows:
            raise ValueError("row_index holds one entry per row of emb")
        return index

    def _segments(self, seg_start, row_index, n_rows):
        """CSR groups of rows: seg_start int64 [n_seg + 1] and the optional row_index on the device."""
        start = self.to_device(seg_start, _torch().int64).reshape(-1)
        if start.numel() < 1:
            raise ValueError("seg_start holds n_seg + 1 offsets")
        return start, self._row_index(row_index, n_rows)

    def synchronize(self):
        check(self.lib.svk_sync(self.ctx), self.ctx)

    # ---- fused front end -------------------------------------------------------
    def plan(self, spec):
        from .speechpy import feature as _feature
        key = spec.key()
        hit = self._plans.get(key)
        if isinstance(hit, str):                 # a configuration the fused kernel refused before: a FRESH exception
            raise _lib.SvkError(_lib.SVK_ERR_UNSUPPORTED, hit)   # each time (a cached one would chain every caller's
        if hit is None:                                          # traceback -- and its frames' inputs -- forever)
            bank = np.ascontiguousarray(
                _feature.filterbanks(spec.num_filters, spec.nfft // 2 + 1, spec.fs, spec.low_freq,
                                     spec.high_freq or spec.fs / 2), dtype=np.float64)
            cfg = spec.c_struct()
            handle = C.c_void_p()
            try:
                check(self.lib.svk_frontend_plan_create(self.ctx, C.byref(cfg),
                                                        bank.ctypes.data_as(C.POINTER(C.c_double)),
                                                        C.byref(handle)), self.ctx)
            except _lib.SvkError as err:
                if err.code == _lib.SVK_ERR_UNSUPPORTED:
                    self._plans[key] = err.message or "unsupported front-end configuration"
                raise
            hit = (handle, cfg)
            self._plans[key] = hit
        return hit

    def features(self, pcm, spec, lengths=None, offsets=None, clip_len=None, max_frames=None,
                 want_energy=False, gather=None):
        """Batched front end.

        pcm     : [n_utt, L] (uniform clips) or, with `offsets`, a 1-D concatenation;
                  int16 or float32, NumPy or CUDA tensor
        lengths : optional [n_utt] int32 samples per clip (device or host)
        gather  : (src_frame [n_utt, F] i32, frame_samples) of vad_energy(..., compact="index"): the clips' VOICED frames
                  are read where they lie in `pcm` (lengths = voiced_len), nothing was copied (int16 PCM, fused kernel only)
        returns (feat [n_utt, max_frames, cols] f32, n_frames [n_utt] i32, energy or None)
        """
        torch = _torch()
        try:
            handle, _ = self.plan(spec)
        except _lib.SvkError as err:
            if err.code != _lib.SVK_ERR_UNSUPPORTED or gather is not None:
                raise
            # what the fused kernel does not cover (other fft lengths, > 64 filters, a bank past bin
            # nfft/4 of 1024 or nfft/2 of 512, frames too long for a CU's LDS): the same stages as
            # separate kernels, clip by clip
            return self._features_staged(pcm, spec, lengths, offsets, clip_len, max_frames, want_energy)
        pcm = self.to_device(pcm)
        if pcm.dtype == torch.int16:
            kind = _lib.PCM_I16
        else:
            pcm = pcm.to(torch.float32) if pcm.dtype != torch.float32 else pcm
            kind = _lib.PCM_F32
        if lengths is not None:
            lengths = self.to_device(lengths, torch.int32)
        if offsets is not None:
            if lengths is None:
                raise ValueError("offsets need lengths")
            offsets = self.to_device(offsets, torch.int64)
            n_utt, stride, length = offsets.numel(), 0, 0
            # (a device-side max would be a host round trip per batch: only when the caller did not size the output)
            longest = (int(lengths.max().item()) if n_utt else 0) if max_frames is None else 0
        else:
            if pcm.dim() == 1:
                pcm = pcm[None]
            n_utt, stride = pcm.shape[0], pcm.shape[1]
            length = stride if clip_len is None else int(clip_len)
            longest = length
        if max_frames is None:
            max_frames = spec.num_frames(longest)
        cols = spec.num_cols
        feat = torch.empty((n_utt, max_frames, cols), dtype=torch.float32, device=self.device)
        n_frames = torch.empty((n_utt,), dtype=torch.int32, device=self.device)
        energy = torch.empty((n_utt, max_frames), dtype=torch.float32, device=self.device) if want_energy else None
        src, chunk, cstride = None, 0, 0
        if gather is not None:
            src, chunk = gather
            if lengths is None or src.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != n_utt or not src.is_contiguous():
                raise ValueError("gather wants (src_frame [n_utt, F] int32, frame_samples) and the voiced lengths")
            cstride = int(src.shape[1])
        self._stream()
        check(self.lib.svk_frontend_run(self.ctx, handle, self._ptr(pcm), kind, self._ptr(offsets),
                                        self._ptr(lengths), stride, length, n_utt, max_frames,
                                        self._ptr(feat), self._ptr(energy), self._ptr(n_frames),
                                        self._ptr(src), int(chunk), cstride), self.ctx)
        return feat, n_frames, energy

    def _features_staged(self, pcm, spec, lengths, offsets, clip_len, max_frames, want_energy):
        """`features` for any configuration: svk_preemphasis -> svk_stack_frames -> svk_spectrum ->
        svk_mel_features per clip (feature.py:156-219 stage by stage).  Same outputs and layout."""
        torch = _torch()
        from .speechpy import feature as _feature
        pcm = self.to_device(pcm)
        if pcm.dtype not in (torch.int16, torch.float32):
            pcm = pcm.to(torch.float32)
        if offsets is not None:
            if lengths is None:
                raise ValueError("offsets need lengths")
            offs = [int(v) for v in torch.as_tensor(offsets).cpu().tolist()]
            lens = [int(v) for v in torch.as_tensor(lengths).cpu().tolist()]
            clips = [pcm.reshape(-1)[o:o + n] for o, n in zip(offs, lens)]
        else:
            if pcm.dim() == 1:
                pcm = pcm[None]
            full = pcm.shape[1] if clip_len is None else int(clip_len)
            lens = [full] * pcm.shape[0] if lengths is None else \
                [int(v) for v in torch.as_tensor(lengths).cpu().tolist()]
            clips = [pcm[i, :n] for i, n in enumerate(lens)]
        if max_frames is None:
            max_frames = spec.num_frames(max(lens) if lens else 0)
        bank = _feature.filterbanks(spec.num_filters, spec.nfft // 2 + 1, spec.fs, spec.low_freq,
                                    spec.high_freq or spec.fs / 2)
        bank_dev = self.to_device(bank, torch.float32)
        cols = spec.num_cols
        feat = torch.zeros((len(clips), max_frames, cols), dtype=torch.float32, device=self.device)
        n_frames = torch.zeros((len(clips),), dtype=torch.int32)
        energy = torch.zeros((len(clips), max_frames), dtype=torch.float32, device=self.device) if want_energy else None
        for i, clip in enumerate(clips):
            T = min(spec.num_frames(int(clip.numel())), max_frames)
            n_frames[i] = T
            if T <= 0:
                continue
            sig = self.preemphasis(clip, spec.preemph_shift, spec.preemph_cof) if spec.preemph else clip.to(torch.float32)
            if spec.input_scale != 1.0:
                sig = sig * spec.input_scale
            frames = self.stack_frames(sig, spec.frame_len, spec.frame_stride, T)
            power = self.spectrum(frames, spec.nfft, power=True)
            f, e = self.mel_features(power, bank_dev, spec.out_kind, spec.num_ceps, spec.dc_elimination, want_energy)
            feat[i, :T] = f
            if want_energy:
                energy[i, :T] = e
        return feat, n_frames.to(self.device), energy

    # ---- stage-level kernels ------------------------------------------------------
    def preemphasis(self, signal, shift=1, cof=0.98):
        torch = _torch()
        x = self.to_device(signal)
        if x.dtype == torch.int16:
            kind = _lib.PCM_I16
        else:
            x = x.to(torch.float32)
            kind = _lib.PCM_F32
        out = torch.empty(x.shape, dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_preemphasis(self.ctx, self._ptr(x), kind, x.numel(), int(shift), float(cof),
                                       self._ptr(out)), self.ctx)
        return out

    def stack_frames(self, sig, frame_len, stride, n_frames, window=None):
        torch = _torch()
        x = self.to_device(sig, torch.float32)
        win = self.to_device(window, torch.float32) if window is not None else None
        out = torch.empty((max(n_frames, 0), frame_len), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_stack_frames(self.ctx, self._ptr(x), x.numel(), int(frame_len), int(stride),
                                        int(max(n_frames, 0)), self._ptr(win), self._ptr(out)), self.ctx)
        return out

    def spectrum(self, frames, nfft, power):
        torch = _torch()
        fr = self.to_device(frames, torch.float32)
        if fr.dim() != 2:
            raise ValueError("frames must be (num_frames, frame_len)")
        out = torch.empty((fr.shape[0], nfft // 2 + 1), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_spectrum(self.ctx, self._ptr(fr), fr.shape[0], fr.shape[1], int(nfft), int(bool(power)),
                                    self._ptr(out)), self.ctx)
        return out

    def cmvn_(self, feat, n_frames=None, variance=False):
        """In place on feat [n_utt, max_frames, cols] (or [rows, cols] = one clip)."""
        torch = _torch()
        if not (isinstance(feat, torch.Tensor) and feat.is_cuda and feat.dtype == torch.float32
                and feat.is_contiguous()):
            raise ValueError("cmvn_ works in place on a contiguous float32 CUDA tensor")
        shape = feat.shape if feat.dim() == 3 else (1,) + tuple(feat.shape)
        nf = self._frames(n_frames)
        self._stream()
        check(self.lib.svk_cmvn(self.ctx, self._ptr(feat), shape[0], shape[1], shape[2], self._ptr(nf),
                                int(bool(variance))), self.ctx)
        return feat

    def cmvn_stats(self, feat, n_frames=None, variance=False):
        """svk_cmvn_stats: per-clip mean and 1 / (std + 2^-30) of feat [n_utt, max_frames, cols] as float64 [n_utt, 2, cols],
        without touching feat (cube_gather(..., stats=...) applies them to the rows it copies)."""
        torch = _torch()
        if not (isinstance(feat, torch.Tensor) and feat.is_cuda and feat.dtype == torch.float32 and feat.is_contiguous()
                and feat.dim() == 3):
            raise ValueError("cmvn_stats wants a contiguous float32 CUDA tensor [n_utt, max_frames, cols]")
        nf = self._frames(n_frames)
        stats = torch.zeros((feat.shape[0], 2, feat.shape[2]), dtype=torch.float64, device=self.device)
        self._stream()
        check(self.lib.svk_cmvn_stats(self.ctx, self._ptr(feat), feat.shape[0], feat.shape[1], feat.shape[2], self._ptr(nf),
                                      int(bool(variance)), self._ptr(stats)), self.ctx)
        return stats

    def _static_rows(self, feat, who):
        feat = self.to_device(feat, _torch().float32)
        if feat.dim() != 3:
            raise ValueError("%s wants static features [n_utt, max_frames, cols]" % who)
        return feat

    def _stats3(self, stats, n, cols):
        torch = _torch()
        if stats is not None and (not isinstance(stats, torch.Tensor) or stats.dtype != torch.float64 or not stats.is_cuda
                                  or tuple(stats.shape) != (n, 3, 2, cols) or not stats.is_contiguous()):
            raise ValueError("stats must be the float64 [n, 3, 2, cols] tensor of delta_cmvn_stats")
        return stats

    def delta_cmvn_stats(self, feat, n_frames=None, delta=2, variance=False):
        """svk_delta_cmvn_stats: the CMVN statistics of the three channels (static, delta, delta-delta: feature.py:261-282)
        of STATIC features [n_utt, max_frames, cols], one pass, as float64 [n_utt, 3, 2, cols] (mean, 1 / (std + 2^-30));
        [:, ch] is bit-identical to cmvn_stats of plane ch.  delta_planes / cube_gather_delta(..., stats=...) apply them."""
        torch = _torch()
        feat = self._static_rows(feat, "delta_cmvn_stats")
        nf = self._frames(n_frames)
        stats = torch.zeros((feat.shape[0], 3, 2, feat.shape[2]), dtype=torch.float64, device=self.device)
        self._stream()
        check(self.lib.svk_delta_cmvn_stats(self.ctx, self._ptr(feat), feat.shape[0], feat.shape[1], feat.shape[2], self._ptr(nf),
                                            int(delta), int(bool(variance)), self._ptr(stats)), self.ctx)
        return stats

    def delta_planes(self, feat, n_frames=None, delta=2, stats=None, out=None):
        """svk_delta_planes: STATIC features [n, T, C] -> [n, 3, T, C] (static, derivative, derivative of the derivative: the
        feature rows svk_c3d2_stage1_c3 reads), CMVN-normalised per channel with `stats` (delta_cmvn_stats); rows at or past
        n_frames are zeros."""
        torch = _torch()
        feat = self._static_rows(feat, "delta_planes")
        n, T, Cc = feat.shape
        nf = self._frames(n_frames)
        stats = self._stats3(stats, n, Cc)
        if out is None:
            out = torch.empty((n, 3, T, Cc), dtype=torch.float32, device=self.device)
        else:
            self._given_out(out, (n, 3, T, Cc), torch.float32, "out must be a contiguous float32 CUDA tensor [n, 3, max_frames, cols]")
        self._stream()
        check(self.lib.svk_delta_planes(self.ctx, self._ptr(feat), n, T, Cc, self._ptr(nf), int(delta), self._ptr(stats),
                                        self._ptr(out)), self.ctx)
        return out

    def mel_features(self, power, bank, out_kind, num_ceps=13, dc_elimination=True, want_energy=False):
        """General mel / log / DCT stage on a device power spectrum [T, bins] (any fft length)."""
        torch = _torch()
        p = self.to_device(power, torch.float32)
        b = self.to_device(bank, torch.float32)
        T, bins = p.shape
        nf = b.shape[0]
        cols = num_ceps if out_kind == _lib.OUT_MFCC else nf
        feat = torch.empty((T, cols), dtype=torch.float32, device=self.device)
        energy = torch.empty((T,), dtype=torch.float32, device=self.device) if want_energy else None
        self._stream()
        check(self.lib.svk_mel_features(self.ctx, self._ptr(p), T, bins, self._ptr(b), nf, int(out_kind),
                                        int(num_ceps), int(bool(dc_elimination)), self._ptr(feat),
                                        self._ptr(energy)), self.ctx)
        return feat, energy

    def cmvnw(self, feat, win_size=301, variance=False, n_frames=None):
        """Sliding-window CMVN of feat [n_utt, max_frames, cols] (or [rows, cols]); returns a new tensor."""
        torch = _torch()
        x = self.to_device(feat, torch.float32)
        shape = x.shape if x.dim() == 3 else (1,) + tuple(x.shape)
        nf = self._frames(n_frames)
        out = x.clone()                         # rows past n_frames keep the input
        tmp = torch.empty_like(x) if variance else None
        self._stream()
        check(self.lib.svk_cmvnw(self.ctx, self._ptr(x), shape[0], shape[1], shape[2], self._ptr(nf), int(win_size),
                                 int(bool(variance)), self._ptr(tmp), self._ptr(out)), self.ctx)
        return out

    def derivative(self, feat, delta):
        torch = _torch()
        x = self.to_device(feat, torch.float32)
        out = torch.empty_like(x)
        self._stream()
        check(self.lib.svk_derivative(self.ctx, self._ptr(x), x.numel() // x.shape[-1], x.shape[-1], int(delta),
                                      self._ptr(out)), self.ctx)
        return out

    def log_power_(self, power, normalize=True):
        """In place: 10 log10(max(p, 1e-20)) [- global max]."""
        self._stream()
        check(self.lib.svk_log_power(self.ctx, self._ptr(power), power.numel(), int(bool(normalize))), self.ctx)
        return power

    def _vad_call(self, pcm, fs, frame_ms, padding_ms, lengths, compact, want_segments, frame_samples, ring_len, offsets,
                  voiced_out, longest):
        """What the two VAD entries share: geometry, output sizing and allocation.  -> (head, tail, result, max_vf, inputs): the
        C-ABI arguments in front of the rule's parameters (pcm .. ring_thresh) and behind max_vad_frames (d_keep .. d_src_frame),
        the dict of outputs, and the device inputs `head` points into (the caller holds them until the launch is queued)."""
        torch = _torch()
        x = self.to_device(pcm)
        if x.dtype != torch.int16:
            raise TypeError("VAD works on int16 PCM (vad.py:16-17 asserts 16-bit mono)")
        fsamp = int(frame_samples) if frame_samples else int(fs * (frame_ms / 1000.0) * 2) // 2   # vad.py:50
        ring_len = int(ring_len) if ring_len else int(padding_ms / frame_ms)                       # vad.py:81
        ring_thresh = int(math.floor(0.9 * ring_len))                    # count > 0.9 * maxlen, vad.py:99,117
        lens = self._frames(lengths)
        if offsets is not None:
            if lens is None:
                raise ValueError("offsets need lengths")
            offs = self.to_device(offsets, torch.int64)
            n_utt, stride = offs.numel(), 0
            if longest is not None:
                longest = int(longest)
            elif not n_utt:
                longest = 0
            elif isinstance(lengths, np.ndarray):          # host lengths: no device round trip
                longest = int(lengths.max())
            else:
                longest = int(lens.max().item())
        else:
            offs = None
            if x.dim() == 1:
                x = x[None]
            n_utt, stride = x.shape
            longest = stride
        max_vf = max(1, (2 * longest - 1) // (2 * fsamp)) if longest > 0 else 1
        keep = torch.empty((n_utt, max_vf), dtype=torch.uint8, device=self.device)
        nvf = torch.empty((n_utt,), dtype=torch.int32, device=self.device)
        seg = torch.empty((n_utt, max_vf), dtype=torch.int32, device=self.device) if want_segments else None
        # only [:voiced_len] of a clip is defined (no 98 MB memset); `voiced_out`: a caller-owned buffer of pcm's shape,
        # reused across batches that address ONE resident concatenation through offsets
        index = compact == "index"
        if index:
            voiced = None
        elif compact and voiced_out is not None:
            if voiced_out.shape != x.shape or voiced_out.dtype != torch.int16 or not voiced_out.is_contiguous():
                raise ValueError("voiced_out must be a contiguous int16 tensor of pcm's shape")
            voiced = voiced_out
        else:
            voiced = torch.empty_like(x) if compact else None
        vlen = torch.empty((n_utt,), dtype=torch.int32, device=self.device) if compact else None
        src = torch.empty((n_utt, max_vf), dtype=torch.int32, device=self.device) if index else None
        head = (self._ptr(x), self._ptr(offs), self._ptr(lens), stride, longest, n_utt, fsamp, ring_len, ring_thresh)
        tail = (self._ptr(keep), self._ptr(seg), self._ptr(nvf), self._ptr(voiced), self._ptr(vlen), self._ptr(src))
        res = {"keep": keep, "n_vad_frames": nvf, "voiced": voiced, "voiced_len": vlen, "seg": seg,
               "frame_samples": fsamp, "src_frame": src}
        return head, tail, res, max_vf, (x, offs, lens)

    def vad_energy(self, pcm, threshold, fs=16000, frame_ms=30, padding_ms=300, lengths=None, compact=True,
                   want_segments=False, frame_samples=None, ring_len=None, offsets=None, voiced_out=None, longest=None):
        """pcm [n_utt, L] int16 (or, with `offsets` + `lengths`, a 1-D concatenation of ragged clips) ->
        dict(keep [n, F] u8, n_vad_frames [n] i32, voiced (same layout as pcm; a clip's samples past its
        voiced_len are unspecified) i16, voiced_len [n] i32, seg [n, F] i32, src_frame).  compact=True copies the kept
        frames to the front of `voiced`; compact="index" copies nothing and returns src_frame [n, F] i32 instead (entry q =
        the q-th kept frame: `features(pcm, ..., lengths=voiced_len, gather=(src_frame, frame_samples))` reads through it).  `longest`: the longest clip in samples when
        the caller knows it (device-side lengths would otherwise cost a host round trip to size the outputs)."""
        head, tail, res, max_vf, _inputs = self._vad_call(pcm, fs, frame_ms, padding_ms, lengths, compact, want_segments,
                                                          frame_samples, ring_len, offsets, voiced_out, longest)
        self._stream()
        check(self.lib.svk_vad_energy(self.ctx, *head, int(threshold), max_vf, *tail), self.ctx)
        return res

    def vad_adaptive(self, pcm, vad, fs=16000, frame_ms=30, padding_ms=300, lengths=None, compact=True,
                     want_segments=False, frame_samples=None, ring_len=None, offsets=None, voiced_out=None, longest=None,
                     want_energy=False):
        """`vad_energy` under the level-adaptive rule (svk_vad_adaptive, include/svk.h "level-adaptive energy VAD"): `vad` is a `vad.AdaptiveEnergyVad`
        (anything with its five integer attributes floor_q16, peak_q16, above_floor_q16, below_peak_q16, min_threshold).  The
        same arguments and the same dict, plus levels [n, 3] i64 = (E_lo, E_hi, T) per clip and, with want_energy, energy
        [n, F] i64 (a clip's entries from its frame count on are unspecified)."""
        torch = _torch()
        head, tail, res, max_vf, _inputs = self._vad_call(pcm, fs, frame_ms, padding_ms, lengths, compact, want_segments,
                                                          frame_samples, ring_len, offsets, voiced_out, longest)
        n_utt = head[5]
        levels = torch.empty((n_utt, 3), dtype=torch.int64, device=self.device)
        energy = torch.empty((n_utt, max_vf), dtype=torch.int64, device=self.device) if want_energy else None
        self._stream()
        check(self.lib.svk_vad_adaptive(self.ctx, *head, int(vad.floor_q16), int(vad.peak_q16), int(vad.above_floor_q16),
                                        int(vad.below_peak_q16), int(vad.min_threshold), max_vf, *tail, self._ptr(levels),
                                        self._ptr(energy)), self.ctx)
        res["levels"] = levels
        if want_energy:
            res["energy"] = energy
        return res

    def draw_crops(self, n_frames, n_crops=20, crop_frames=80, seed=12345, first_utt=0, bad_count=None,
                   utt_index=None):
        """[n] i32 frame counts (device) -> [n, n_crops] i32 crop starts drawn on the device, keyed by
        the clip's global index: `utt_index[u]` if given, else first_utt + u."""
        torch = _torch()
        nf = self.to_device(n_frames, torch.int32)
        gi = self.to_device(utt_index, torch.int64) if utt_index is not None else None
        idx = torch.empty((nf.numel(), n_crops), dtype=torch.int32, device=self.device)
        self._stream()
        check(self.lib.svk_cube_draw_crops(self.ctx, self._ptr(nf), nf.numel(), int(first_utt), self._ptr(gi), n_crops,
                                           crop_frames, int(seed) & 0xFFFFFFFFFFFFFFFF, self._ptr(idx),
                                           self._ptr(bad_count)), self.ctx)
        return idx

    def cube_gather(self, feat, crop_idx, crop_frames=80, out=None, stats=None):
        """feat [n, T, C] + crop_idx [n, n_crops] -> [n, 1, n_crops, crop_frames, C] (utils.py:364-379).  `stats` (cmvn_stats):
        the copied rows are CMVN-normalised on the way (svk_cube_gather_cmvn) -- feat itself stays raw."""
        torch = _torch()
        feat = self.to_device(feat, torch.float32)
        idx = self.to_device(crop_idx, torch.int32)
        n, T, Cc = feat.shape
        n_crops = idx.shape[1]
        if out is None:
            out = torch.empty((n, 1, n_crops, crop_frames, Cc), dtype=torch.float32, device=self.device)
        self._stream()
        if stats is not None:
            if stats.dtype != torch.float64 or tuple(stats.shape) != (n, 2, Cc) or not stats.is_contiguous():
                raise ValueError("stats must be the float64 [n, 2, cols] tensor of cmvn_stats")
            check(self.lib.svk_cube_gather_cmvn(self.ctx, self._ptr(feat), n, T, Cc, self._ptr(idx), n_crops, crop_frames,
                                                self._ptr(stats), self._ptr(out)), self.ctx)
            return out
        check(self.lib.svk_cube_gather(self.ctx, self._ptr(feat), n, T, Cc, self._ptr(idx), n_crops, crop_frames,
                                       self._ptr(out)), self.ctx)
        return out

    def cube_gather_delta(self, feat, crop_idx, crop_frames=80, delta=2, stats=None, out=None):
        """svk_cube_gather_delta: STATIC feat [n, T, C] + crop_idx [n, n_crops] -> the three-channel cube
        [n, 3, n_crops, crop_frames, C] (utils.py:325-348), normalised per channel with `stats` (delta_cmvn_stats): the delta
        channels exist only for the rows the crops read."""
        torch = _torch()
        feat = self._static_rows(feat, "cube_gather_delta")
        idx = self.to_device(crop_idx, torch.int32)
        n, T, Cc = feat.shape
        if idx.dim() != 2 or idx.shape[0] != n or not idx.is_contiguous():
            raise ValueError("crop_idx must be [n, n_crops] int32")
        n_crops = idx.shape[1]
        stats = self._stats3(stats, n, Cc)
        shape = (n, 3, n_crops, crop_frames, Cc)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            self._given_out(out, shape, torch.float32, "out must be a contiguous float32 CUDA tensor [n, 3, n_crops, crop_frames, cols]")
        self._stream()
        check(self.lib.svk_cube_gather_delta(self.ctx, self._ptr(feat), n, T, Cc, self._ptr(idx), n_crops, int(crop_frames),
                                             int(delta), self._ptr(stats), self._ptr(out)), self.ctx)
        return out

    def c3d2_stage1(self, feat, crop_idx, tables, crop_frames=80, cubes_per_clip=1, live_cols=18):
        """svk_c3d2_stage1: feature rows [n, T, 40] + crop starts [n, 20] -> the activation after C3D2's first block (conv1_1,
        conv1_2, pool1 with their BN + PReLU): [n, 16, 36, 18, 16] f32, channels last.  Two-piece f16 products on
        v_mfma_f32_16x16x32_f16 (x = h + l, three piece products per f32 product, f32 accumulation: ~1e-6 of the scale from the
        f32 form); tables: `FusedEmbedder.stage1_tables()`.  The tables of a three-channel model (conv1_1 block [3, 2, 64, 8])
        run svk_c3d2_stage1_c3 on feature rows [n, 3, T, 40] (static, delta, delta-delta) instead: the same output layout.
        cubes_per_clip = K > 1 (or crop starts [n, K, 20]): K cubes of every clip's rows through svk_c3d2_stage1_multi /
        svk_c3d2_stage1_c3_multi -> [n K, 16, 36, 18, 16], cube-major; K = 1 with [n, 20] starts runs the entries above.
        live_cols = 17 (flags bit 5) is for an output that goes to `c3d2_stage2` and nowhere else: pooled column 17, which the
        second block never reads, is neither computed nor written -- out[:, :, :, 17] is whatever the allocator handed over --
        and columns 0 .. 16 are the bits of the default call."""
        torch = _torch()
        if live_cols not in (17, 18):
            raise ValueError("live_cols must be 18 (the whole output) or 17 (column 17 left unwritten), got %r" % (live_cols,))
        feat = self.to_device(feat, torch.float32)
        idx = self.to_device(crop_idx, torch.int32)
        three = tuple(tables[0].shape) == (3, 2, 64, 8)
        if feat.dim() != (4 if three else 3) or (three and feat.shape[1] != 3):
            raise ValueError("these stage-1 tables take feature rows %s, got %s"
                             % ("[n, 3, T, cols]" if three else "[n, T, cols]", tuple(feat.shape)))
        n, T, Cc = feat.shape[0], feat.shape[-2], feat.shape[-1]
        K = int(cubes_per_clip)
        multi = idx.dim() == 3 or K != 1
        if multi and K >= 1:              # (K < 1 goes to the library as it is: SVK_ERR_BAD_ARG)
            if idx.dim() == 2 and idx.shape[0] == n and idx.shape[1] % K == 0:
                idx = idx.view(n, K, -1)              # [n, 20 K], as draw_crops(n_crops=20 K) returns it
            if idx.dim() != 3 or idx.shape[0] != n or idx.shape[1] < 1 or (K != 1 and idx.shape[1] != K):
                raise ValueError("crop_idx must be [n, K, n_crops] for K cubes of each of the n = %d clips, got %s" % (n, tuple(idx.shape)))
            K = int(idx.shape[1])
        elif not multi and (idx.dim() != 2 or idx.shape[0] != n):
            raise ValueError("crop_idx must be [n, n_crops] for the n = %d cubes, got %s" % (n, tuple(idx.shape)))
        layers = self._c3d2_layers(tables, ((3, 2, 64, 8) if three else (2, 64, 8), (14, 2, 64, 8)), torch.float16, 16)
        if live_cols == 17:
            layers[-1] |= 32
        out = torch.empty((n * max(K, 0), 16, 36, 18, 16), dtype=torch.float32, device=self.device)
        self._stream()
        if multi:
            fn = self.lib.svk_c3d2_stage1_c3_multi if three else self.lib.svk_c3d2_stage1_multi
            check(fn(self.ctx, self._ptr(feat), n, T, Cc, self._ptr(idx), idx.shape[-1], crop_frames, *layers, self._ptr(out), K), self.ctx)
            return out
        fn = self.lib.svk_c3d2_stage1_c3 if three else self.lib.svk_c3d2_stage1
        check(fn(self.ctx, self._ptr(feat), n, T, Cc, self._ptr(idx), idx.shape[1], crop_frames, *layers, self._ptr(out)), self.ctx)
        return out

    def _c3d2_layers(self, tables, w_shapes, w_dtype, co):
        """The operand tables of a network entry point -- (weight blocks, bias, slope) per layer, then optionally whether every
        slope lies in [0, 1] -- checked against the blocks' shapes and the `co` output channels of each layer (the kernels read
        them unchecked); -> their pointers and the flags, in C-ABI order."""
        f32, ptr = _torch().float32, self._ptr
        args = []
        for i, w_shape in enumerate(w_shapes):
            wfrag, bias, slope = tables[3 * i], tables[3 * i + 1], tables[3 * i + 2]
            if wfrag.shape != w_shape or wfrag.dtype != w_dtype or not wfrag.is_contiguous():
                raise ValueError("weight blocks: want %s of %s, got %s of %s" % (w_shape, w_dtype, tuple(wfrag.shape), wfrag.dtype))
            if bias.numel() != co or slope.numel() != co or bias.dtype != f32 or slope.dtype != f32:
                raise ValueError("bias / slope: want %d float32 values each" % co)
            args += (ptr(wfrag), ptr(bias), ptr(slope))
        k = 3 * len(w_shapes)
        args.append(2 if len(tables) > k and tables[k] else 0)      # bit 1: every slope in [0, 1], the two-instruction PReLU
        return args

    def _c3d2_block(self, fn, act, tables, out_shape, w_shapes, co, w_dtype=None, scratch_shape=None, scratch_used=True):
        """fn(ctx, act, n, (weight blocks, bias, slope) per layer, flags[, scratch], out) -> out [n, *out_shape] f32
        (weight blocks of f16 unless `w_dtype`)."""
        torch = _torch()
        n = act.shape[0]
        args = self._c3d2_layers(tables, w_shapes, w_dtype or torch.float16, co)
        if scratch_shape is not None:      # held until the launch is enqueued: `out` must not reuse its memory
            scratch = torch.empty((n,) + scratch_shape, dtype=torch.float32, device=self.device) if scratch_used else None
            args.append(self._ptr(scratch) if scratch_used else None)       # (None: a NULL scratch the entry point never touches)
        out = torch.empty((n,) + out_shape, dtype=torch.float32, device=self.device)
        self._stream()
        check(fn(self.ctx, self._ptr(act), n, *args, self._ptr(out)), self.ctx)
        return out

    def c3d2_stage2(self, act1, tables):
        """svk_c3d2_stage2: [n, 16, 36, 18, 16] (svk_c3d2_stage1's output) -> conv2_1 -> conv2_2 -> pool2 with their
        BN + PReLU -> [n, 12, 15, 7, 32] f32 (channels last), both convolutions through two-piece f16 products.  Pooled column
        17 of act1 is not read by any product (conv2_1's last live column, 13, ends at column 16): `c3d2_stage1(live_cols=17)`
        may leave it unwritten."""
        if tuple(act1.shape[1:]) != (16, 36, 18, 16) or not act1.is_contiguous():
            raise ValueError("c3d2_stage2 wants the activation [n, 16, 36, 18, 16]")
        # conv2_1's activation stays in LDS; only the two-kernel reference path (SVK_C3D2_STAGE2_TWO_KERNELS, read by the library at
        # every call) goes through the scratch: the 14 columns of conv2_1 that pool2 leaves alive, 903 KB per cube
        return self._c3d2_block(self.lib.svk_c3d2_stage2, act1, tables, (12, 15, 7, 32), ((2, 6, 2, 64, 8), (2, 24, 2, 64, 8)), 32,
                                scratch_shape=(14, 36, 14, 32), scratch_used="SVK_C3D2_STAGE2_TWO_KERNELS" in os.environ)

    def c3d2_conv31(self, act, tables):
        """svk_c3d2_conv31: [n, 12, 15, 7, 32] (svk_c3d2_stage2's output) -> conv3_1 + BN + PReLU -> chunked, column-major
        [n, 10 d, 8 chunks, 5 w, 15 h, 8] f32: what svk_c3d2_conv32t stages from."""
        if tuple(act.shape[1:]) != (12, 15, 7, 32) or not act.is_contiguous():
            raise ValueError("c3d2_conv31 wants the activation [n, 12, 15, 7, 32]")
        return self._c3d2_block(self.lib.svk_c3d2_conv31, act, tables, (10, 8, 5, 15, 8), ((4, 9, 2, 64, 8),), 64)

    def c3d2_conv32t(self, act, tables):
        """svk_c3d2_conv32t: chunked, column-major [n, 10, 8, 5, 15, 8] (svk_c3d2_conv31's output) -> conv3_2 + BN + PReLU ->
        chunked [n, 8 d, 8 chunks, 45 = 9 h x 5 w, 8] (the shape of the last block: M tile = one position of 16 cubes)."""
        if tuple(act.shape[1:]) != (10, 8, 5, 15, 8) or not act.is_contiguous():
            raise ValueError("c3d2_conv32t wants the chunked activation [n, 10, 8, 5, 15, 8]")
        return self._c3d2_block(self.lib.svk_c3d2_conv32t, act, tables, (8, 8, 45, 8), ((4, 2, 21, 2, 64, 8),), 64)

    def c3d2_conv41(self, act, tables):
        """svk_c3d2_conv41: chunked [n, 8 d, 8 chunks, 45, 8] (svk_c3d2_conv32t's output) -> conv4_1 + BN + PReLU
        -> chunked [n, 6 d, 16 chunks, 27 = 9 h x 3 w, 8]."""
        if tuple(act.shape[1:]) != (8, 8, 45, 8) or not act.is_contiguous():
            raise ValueError("c3d2_conv41 wants the chunked activation [n, 8, 8, 45, 8]")
        return self._c3d2_block(self.lib.svk_c3d2_conv41, act, tables, (6, 16, 27, 8), ((8, 9, 2, 2, 64, 8),), 128)

    def c3d2_conv42(self, act, tables):
        """svk_c3d2_conv42: chunked [n, 6, 16, 27, 8] -> conv4_2 + BN + PReLU -> chunked [n, 4 d, 16 chunks, 9 = 3 h x 3 w, 8]."""
        if tuple(act.shape[1:]) != (6, 16, 27, 8) or not act.is_contiguous():
            raise ValueError("c3d2_conv42 wants the chunked activation [n, 6, 16, 27, 8]")
        return self._c3d2_block(self.lib.svk_c3d2_conv42, act, tables, (4, 16, 9, 8), ((8, 16, 7, 4, 64, 2),), 128, _torch().float32)

    def c3d2_fc5(self, act, tables):
        """svk_c3d2_fc5: chunked [n, 4, 16, 9, 8] (= [n, 4 608]) -> FC5 -> [n, 128] embeddings."""
        torch = _torch()
        n = act.shape[0]
        if act.numel() != n * 4608 or not act.is_contiguous():
            raise ValueError("c3d2_fc5 wants [n, 4608] (svk_c3d2_conv42's output)")
        wfrag, bias = tables
        work = torch.empty((int(self.lib.svk_c3d2_fc5_workspace_floats(n)),), dtype=torch.float32, device=self.device)
        out = torch.empty((n, 128), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_c3d2_fc5(self.ctx, self._ptr(act), n, self._ptr(wfrag), self._ptr(bias), self._ptr(work),
                                    self._ptr(out)), self.ctx)
        return out

    def c3d2_head(self, emb, tables, probs=True, k=1, true_idx=None):
        """svk_c3d2_head: embeddings [n, 128] -> PReLU5 -> FC6 -> softmax (model.py:170-174).  tables = (w6 [n_labels, 128],
        b6 [n_labels], slope) as `C3D2.fused_head()` holds them.  Returns (probs f32 [n, n_labels] | None, top-k int32 [n, k] |
        None, hits | None), tensors on the device: the top-k when k is not None, hits (a list of k ints: rows whose true label
        is among their first r + 1) when true_idx ([n] ints, -1 = none) is given."""
        torch = _torch()
        w6, b6, slope = tables
        x = self.to_device(emb, torch.float32)
        if x.dim() != 2 or x.shape[1] != 128:
            raise ValueError("c3d2_head wants embeddings (n, 128)")
        x = x.contiguous()
        n, n_labels = int(x.shape[0]), int(w6.shape[0])
        if tuple(w6.shape) != (n_labels, 128) or tuple(b6.shape) != (n_labels,) or w6.device != x.device or b6.device != x.device:
            raise ValueError("c3d2_head wants FC6 tables w6 (n_labels, 128) and b6 (n_labels,) on the device")
        if true_idx is not None and k is None:
            raise ValueError("c3d2_head counts hits over the top-k: give k with true_idx")
        tr = None
        if true_idx is not None:
            tr = self.to_device(true_idx, torch.int32).reshape(-1).contiguous()
            if tr.numel() != n:
                raise ValueError("c3d2_head wants one true label per row")
        p = torch.empty((n, n_labels), dtype=torch.float32, device=self.device) if probs else None
        top = torch.empty((n, int(k)), dtype=torch.int32, device=self.device) if k is not None and int(k) >= 1 else None
        hits = (C.c_int64 * max(1, int(k) if k is not None else 1))()
        self._stream()
        check(self.lib.svk_c3d2_head(self.ctx, self._ptr(x), n, n_labels, float(slope), self._ptr(w6), self._ptr(b6),
                                     self._ptr(p), int(k) if k is not None else 0, self._ptr(top), self._ptr(tr),
                                     hits if tr is not None else None), self.ctx)
        return p, top, ([int(v) for v in hits[:int(k)]] if tr is not None else None)

    def cosine_scores(self, test, enroll):
        torch = _torch()
        t, e = self._two_matrices(test, enroll, "cosine_scores")
        out = torch.empty((t.shape[0], e.shape[0]), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_cosine_scores(self.ctx, self._ptr(t), self._ptr(e), t.shape[0], e.shape[0], t.shape[1],
                                         self._ptr(out)), self.ctx)
        return out

    def roc_eer(self, scores, labels):
        """(eer, auc) of flat scores / 0-1 labels, computed on the device (svk_roc_eer)."""
        sc, lb = self._scores_labels(scores, labels)
        n = sc.numel()
        work = self._workspace(self.lib.svk_roc_workspace_bytes(n))
        out = (C.c_double * 4)()
        self._stream()
        check(self.lib.svk_roc_eer(self.ctx, self._ptr(sc), self._ptr(lb), n, self._ptr(work), work.numel(), out),
              self.ctx)
        return float(out[0]), float(out[1])

    def roc_dcf(self, scores, labels, operating_points=()):
        """svk_roc_dcf: EER, AUC, minDCF and the thresholds of flat scores / 0-1 labels from one sort on the device.
        operating_points: up to 8 (p_target, c_miss, c_fa).  Returns a dict: eer, auc, positives, points, eer_threshold, and one
        entry per operating point in the lists min_dcf, threshold, p_miss, p_fa (accept when score >= threshold; the origin of
        the ROC, "reject everything", has threshold +inf).  eer and auc are roc_eer's values, bit for bit.  Raises for a
        non-finite score or a single class."""
        return self._roc_dcf_call(scores, labels, operating_points, None)[0]

    def _roc_dcf_call(self, scores, labels, operating_points, planes):
        """svk_roc_dcf (planes None) or svk_rocch (planes: int32 [3, capacity] on the device) -> (roc_dcf's dict, the vertex
        count or None): the two entries' shared arguments and the shared head of h_out, stated once."""
        sc, lb = self._scores_labels(scores, labels)
        n = sc.numel()
        ops = np.ascontiguousarray(np.asarray(operating_points, dtype=np.float64).reshape(-1, 3))
        n_op = int(ops.shape[0])
        h_ops = ops.ctypes.data_as(C.POINTER(C.c_double))
        out = (C.c_double * (6 + 4 * n_op))()
        self._stream()
        if planes is None:
            work = self._workspace(self.lib.svk_roc_dcf_workspace_bytes(n))
            check(self.lib.svk_roc_dcf(self.ctx, self._ptr(sc), self._ptr(lb), n, h_ops, n_op, self._ptr(work), work.numel(), out),
                  self.ctx)
        else:
            work = self._workspace(self.lib.svk_rocch_workspace_bytes(n))
            check(self.lib.svk_rocch(self.ctx, self._ptr(sc), self._ptr(lb), n, h_ops, n_op, self._ptr(work), work.numel(),
                                     self._ptr(planes[0]), self._ptr(planes[1]), self._ptr(planes[2]), int(planes.shape[1]), out),
                  self.ctx)
        res = {"eer": float(out[0]), "auc": float(out[1]), "positives": int(out[2]), "points": int(out[3]),
               "eer_threshold": float(out[4])}
        for j, name in enumerate(("min_dcf", "threshold", "p_miss", "p_fa")):
            res[name] = [float(out[5 + 4 * o + j]) for o in range(n_op)]
        return res, (None if planes is None else int(out[5 + 4 * n_op]))

    def rocch(self, scores, labels, operating_points=()):
        """svk_rocch (include/svk.h, "the ROC convex hull"): roc_dcf's dict -- the same values, bit for bit -- plus the ROC convex hull from
        the same sort: vertices (int64 [K + 1, 2] on the host: fps, tps, the origin first, (N, P) last), vertex_scores (float32
        [K + 1]: the score at each vertex, +inf at the origin), and min_cllr and rocch_eer, computed from the integer vertices
        in float64 on the host (`calibration.min_cllr_of`, `calibration.rocch_eer_of`).  ONE library call, the planes sized by
        svk_rocch_max_vertices.  Raises as roc_dcf does."""
        from . import calibration as cal
        torch = _torch()
        sc, lb = self._scores_labels(scores, labels)
        cap = max(1, int(self.lib.svk_rocch_max_vertices(sc.numel())))
        planes = torch.empty((3, cap), dtype=torch.int32, device=self.device)
        res, count = self._roc_dcf_call(sc, lb, operating_points, planes)
        host = planes[:, :count].cpu().numpy()
        res["vertices"] = np.ascontiguousarray(host[:2].view(np.uint32).T.astype(np.int64))
        res["vertex_scores"] = host[2].view(np.float32).copy()
        res["min_cllr"] = cal.min_cllr_of(res["vertices"])
        res["rocch_eer"] = cal.rocch_eer_of(res["vertices"])
        return res

    def pav_apply(self, scores, edges, llr, out=None):
        """svk_pav_apply: float32 [n] on the device, out[p] = llr[k] for the smallest k with scores[p] >= edges[k] (edges
        descending; the last bin below every edge; a NaN stays NaN).  out: the tensor to write; it may be the scores
        themselves (in place)."""
        torch = _torch()
        sc = self.to_device(scores, torch.float32).reshape(-1)
        ed = self.to_device(edges, torch.float32).reshape(-1)
        ll = self.to_device(llr, torch.float32).reshape(-1)
        n = sc.numel()
        if ed.numel() < 1 or ed.numel() != ll.numel():
            raise ValueError("pav_apply wants one LLR per edge and at least one bin")
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=self.device)
        else:
            self._given_out(out, n, torch.float32, "out wants a contiguous float32 device tensor of %d elements" % n)
        self._stream()
        check(self.lib.svk_pav_apply(self.ctx, self._ptr(sc), n, self._ptr(ed), self._ptr(ll), ed.numel(), self._ptr(out)),
              self.ctx)
        return out.reshape(-1)

    def decision_counts(self, scores, labels, thresholds):
        """svk_decision_counts: one pass over unsorted scores / 0-1 labels.  thresholds: 1 to 16 floats (+-inf allowed).  Returns
        (accepted int64 [n_thr, 2], totals): accepted[t] = (targets, non-targets) with score >= thresholds[t], totals = (targets,
        non-targets) of the set.  A NaN score is never accepted."""
        sc, lb = self._scores_labels(scores, labels)
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        n_thr = int(thr.size)
        out = (C.c_int64 * (2 * max(n_thr, 1) + 2))()
        self._stream()
        check(self.lib.svk_decision_counts(self.ctx, self._ptr(sc), self._ptr(lb), sc.numel(),
                                           thr.ctypes.data_as(C.POINTER(C.c_float)), n_thr, out), self.ctx)
        flat = np.array(out[:2 * n_thr + 2], dtype=np.int64)
        return flat[:2 * n_thr].reshape(n_thr, 2), (int(flat[2 * n_thr]), int(flat[2 * n_thr + 1]))

    def _score_planes(self, scores):
        """Scores as the calibration entries read them -> (f32 tensor [n_sys, n] with unit stride along n, plane_stride).
        scores: a tensor / array [n] or [n_sys, n], or a sequence of [n] tensors, stacked once (planes a multiple of four floats
        apart: the 16-byte loads).  A device f32 view whose rows are plane_stride >= n apart is taken as it is (no copy)."""
        torch = _torch()
        if isinstance(scores, (list, tuple)):
            rows = [self.to_device(s, torch.float32).reshape(-1) for s in scores]
            if not rows or any(r.numel() != rows[0].numel() for r in rows):
                raise ValueError("a sequence of systems wants one score per trial in each")
            n = rows[0].numel()
            scores = torch.empty((len(rows), (n + 3) // 4 * 4), dtype=torch.float32, device=self.device)[:, :n]
            for d, r in enumerate(rows):
                scores[d].copy_(r)
        if not (isinstance(scores, torch.Tensor) and scores.device == self.device and scores.dtype == torch.float32
                and scores.dim() == 2 and scores.stride(1) == 1 and scores.stride(0) >= scores.shape[1]):
            scores = self.to_device(scores, torch.float32)
            if scores.dim() == 1:
                scores = scores.reshape(1, -1)
        if scores.dim() != 2:
            raise ValueError("calibration scores want [n] or [n_sys, n], got %s" % (tuple(scores.shape),))
        n_sys, n = int(scores.shape[0]), int(scores.shape[1])
        return scores, (int(scores.stride(0)) if n_sys > 1 else n)

    def calibration_stats(self, scores, labels, weights, tau, class_weight, value_only=False):
        """svk_calibration_stats: one pass over the trials -> (l_tar, l_non, grad, hess, counts) at `weights` (float64
        [n_sys + 1], the offset last): the softplus sums of the two classes in nats (unweighted), the class-weighted gradient
        float64 [n_sys + 1] and Hessian float64 [n_sys + 1, n_sys + 1] (symmetric, filled from the packed triangle) of
        z = w . (s, 1) + tau, and counts = (targets, non-targets, skipped): a trial with a non-finite score is left out and
        counted as skipped.  class_weight = (target, non-target).  value_only: grad and hess are None (not computed)."""
        sc, stride = self._score_planes(scores)
        n_sys, n = int(sc.shape[0]), int(sc.shape[1])
        lb = self._labels01(labels, n)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        cw = np.ascontiguousarray(np.asarray(class_weight, dtype=np.float64).reshape(-1))
        if w.size != n_sys + 1 or cw.size != 2:
            raise ValueError("calibration_stats wants n_sys + 1 = %d weights and 2 class weights" % (n_sys + 1))
        dim = n_sys + 1
        work = self._workspace(self.lib.svk_calibration_stats_workspace_bytes(n, n_sys))
        out = (C.c_double * (2 + dim + dim * (dim + 1) // 2))()
        count = (C.c_int64 * 3)()
        dp = C.POINTER(C.c_double)
        self._stream()
        check(self.lib.svk_calibration_stats(self.ctx, self._ptr(sc), n_sys, stride, self._ptr(lb), n, w.ctypes.data_as(dp),
                                             float(tau), cw.ctypes.data_as(dp), 1 if value_only else 0, self._ptr(work),
                                             work.numel(), out, count), self.ctx)
        counts = (int(count[0]), int(count[1]), int(count[2]))
        if value_only:
            return float(out[0]), float(out[1]), None, None, counts
        flat = np.array(out[:], dtype=np.float64)
        hess = np.zeros((dim, dim), dtype=np.float64)
        hess[np.triu_indices(dim)] = flat[2 + dim:]
        hess = hess + np.triu(hess, 1).T
        return float(flat[0]), float(flat[1]), flat[2:2 + dim].copy(), hess, counts

    def calibration_apply(self, scores, weights, out=None):
        """svk_calibration_apply: f32 [n] on the device, out[p] = f32(sum_d weights[d] * scores[d, p] + weights[n_sys]) in
        float64.  out: the tensor to write; for one system it may be the scores themselves (in place)."""
        torch = _torch()
        sc, stride = self._score_planes(scores)
        n_sys, n = int(sc.shape[0]), int(sc.shape[1])
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.size != n_sys + 1:
            raise ValueError("calibration_apply wants n_sys + 1 = %d weights, got %d" % (n_sys + 1, w.size))
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=self.device)
        else:
            self._given_out(out, n, torch.float32, "out wants a contiguous float32 device tensor of %d elements" % n)
        self._stream()
        check(self.lib.svk_calibration_apply(self.ctx, self._ptr(sc), n_sys, stride, n, w.ctypes.data_as(C.POINTER(C.c_double)),
                                             self._ptr(out)), self.ctx)
        return out.reshape(-1)

    def _score_rows(self, scores, who):
        """A score matrix as the normalisation entries read it -> f32 [n_rows, n_cols] on the device with unit stride along a
        row.  A device f32 view whose rows are row_stride >= n_cols apart is taken as it is (no copy)."""
        torch = _torch()
        if not (isinstance(scores, torch.Tensor) and scores.device == self.device and scores.dtype == torch.float32
                and scores.dim() == 2 and (scores.shape[1] <= 1 or scores.stride(1) == 1)
                and (scores.shape[0] <= 1 or scores.stride(0) >= scores.shape[1])):
            scores = self.to_device(scores, torch.float32)
        if scores.dim() != 2:
            raise ValueError("%s wants a [n_rows, n_cols] score matrix, got %s" % (who, tuple(scores.shape)))
        return scores, (int(scores.stride(0)) if scores.shape[0] > 1 else int(scores.shape[1]))

    def _moments(self, moments, n, name):
        """An optional {mean, std} table as float64 [n, 2] on the device."""
        if moments is None:
            return None
        mom = self.to_device(moments, _torch().float64)
        if tuple(mom.shape) != (n, 2):
            raise ValueError("%s wants float64 [%d, 2] (mean, std), got %s" % (name, n, tuple(mom.shape)))
        return mom

    def cohort_moments(self, scores, top_k=0, want_used=False, want_kth=False):
        """svk_cohort_moments: the mean and population standard deviation of the top_k largest finite scores of every row of
        scores [n_rows, n_cohort] (top_k = 0: of all of them) -> float64 [n_rows, 2] on the device; a row without a finite
        score gives NaN, NaN.  With want_used or want_kth the result is (moments, used, kth): used int32 [n_rows] = the values
        that entered, kth float32 [n_rows] = the smallest of them (None for the one not asked for)."""
        torch = _torch()
        sc, stride = self._score_rows(scores, "cohort_moments")
        n_rows, n_cohort = int(sc.shape[0]), int(sc.shape[1])
        mom = torch.empty((n_rows, 2), dtype=torch.float64, device=self.device)
        used = torch.empty((n_rows,), dtype=torch.int32, device=self.device) if want_used else None
        kth = torch.empty((n_rows,), dtype=torch.float32, device=self.device) if want_kth else None
        self._stream()
        check(self.lib.svk_cohort_moments(self.ctx, self._ptr(sc), n_rows, n_cohort, stride, int(top_k), self._ptr(mom),
                                          self._ptr(used), self._ptr(kth)), self.ctx)
        return (mom, used, kth) if (want_used or want_kth) else mom

    def score_norm(self, scores, row_moments=None, col_moments=None, out=None):
        """svk_score_norm: scores [n_rows, n_cols] normalised by the rows' moments (T-norm), the columns' (Z-norm) or both
        (S-norm, the mean of the two) -> float32 [n_rows, n_cols] on the device, float64 arithmetic.  The tables are float64
        [n_rows, 2] and [n_cols, 2] as `cohort_moments` returns them.  out: the tensor to write; it may be the scores
        themselves (in place)."""
        torch = _torch()
        sc, stride = self._score_rows(scores, "score_norm")
        n_rows, n_cols = int(sc.shape[0]), int(sc.shape[1])
        rm, cm = self._moments(row_moments, n_rows, "row_moments"), self._moments(col_moments, n_cols, "col_moments")
        if out is None:
            out, out_stride = torch.empty((n_rows, n_cols), dtype=torch.float32, device=self.device), n_cols
        else:
            if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (n_rows, n_cols)):
                raise ValueError("out wants a float32 device tensor of shape %s" % ((n_rows, n_cols),))
            kept, out_stride = self._score_rows(out, "score_norm")
            if kept.data_ptr() != out.data_ptr():
                raise ValueError("out wants rows of unit stride on this device")
        self._stream()
        check(self.lib.svk_score_norm(self.ctx, self._ptr(sc), n_rows, n_cols, stride, self._ptr(rm), self._ptr(cm),
                                      self._ptr(out), out_stride), self.ctx)
        return out

    def score_norm_pairs(self, scores, mom_a, idx_a, mom_b, idx_b, out=None, bad_count=None):
        """svk_score_norm_pairs: `score_norm` for a trial list -> float32 [n] on the device: trial p takes the row moments
        mom_a[idx_a[p]] and the column moments mom_b[idx_b[p]].  A table (and then its indices) may be None.  An index outside
        its table gives NaN at that trial and counts in bad_count (an int32 [1] device tensor the caller zeroes), if given.
        out: the tensor to write; it may be the scores themselves."""
        torch = _torch()
        sc = self.to_device(scores, torch.float32).reshape(-1)
        n = sc.numel()
        i64 = torch.int64
        ma = None if mom_a is None else self.to_device(mom_a, torch.float64)
        mb = None if mom_b is None else self.to_device(mom_b, torch.float64)
        for mom, name in ((ma, "mom_a"), (mb, "mom_b")):
            if mom is not None and (mom.dim() != 2 or mom.shape[1] != 2):
                raise ValueError("%s wants float64 [n, 2] (mean, std), got %s" % (name, tuple(mom.shape)))
        ia = None if ma is None else self.to_device(idx_a, i64).reshape(-1)
        ib = None if mb is None else self.to_device(idx_b, i64).reshape(-1)
        if any(ix is not None and ix.numel() != n for ix in (ia, ib)):
            raise ValueError("one index per trial and table")
        bad_count = self._counter(bad_count, "bad_count")
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=self.device)
        else:
            self._given_out(out, n, torch.float32, "out wants a contiguous float32 device tensor of %d elements" % n)
        self._stream()
        check(self.lib.svk_score_norm_pairs(self.ctx, self._ptr(sc), n, self._ptr(ma), 0 if ma is None else ma.shape[0],
                                            self._ptr(mb), 0 if mb is None else mb.shape[0], self._ptr(ia), self._ptr(ib),
                                            self._ptr(out), self._ptr(bad_count)), self.ctx)
        return out.reshape(-1)

    def roc_k(self, scores, labels, k=1, curve=False):
        """svk_roc_k: per split of `split_step(n, k)` consecutive pairs (evaluation.py:11-33), (eer, auc), or with
        curve=True (eer, auc, fpr, tpr): sklearn's roc_curve(drop_intermediate=True) as float64 NumPy arrays, fps / fps[-1]
        and tps / tps[-1] on the device's integer counts.  Raises for a split with one class or a non-finite score."""
        torch = _torch()
        sc, lb = self._scores_labels(scores, labels)
        n, k = sc.numel(), int(k)
        step = split_step(n, k) if k >= 1 else 0
        work = self._workspace(self.lib.svk_roc_k_workspace_bytes(n, k))
        planes = torch.empty((2, k, step + 1), dtype=torch.int32, device=self.device) if curve and step >= 2 else None
        out = (C.c_double * (4 * max(k, 1)))()
        self._stream()
        check(self.lib.svk_roc_k(self.ctx, self._ptr(sc), self._ptr(lb), n, k, self._ptr(work), work.numel(),
                                 self._ptr(planes), out), self.ctx)
        res = []
        for s in range(k):
            eer, auc, length = float(out[4 * s]), float(out[4 * s + 1]), int(out[4 * s + 3])
            if planes is None:
                res.append((eer, auc))
                continue
            fps, tps = (planes[p, s, :length].cpu().numpy().view(np.uint32).astype(np.float64) for p in (0, 1))
            res.append((eer, auc, fps / fps[-1], tps / tps[-1]))
        return res

    def top1(self, scores, true_idx, want_labels=False):
        """svk_top1 on a [n_rows, n_cols] score matrix: (argmax int32 [n_rows], correct, [labels uint8 [n_rows, n_cols]]),
        tensors on the device.  true_idx[r]: the enrolled column of row r's speaker, -1 = not enrolled; argmax is
        np.argmax's (first maximum, NaN first); correct counts the rows whose argmax is their true column."""
        torch = _torch()
        sc = self.to_device(scores, torch.float32)
        tr = self.to_device(true_idx, torch.int32).reshape(-1)
        if sc.dim() != 2 or tr.numel() != sc.shape[0]:
            raise ValueError("top1 wants scores (n_rows, n_cols) and one true index per row")
        n_rows, n_cols = int(sc.shape[0]), int(sc.shape[1])
        amax = torch.empty((n_rows,), dtype=torch.int32, device=self.device)
        labels = torch.empty((n_rows, n_cols), dtype=torch.uint8, device=self.device) if want_labels else None
        correct = C.c_int64()
        self._stream()
        check(self.lib.svk_top1(self.ctx, self._ptr(sc), n_rows, n_cols, self._ptr(tr), self._ptr(amax), self._ptr(labels),
                                C.byref(correct)), self.ctx)
        return (amax, int(correct.value), labels) if want_labels else (amax, int(correct.value))

    def embedding_pool(self, emb, rows_per_seg=None, seg_start=None, row_index=None, l2_rows=False, l2_mean=False,
                       empty_count=None):
        """svk_embedding_pool: the float64 mean over groups of the rows of emb [n_rows, dim] -> [n_seg, dim] f32.  Groups:
        `rows_per_seg` = K consecutive rows each (n_rows a multiple of K), or `seg_start` int64 [n_seg + 1] CSR offsets; with
        `row_index` int64 [n_rows] the rows of a group are emb[row_index[i]] over its range.  l2_rows: every row enters
        L2-normalised; l2_mean: the mean leaves L2-normalised.  empty_count: an int32 [1] device tensor (the caller zeroes it)
        that takes the number of empty groups, which come out as zeros."""
        torch = _torch()
        x = self.to_device(emb, torch.float32)
        if x.dim() != 2:
            raise ValueError("embedding_pool wants rows (n_rows, dim)")
        n_rows, dim = int(x.shape[0]), int(x.shape[1])
        if (rows_per_seg is None) == (seg_start is None):
            raise ValueError("embedding_pool wants either rows_per_seg or seg_start")
        K = 0
        if seg_start is not None:
            start, index = self._segments(seg_start, row_index, n_rows)
            n_seg = start.numel() - 1
        else:
            K = int(rows_per_seg)
            if K < 1 or n_rows % K:
                raise ValueError("rows_per_seg = %d does not divide the %d rows" % (K, n_rows))
            n_seg = n_rows // K
            start, index = None, self._row_index(row_index, n_rows)
        self._counter(empty_count, "empty_count")
        out = torch.empty((n_seg, dim), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_embedding_pool(self.ctx, self._ptr(x), n_rows, dim, n_seg, K, self._ptr(start), self._ptr(index),
                                          int(bool(l2_rows)) | 2 * int(bool(l2_mean)), self._ptr(out), self._ptr(empty_count)),
              self.ctx)
        return out

    def window_crops(self, n_frames, max_windows, win_frames=150, hop_frames=75, crop_frames=80, n_crops=20, bad_count=None,
                     want_spans=True):
        """svk_window_crops: frame counts [n_rec] i32 -> (crop_idx [n_rec, max_windows, n_crops] i32 with -1 in unused windows,
        n_windows [n_rec] i32, spans [n_rec, max_windows, 2] i32 = (first frame, length), or None without want_spans), all on the
        device.  A recording of T frames has no window below crop_frames, the one window [0, T) below win_frames, else windows of
        win_frames every hop_frames and a last one flush with the end; crop c of a window spreads evenly over it.  A recording
        that needs more than max_windows keeps the first ones and counts in bad_count (int32 [1] device tensor, caller zeroes)."""
        torch = _torch()
        nf = self.to_device(n_frames, torch.int32).reshape(-1)
        n_rec, K, nc = nf.numel(), int(max_windows), int(n_crops)
        self._counter(bad_count, "bad_count")
        idx = torch.empty((n_rec, max(K, 0), max(nc, 0)), dtype=torch.int32, device=self.device)
        nwin = torch.empty((n_rec,), dtype=torch.int32, device=self.device)
        spans = torch.empty((n_rec, max(K, 0), 2), dtype=torch.int32, device=self.device) if want_spans else None
        self._stream()
        check(self.lib.svk_window_crops(self.ctx, self._ptr(nf), n_rec, int(win_frames), int(hop_frames), int(crop_frames), nc, K,
                                        self._ptr(idx), self._ptr(nwin), self._ptr(spans), self._ptr(bad_count)), self.ctx)
        return idx, nwin, spans

    def _n_seg(self, n_seg, n_rec):
        """The live-row counts of a padded batch as int32 [n_rec] on the device."""
        ns = self.to_device(n_seg, _torch().int32).reshape(-1)
        if ns.numel() != n_rec:
            raise ValueError("n_seg holds one count per recording")
        return ns

    def segment_affinity(self, emb, n_seg, out=None):
        """svk_segment_affinity: emb [n_rec, seg_stride, dim] f32 + n_seg [n_rec] i32 -> the cosines of every pair of live rows
        of every recording, float32 [n_rec, seg_stride, seg_stride] on the device (float64 arithmetic, symmetric bit for bit).
        Entries of dead rows are NOT written: `out` (a float32 device tensor of that shape) keeps what it held there; without
        `out` they are zeros."""
        torch = _torch()
        x = self.to_device(emb, torch.float32)
        if x.dim() != 3:
            raise ValueError("segment_affinity wants rows (n_rec, seg_stride, dim)")
        n_rec, stride, dim = (int(v) for v in x.shape)
        ns = self._n_seg(n_seg, n_rec)
        if out is None:
            out = torch.zeros((n_rec, stride, stride), dtype=torch.float32, device=self.device)
        else:
            self._given_out(out, (n_rec, stride, stride), torch.float32, "out must be a contiguous float32 device tensor [n_rec, seg_stride, seg_stride]")
        self._stream()
        check(self.lib.svk_segment_affinity(self.ctx, self._ptr(x), n_rec, stride, dim, self._ptr(ns), self._ptr(out)), self.ctx)
        return out

    def ahc_limits(self):
        """svk_ahc_limits: (the largest n_seg clustered in LDS, the largest seg_stride svk_ahc takes)."""
        out = (C.c_int32 * 2)()
        check(self.lib.svk_ahc_limits(out))
        return int(out[0]), int(out[1])

    def ahc(self, aff, n_seg, threshold=None, min_clusters=1, max_clusters=None, target=None, want_merges=False,
            bad_count=None, labels_out=None):
        """svk_ahc: average-linkage agglomerative clustering of every recording of aff [n_rec, seg_stride, seg_stride] f32
        (similarities, only the entries above the diagonal of the n_seg[r] live rows are read) -> (labels [n_rec, seg_stride]
        i32, n_clusters [n_rec] i32) on the device; with want_merges also merge_pair [n_rec, seg_stride, 2] i32 and merge_sim
        [n_rec, seg_stride] f64.  A step merges the most similar pair while more than max_clusters clusters are left, or while
        more than min_clusters are left and the pair reaches `threshold` (None: nothing does).  target: int32 [n_rec], a value
        >= 1 fixes that recording's cluster count.  Labels of dead rows are -1 here (the library leaves them alone: a given
        labels_out, int32 [n_rec, seg_stride] on the device, keeps what it held there); a recording
        with a non-finite entry or a count out of range gets labels -1, count -1 and counts in bad_count."""
        torch = _torch()
        a = self.to_device(aff, torch.float32)
        if a.dim() != 3 or a.shape[1] != a.shape[2]:
            raise ValueError("ahc wants matrices (n_rec, seg_stride, seg_stride)")
        n_rec, stride = int(a.shape[0]), int(a.shape[1])
        ns = self._n_seg(n_seg, n_rec)
        tg = self._n_seg(target, n_rec) if target is not None else None
        self._counter(bad_count, "bad_count")
        thr = float("inf") if threshold is None else float(threshold)
        max_c = 0x7fffffff if max_clusters is None else int(max_clusters)
        work = self._workspace(self.lib.svk_ahc_workspace_bytes(n_rec, stride))
        if labels_out is None:
            labels = torch.full((n_rec, stride), -1, dtype=torch.int32, device=self.device)
        else:
            labels = labels_out
            self._given_out(labels, (n_rec, stride), torch.int32, "labels_out must be a contiguous int32 device tensor [n_rec, seg_stride]")
        count = torch.empty((n_rec,), dtype=torch.int32, device=self.device)
        pair = torch.empty((n_rec, stride, 2), dtype=torch.int32, device=self.device) if want_merges else None
        sim = torch.empty((n_rec, stride), dtype=torch.float64, device=self.device) if want_merges else None
        self._stream()
        check(self.lib.svk_ahc(self.ctx, self._ptr(a), n_rec, stride, self._ptr(ns), thr, int(min_clusters), max_c, self._ptr(tg),
                               self._ptr(work), work.numel(), self._ptr(labels), self._ptr(count), self._ptr(pair), self._ptr(sim),
                               self._ptr(bad_count)), self.ctx)
        return (labels, count, pair, sim) if want_merges else (labels, count)

    def spectral_limits(self):
        """svk_spectral_limits: (the most nodes per recording, the largest seg_stride, the largest max_speakers)."""
        out = (C.c_int32 * 3)()
        check(self.lib.svk_spectral_limits(out))
        return int(out[0]), int(out[1]), int(out[2])

    @staticmethod
    def _neighbour_sweep(neighbours):
        """An int p, or (lo, hi, step): the candidates lo, lo + step, ... up to hi -> (lo, step, count)."""
        if isinstance(neighbours, (int, np.integer)):
            return int(neighbours), 1, 1
        lo, hi, step = (int(v) for v in neighbours)
        if lo < 1 or step < 1 or hi < lo:
            raise ValueError("neighbours is an int >= 1 or (lo, hi, step) with 1 <= lo <= hi and step >= 1")
        return lo, step, (hi - lo) // step + 1

    def spectral_embed(self, aff, n_seg, group=None, neighbours=(2, 32, 2), min_speakers=1, max_speakers=8, target=None,
                       want_spectrum=False, want_graph=False, bad_count=None):
        """svk_spectral_embed: the spectral embedding of every recording of aff [n_rec, seg_stride, seg_stride] f32 (only the
        entries above the diagonal of the n_seg[r] live rows are read), the speaker count from the largest eigengap and the
        graph's neighbour count from the normalised maximum eigengap -> (embed [n_rec, node_stride, max_speakers] f32,
        n_nodes, n_speakers, neighbours, each [n_rec] i32) on the device; with want_spectrum also eigval [n_rec, node_stride]
        f64 and eigvec [n_rec, max_speakers, node_stride] f64, with want_graph also graph [n_rec, node_stride, node_stride]
        u8 (twice the symmetrised adjacency) and ratio [n_rec, candidates] f64.  group: None (every window is a node;
        node_stride = seg_stride), or svk_ahc's labels int32 [n_rec, seg_stride] (node_stride = spectral_limits()[0]).
        neighbours: an int, or a (lo, hi, step) search range.  target: int32 [n_rec], a value >= 1 fixes that recording's
        count.  What the library leaves alone (dead rows, unused vectors) is zero here.  A bad recording (non-finite entry,
        counts or labels out of range, no convergence) reads -1 in the three counts and counts in bad_count."""
        torch = _torch()
        a = self.to_device(aff, torch.float32)
        if a.dim() != 3 or a.shape[1] != a.shape[2]:
            raise ValueError("spectral_embed wants matrices (n_rec, seg_stride, seg_stride)")
        n_rec, stride = int(a.shape[0]), int(a.shape[1])
        ns = self._n_seg(n_seg, n_rec)
        tg = self._n_seg(target, n_rec) if target is not None else None
        self._counter(bad_count, "bad_count")
        grp, nodes = None, stride
        if group is not None:
            grp = self.to_device(group, torch.int32)
            if tuple(grp.shape) != (n_rec, stride):
                raise ValueError("group holds one label per window: int32 [n_rec, seg_stride]")
            nodes = self.spectral_limits()[0]
        lo, step, count = self._neighbour_sweep(neighbours)
        K = int(max_speakers)
        work = self._workspace(self.lib.svk_spectral_workspace_bytes(n_rec, stride, nodes))
        dev = self.device
        embed = torch.zeros((n_rec, nodes, max(K, 0)), dtype=torch.float32, device=dev)
        n_nodes, n_spk, chosen = (torch.empty((n_rec,), dtype=torch.int32, device=dev) for _ in range(3))
        eigval = torch.zeros((n_rec, nodes), dtype=torch.float64, device=dev) if want_spectrum else None
        eigvec = torch.zeros((n_rec, max(K, 0), nodes), dtype=torch.float64, device=dev) if want_spectrum else None
        graph = torch.zeros((n_rec, nodes, nodes), dtype=torch.uint8, device=dev) if want_graph else None
        ratio = torch.empty((n_rec, count), dtype=torch.float64, device=dev) if want_graph else None
        self._stream()
        check(self.lib.svk_spectral_embed(self.ctx, self._ptr(a), n_rec, stride, self._ptr(ns), self._ptr(grp), nodes, lo, step,
                                          count, int(min_speakers), K, self._ptr(tg), self._ptr(work), work.numel(),
                                          self._ptr(embed), self._ptr(n_nodes), self._ptr(n_spk), self._ptr(chosen),
                                          self._ptr(eigval), self._ptr(eigvec), self._ptr(graph), self._ptr(ratio),
                                          self._ptr(bad_count)), self.ctx)
        out = (embed, n_nodes, n_spk, chosen)
        if want_spectrum:
            out += (eigval, eigvec)
        if want_graph:
            out += (graph, ratio)
        return out

    def class_scatter(self, emb, seg_start, row_index=None, l2_rows=False):
        """svk_class_scatter: the float64 class means [n_class, dim] and the within-class scatter S_w [dim, dim] (two-pass, on
        the centred rows) of emb [n_rows, dim] f32 -> two float64 device tensors.  Class c is rows
        row_index[seg_start[c] : seg_start[c + 1]] (`pipeline.speaker_segments`); l2_rows: every row enters L2-normalised.
        Bit-identical from run to run, S_w symmetric bit for bit.  The workspace is a torch allocation sized by the library."""
        torch = _torch()
        x = self.to_device(emb, torch.float32)
        if x.dim() != 2:
            raise ValueError("class_scatter wants rows (n_rows, dim)")
        n_rows, dim = int(x.shape[0]), int(x.shape[1])
        start, index = self._segments(seg_start, row_index, n_rows)
        n_class = start.numel() - 1
        work = self._workspace(self.lib.svk_class_scatter_workspace_bytes(n_rows, dim, n_class))
        mean = torch.empty((n_class, dim), dtype=torch.float64, device=self.device)
        sw = torch.empty((dim, dim), dtype=torch.float64, device=self.device)
        self._stream()
        check(self.lib.svk_class_scatter(self.ctx, self._ptr(x), n_rows, dim, self._ptr(start), self._ptr(index), n_class,
                                         int(bool(l2_rows)), self._ptr(work), work.numel(), self._ptr(mean), self._ptr(sw)),
              self.ctx)
        return mean, sw

    def embedding_project(self, emb, mean=None, w=None, l2_in=False, l2_out=False):
        """svk_embedding_project: y = l2_out((l2_in(x) - mean) @ w) for every row of emb [n, dim] -> float32 [n, out_dim] on the
        device in one pass.  mean: None or [dim]; w: None (the identity) or [dim, out_dim], out_dim <= dim <= 512.  The norms
        are float64, the product is f32 on the matrix pipe; a row's bits depend on that row alone."""
        torch = _torch()
        x = self.to_device(emb, torch.float32)
        if x.dim() != 2:
            raise ValueError("embedding_project wants rows (n, dim)")
        n, dim = int(x.shape[0]), int(x.shape[1])
        mu = None
        if mean is not None:
            mu = self.to_device(mean, torch.float32).reshape(-1)
            if mu.numel() != dim:
                raise ValueError("mean holds one entry per column of emb")
        out_dim, wt = dim, None
        if w is not None:
            wt = self.to_device(w, torch.float32)
            if wt.dim() != 2 or int(wt.shape[0]) != dim:
                raise ValueError("w wants (dim, out_dim)")
            out_dim = int(wt.shape[1])
        out = torch.empty((n, out_dim), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_embedding_project(self.ctx, self._ptr(x), n, dim, self._ptr(mu), self._ptr(wt), out_dim,
                                             int(bool(l2_in)) | 2 * int(bool(l2_out)), self._ptr(out)), self.ctx)
        return out

    PAIR_METRICS = {"cosine": 0, "l2": 1}

    def pair_scores(self, a, b, idx_a, idx_b, metric="cosine", bad_count=None):
        """svk_pair_scores: out[p] = score of a[idx_a[p]] against b[idx_b[p]] for a trial list -> float32 [n_pairs] on the
        device.  metric: "cosine", or "l2" = -||x - y|| (larger = same speaker); b may be a itself.  An index outside its matrix
        gives NaN at that trial and counts in bad_count (an int32 [1] device tensor the caller zeroes), if given."""
        torch = _torch()
        if metric not in self.PAIR_METRICS:
            raise ValueError("metric must be 'cosine' or 'l2', got %r" % (metric,))
        x, y = self._two_matrices(a, b, "pair_scores")
        ia, ib, bad_count = self._trials(idx_a, idx_b, bad_count)
        out = torch.empty((ia.numel(),), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_pair_scores(self.ctx, self._ptr(x), x.shape[0], self._ptr(y), y.shape[0], x.shape[1], self._ptr(ia),
                                       self._ptr(ib), ia.numel(), self.PAIR_METRICS[metric], self._ptr(out),
                                       self._ptr(bad_count)), self.ctx)
        return out

    def _plda_operands(self, psi, counts, dim, n_enroll):
        """psi as float64 [dim] and the counts as int32 [n_enroll] (or None) on the device, shapes checked (not the values:
        `plda.Plda` validates those on the host)."""
        torch = _torch()
        p = self.to_device(psi, torch.float64).reshape(-1)
        if p.numel() != dim:
            raise ValueError("psi holds one entry per column of the projected rows (%d), got %d" % (dim, p.numel()))
        cnt = None
        if counts is not None:
            cnt = self.to_device(counts, torch.int32).reshape(-1)
            if cnt.numel() != n_enroll:
                raise ValueError("counts holds one entry per enrolled row (%d), got %d" % (n_enroll, cnt.numel()))
        return p, cnt

    def plda_scores(self, test, enroll, psi, counts=None):
        """svk_plda_scores: the PLDA log-likelihood ratio of every PROJECTED test row [Nt, D] against every enrolled model
        [Ns, D] (the mean of counts[j] >= 1 projected utterances; None: 1 each) -> float32 [Nt, Ns] on the device.  psi:
        float64 [D], the between-speaker variances (`plda.Plda`).  A float64 pre-pass and one f32 MFMA product; the workspace
        is a torch allocation sized by the library."""
        torch = _torch()
        t, e = self._two_matrices(test, enroll, "plda_scores")
        nt, ns, dim = int(t.shape[0]), int(e.shape[0]), int(t.shape[1])
        p, cnt = self._plda_operands(psi, counts, dim, ns)
        work = self._workspace(self.lib.svk_plda_scores_workspace_bytes(nt, ns, dim, int(cnt is not None)))
        out = torch.empty((nt, ns), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_plda_scores(self.ctx, self._ptr(t), nt, self._ptr(e), ns, dim, self._ptr(p), self._ptr(cnt),
                                       self._ptr(work), work.numel(), self._ptr(out)), self.ctx)
        return out

    def plda_pair_scores(self, a, b, idx_a, idx_b, psi, counts_b=None, bad_count=None):
        """svk_plda_pair_scores: out[p] = the PLDA log-likelihood ratio of the test row a[idx_a[p]] against the enrolled model
        b[idx_b[p]] (of counts_b[idx_b[p]] utterances; None: 1) -> float32 [n_pairs] on the device, float64 arithmetic.  b may
        be a itself.  An index outside its matrix gives NaN at that trial and counts in bad_count (an int32 [1] device tensor
        the caller zeroes), if given."""
        torch = _torch()
        x, y = self._two_matrices(a, b, "plda_pair_scores")
        ia, ib, bad_count = self._trials(idx_a, idx_b, bad_count)
        p, cnt = self._plda_operands(psi, counts_b, int(x.shape[1]), int(y.shape[0]))
        out = torch.empty((ia.numel(),), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_plda_pair_scores(self.ctx, self._ptr(x), x.shape[0], self._ptr(y), y.shape[0], x.shape[1],
                                            self._ptr(p), self._ptr(cnt), self._ptr(ia), self._ptr(ib), ia.numel(),
                                            self._ptr(out), self._ptr(bad_count)), self.ctx)
        return out

    def _search_lists(self, n, k, exclude, into):
        """The operands `cosine_topk` and `cosine_topk_norm` share: (exclude as int64 [n] on the device or None, scores,
        indices), the two lists fresh or the caller's `into`."""
        torch = _torch()
        ex = None
        if exclude is not None:
            ex = self.to_device(exclude, torch.int64).reshape(-1)
            if ex.numel() != n:
                raise ValueError("exclude holds one index per query row")
        if into is None:
            scores = torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device)
            indices = torch.empty((n, max(k, 0)), dtype=torch.int64, device=self.device)
        else:
            scores, indices = into
            for t, dt in ((scores, torch.float32), (indices, torch.int64)):
                self._given_out(t, (n, k), dt, "into wants contiguous device tensors (float32 [n, k], int64 [n, k])")
        return ex, scores, indices

    def cosine_topk(self, query, gallery, k, exclude=None, index_base=0, into=None):
        """svk_cosine_topk: the k best gallery rows of every query row by cosine score, without the score matrix ->
        (scores float32 [n, k], indices int64 [n, k]) on the device, best first; an index is index_base + the gallery row,
        empty slots hold -1 / -inf.  Higher score first, NaN above every number, the lower index among equal scores.
        exclude: int64 [n], the global index that is no candidate for each query (a self-search).  into=(scores, indices):
        accumulate into those tensors (lists of earlier calls over other chunks of the gallery, disjoint index ranges); the
        result equals one call over the whole gallery bit for bit.  The workspace is a torch allocation sized by the library."""
        q, g = self._two_matrices(query, gallery, "cosine_topk")
        n, ng, dim, k = int(q.shape[0]), int(g.shape[0]), int(q.shape[1]), int(k)
        ex, scores, indices = self._search_lists(n, k, exclude, into)
        work = self._workspace(self.lib.svk_cosine_topk_workspace_bytes(n, ng, dim, k))
        self._stream()
        check(self.lib.svk_cosine_topk(self.ctx, self._ptr(q), n, self._ptr(g), ng, dim, k, int(index_base), self._ptr(ex),
                                       0 if into is None else 1, self._ptr(work), work.numel(), self._ptr(scores),
                                       self._ptr(indices)), self.ctx)
        return scores, indices

    def cosine_topk_norm(self, query, gallery, k, query_moments=None, gallery_moments=None, exclude=None, index_base=0, into=None):
        """svk_cosine_topk_norm: `cosine_topk` ranked by the NORMALISED score -- `score_norm`'s expression on the cosine, bit
        for bit, inside the selection; the score matrix is never written -> (normalised scores float32 [n, k], indices int64
        [n, k]) on the device.  query_moments float64 [n, 2] (the T-norm side, `score_norm`'s row table), gallery_moments
        float64 [n_gallery, 2] of THIS call's gallery rows (the Z-norm side, the column table), as `cohort_moments` returns
        them; one of the two may be None, not both (that is `cosine_topk`).  exclude, index_base and into as in `cosine_topk`;
        the lists in `into` hold normalised scores."""
        q, g = self._two_matrices(query, gallery, "cosine_topk_norm")
        n, ng, dim, k = int(q.shape[0]), int(g.shape[0]), int(q.shape[1]), int(k)
        qm, gm = self._moments(query_moments, n, "query_moments"), self._moments(gallery_moments, ng, "gallery_moments")
        # an empty tensor has no address, and the entry tells a given table by its address: an empty side (a chunk without
        # rows) hands over one spare pair, of which the entry reads nothing
        qm, gm = (m.new_empty((1, 2)) if m is not None and m.shape[0] == 0 else m for m in (qm, gm))
        ex, scores, indices = self._search_lists(n, k, exclude, into)
        work = self._workspace(self.lib.svk_cosine_topk_norm_workspace_bytes(n, ng, dim, k))
        self._stream()
        check(self.lib.svk_cosine_topk_norm(self.ctx, self._ptr(q), n, self._ptr(g), ng, dim, k, int(index_base), self._ptr(ex),
                                            0 if into is None else 1, self._ptr(qm), self._ptr(gm), self._ptr(work),
                                            work.numel(), self._ptr(scores), self._ptr(indices)), self.ctx)
        return scores, indices

    def knn_cluster(self, nbr_score, nbr_index, k=None, *, threshold, min_shared=0, mutual=True, min_size=1):
        """svk_knn_cluster (include/svk.h, "shared-neighbour (Jarvis-Patrick) clustering of k-NN lists"): the connected components of the shared-neighbour graph read off the k-NN
        lists of a self-search (`cosine_topk(x, x, k, exclude=arange(n))`: float32 / int64 [n, list_stride]) -> (labels int32
        [n], roots int32 [n], sizes int32 [n], counts int32 [4]) on the device.  Only the first k slots of a row count (None:
        all of them).  An edge {i, j} needs the arcs i -> j and j -> i (mutual; either one otherwise), an arc a slot with
        score >= threshold (float32; -inf: every slot), and at least min_shared common neighbours.  roots[i] is the smallest
        row of i's component; components of at least min_size rows are labelled 0 .. C-1 by their smallest member, the other
        rows -1; sizes holds the C cluster sizes, then zeros; counts = (C, rows labelled -1, bad slots, gave_up)."""
        torch = _torch()
        sc, ix = self.to_device(nbr_score, torch.float32), self.to_device(nbr_index, torch.int64)
        if sc.dim() != 2 or tuple(sc.shape) != tuple(ix.shape):
            raise ValueError("knn_cluster wants the two lists of a search: float32 [n, list_stride] and int64 [n, list_stride]")
        n, stride = int(sc.shape[0]), int(sc.shape[1])
        k = stride if k is None else int(k)
        labels, roots, sizes = (torch.empty((n,), dtype=torch.int32, device=self.device) for _ in range(3))
        counts = torch.empty((4,), dtype=torch.int32, device=self.device)
        work = self._workspace(self.lib.svk_knn_cluster_workspace_bytes(n, k))
        self._stream()
        check(self.lib.svk_knn_cluster(self.ctx, self._ptr(sc), self._ptr(ix), n, k, stride, float(threshold), int(min_shared),
                                       int(min_size), _lib.KNN_CLUSTER_MUTUAL if mutual else 0, self._ptr(work), work.numel(),
                                       self._ptr(labels), self._ptr(roots), self._ptr(sizes), self._ptr(counts)), self.ctx)
        return labels, roots, sizes, counts

    def l2_dist(self, a, b):
        torch = _torch()
        a, b = self._two_matrices(a, b, "l2_dist")
        if a.shape != b.shape:
            raise ValueError("l2_dist wants two (n, D) matrices")
        out = torch.empty((a.shape[0],), dtype=torch.float32, device=self.device)
        self._stream()
        check(self.lib.svk_l2_dist(self.ctx, self._ptr(a), self._ptr(b), a.shape[0], a.shape[1], self._ptr(out)),
              self.ctx)
        return out

    # ---- audio ingest ------------------------------------------------------------
    def resample(self, pcm, up, down, taps, lengths=None, out_dtype="f32"):
        """svk_ingest_resample: pcm int16 [n_utt, frames] or [n_utt, frames, channels] -> mono
        [n_utt, ceil(frames * up / down)] float32 in [-1, 1) or int16, plus the per-clip lengths."""
        torch = _torch()
        x = self.to_device(pcm)
        if x.dtype != torch.int16 or x.dim() not in (2, 3):
            raise ValueError("resample wants int16 PCM shaped (n_utt, frames) or (n_utt, frames, channels)")
        n_utt, n_in = int(x.shape[0]), int(x.shape[1])
        n_ch = int(x.shape[2]) if x.dim() == 3 else 1
        taps = np.asarray(taps, dtype=np.float32)
        key = (int(up), int(down), taps.size, float(taps[taps.size // 2]))
        cache = self.__dict__.setdefault("_resample_taps", {})
        if key not in cache:                         # the FIR is a per-ratio table: upload it once
            cache[key] = self.to_device(taps)
        h = cache[key]
        lens = self.to_device(np.asarray(lengths, dtype=np.int32)) if lengths is not None else None
        n_out = (n_in * up + down - 1) // down
        dt = {"f32": (torch.float32, _lib.PCM_F32), "i16": (torch.int16, _lib.PCM_I16)}[out_dtype]
        out = torch.empty((n_utt, max(n_out, 1)), dtype=dt[0], device=self.device)
        out_len = torch.empty((n_utt,), dtype=torch.int32, device=self.device)
        self._stream()
        check(self.lib.svk_ingest_resample(self.ctx, self._ptr(x), n_ch, n_in, self._ptr(lens), n_in, n_utt,
                                           self._ptr(h), int(h.numel()), int(up), int(down), self._ptr(out), dt[1],
                                           int(out.shape[1]), n_out, self._ptr(out_len)), self.ctx)
        return out[:, :n_out], out_len


_engines = {}


def get_engine(device=None):
    """Process-wide engine for `device` (default: torch's current CUDA device)."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("speaker_verification_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    index = torch.cuda.current_device() if device is None else int(device)
    eng = _engines.get(index)
    if eng is None:
        eng = _engines[index] = Engine(index)
    return eng
