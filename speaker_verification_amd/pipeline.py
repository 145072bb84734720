"""End-to-end hot path on one GPU: 16 kHz PCM -> energy VAD -> log-mel front end
(-> CMVN) -> 20 x 80 x 40 feature cube -> C3D2 embedding -> cosine scores.  A three-channel model (constants.DERIVATIVE:
static, delta, delta-delta) gets its channels from the static features inside the same two steps: one statistics pass
(`svk_delta_cmvn_stats`) and one writing pass (`svk_delta_planes`, or `svk_cube_gather_delta` on the ragged paths).

This is the batched, device-resident form of what the reference does one
utterance at a time on the host:
  vad.py:135-168  ->  load_data.py:50-87  ->  utils.py:351-397  ->
  model.py:141-170  ->  evaluation.py:67-84.
Every stage is a libsvk.so kernel, the C3D2 forward included (`svk_c3d2_stage1`, `svk_c3d2_stage2`,
`svk_c3d2_conv31/32t/41/42`, `svk_c3d2_fc5`: `model.FusedEmbedder`); PyTorch-ROCm serves as device memory, streams and
the module checkpoints load into.
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import torch

from . import _lib
from . import constants as c
from .engine import get_engine, spec_from_seconds


def _timed(spans, name, fn):
    """fn() between two timing HIP events on the current stream, kept in `spans`: spans[name] = (start, end) in a dict,
    (name, start, end) appended to a list; just fn() when spans is None."""
    if spans is None:
        return fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    if isinstance(spans, dict):
        spans[name] = (start, end)
    else:
        spans.append((name, start, end))
    return out


class _Upload:
    """Host -> device copies, issued in order from a helper thread on `stream`: a pageable copy holds its calling thread,
    and the caller's thread keeps launching kernels meanwhile.  copies: (device dst, host src) pairs.  With `slots`, the
    destinations repeat every `slots` copies: copy k is issued once the caller has released copy k - slots and runs once
    the GPU has done the kernels queued before that release.  A failure in the helper is raised in the caller's `wait`;
    leaving the `with` block releases everything (the helper never waits for a caller that failed) and joins the helper."""

    def __init__(self, stream, copies, slots=0):
        self.stream, self.slots = stream, slots
        self.main = torch.cuda.current_stream(stream.device)
        self.copied = [torch.cuda.Event() for _ in copies]
        self.consumed = [torch.cuda.Event() for _ in copies]
        self.issued = [threading.Event() for _ in copies]
        self.released = [threading.Event() for _ in copies]
        self.failure = []
        stream.wait_stream(self.main)        # destinations may outlive a call: kernels queued before may still read them
        self.worker = threading.Thread(target=self._run, args=(copies,), daemon=True)
        self.worker.start()

    def _run(self, copies):
        try:
            with torch.cuda.stream(self.stream):
                for k, (dst, src) in enumerate(copies):
                    if self.slots and k >= self.slots:
                        self.released[k - self.slots].wait()
                        self.stream.wait_event(self.consumed[k - self.slots])
                    dst.copy_(src, non_blocking=True)
                    self.copied[k].record(self.stream)
                    self.issued[k].set()
        except BaseException as err:
            self.failure.append(err)
            for ev in self.issued:
                ev.set()

    def wait(self, k):
        """Order the caller's stream behind copy k."""
        self.issued[k].wait()
        if self.failure:
            raise self.failure[0]
        self.main.wait_event(self.copied[k])

    def release(self, k):
        """The kernels that read copy k are queued: its destination may take copy k + slots once they have run."""
        self.consumed[k].record(self.main)
        self.released[k].set()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for ev in self.released:
            ev.set()
        self.worker.join()


def clips_per_chunk(micro_batch, cubes_per_clip):
    """`micro_batch` counts CUBES (it sizes the network's launches); with K cubes per clip a chunk holds micro_batch // K clips,
    at least one."""
    return max(1, int(micro_batch) // int(cubes_per_clip))


def speaker_segments(speaker_ids):
    """The host half of `enroll_mean`: (sorted unique ids, CSR offsets int64 [S + 1], row index int64 [n]) -- speaker s's
    utterances are rows row_index[seg_start[s] : seg_start[s + 1]], in the order they were listed (a stable sort of the ids)."""
    speaker_ids = np.asarray(speaker_ids)
    row_index = np.argsort(speaker_ids, kind="stable").astype(np.int64)
    uniq, counts = np.unique(speaker_ids, return_counts=True)
    seg_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return uniq, seg_start, row_index


class VerificationPipeline:
    def __init__(self, model, use_vad=True, vad_threshold=c.VAD_ENERGY_THRESHOLD, normalize=c.NORMALIZE,
                 crop_seed=12345, micro_batch=1024, preemph_cof=None, crop_rng="reference", overlap_front=False,
                 pcm_scale=1.0 / 32768.0, cubes_per_clip=1, pool="mean", backend=None, plda=None,
                 calibration=None, score_norm=None, vad=None):
        """model: a `model.C3D2` with one channel, or with three (static, delta, delta-delta features: utils.py:325-348,
        :382-397; every method then carries [n, 3, T, 40] feature rows and [n, 3, 20, 80, 40] cubes): its inference form is
        `model.fused_inference()`, seven libsvk kernels.  Any other channel count raises ValueError.
        crop_rng: "reference" draws crop starts on the host exactly like utils.py:372 (needs the
        per-clip frame counts on the host: one small D2H per micro-batch); "device" draws them
        in a kernel keyed by (crop_seed, global clip index) -- no host round trip.
        preemph_cof: fuse processing.preemphasis(clip, cof=...) in front of the log-mel stage.
        pcm_scale: amplitude factor on the int16 PCM before the front end.  The reference's model path
        reads audio with librosa (utils.py:170-173): float32 in [-1, 1) = int16 / 32768 -> lmfe
        (load_data.py:50-70), and ships NORMALIZE = False, so a reference-format checkpoint expects
        log-mel values of THAT scale (2 ln 32768 = 20.79 below those of raw int16 amplitudes).  The
        default reproduces it (a power of two folded into the filterbank weights: exact); 1.0 gives
        speechpy-on-raw-int16 values.
        overlap_front: run VAD, front end, CMVN and the crop draw of micro-batch k+1 on a second HIP stream
        while the network runs on micro-batch k (device-drawn crops only).
        cubes_per_clip: K cubes (K x 20 crops) of every clip instead of the reference's one; every embed method still returns
        ONE row per clip, the float64 mean of the clip's K embeddings (pool="mean") or of its L2-normalised embeddings
        (pool="mean_l2"), svk_embedding_pool.  The clip's feature rows are read K times by the first block, never copied.
        `micro_batch` keeps counting cubes: a chunk holds `clips_per_chunk(micro_batch, K)` clips.  crop_rng="device" draws
        20 K starts per clip (the first 20 are the one-cube draw), "reference" calls randint(T - 80, size=20) K times per clip,
        in clip order.  K = 1 (the default) is today's path: no pooling, the same kernels, the same results.
        backend: a fitted `backend.EmbeddingBackend`, or None.  With one, `score`, `search` and `score_trials` project both
        sides (`project`: centre, LDA / WCCN / whitening, length norm -- svk_embedding_project) before they compare them; the
        embed methods keep returning raw embeddings.  None (the default) changes no code path.
        plda: a fitted `plda.Plda` (fitted on what the back end returns, if there is one), or None.  With one, `project` applies
        the back end and then the PLDA projection, and `score` / `score_trials` return PLDA log-likelihood ratios
        (svk_plda_scores / svk_plda_pair_scores) instead of cosines; `search` raises ValueError (top-k by LLR is not built).
        None (the default) changes no code path.
        calibration: a fitted one-system `calibration.Calibration` (fitted on the scores this pipeline produces: cosines, or
        with `plda` its LLRs), or None.  With one, `score` and `score_trials` return calibrated log-likelihood ratios
        (svk_calibration_apply, in place on the fresh scores) and `decide` thresholds them; `search` raises ValueError, `identify`
        ranks by the calibrated score.  None (the default) changes no code path.
        score_norm: a `score_norm.ScoreNorm` fitted on a cohort with this pipeline's `backend` and `plda`, or None.  With one,
        `score` and `score_trials` normalise between the raw score and the calibration (svk_cohort_moments of both sides
        against the cohort, then svk_score_norm / svk_score_norm_pairs in place on the fresh scores; a calibration is then one
        fitted on normalised scores); `search` raises ValueError, `identify` ranks by the normalised score (svk_cosine_topk_norm).
        None (the default) changes no code path.
        vad: a `vad.AdaptiveEnergyVad`, or None.  With one, `voiced` and `vad` -- and so `embed`, the ragged and arena paths and
        `diarize` -- decide by the level-adaptive rule (svk_vad_adaptive: thresholds from each clip's own frame-energy
        quantiles) and `vad_threshold` is unused; together with use_vad=False it is a ValueError.  None (the default) is the
        absolute rule: the same code path and the same bits as before."""
        if vad is not None and not use_vad:
            raise ValueError("vad= names the rule the VAD decides by; with use_vad=False there is no VAD to hand it to")
        if vad is not None and not all(hasattr(vad, k) for k in ("floor_q16", "peak_q16", "above_floor_q16", "below_peak_q16",
                                                                 "min_threshold")):
            raise ValueError("vad must be a vad.AdaptiveEnergyVad or None, got %r" % (vad,))
        self.adaptive_vad = vad
        self.channels = int(getattr(model, "num_channels", 0))
        if self.channels not in (1, 3):
            raise ValueError("VerificationPipeline runs C3D2 models with 1 or 3 input channels, got num_channels = %r"
                             % (getattr(model, "num_channels", None),))
        self.eng = get_engine()
        # bench.py sets this to a list: one {kernel name: (start, end) HIP events on the launch stream, "cubes": n} per
        # micro-batch, around every network kernel
        self.kernel_events = None
        self.model = model.to(self.eng.device).eval()
        self.refresh_model()
        self.use_vad, self.vad_threshold, self.normalize = use_vad, int(vad_threshold), bool(normalize)
        self.micro_batch = int(micro_batch)
        self.cubes_per_clip = int(cubes_per_clip)
        if self.cubes_per_clip < 1 or pool not in ("mean", "mean_l2"):
            raise ValueError("cubes_per_clip must be at least 1 and pool 'mean' or 'mean_l2', got %r, %r" % (cubes_per_clip, pool))
        self.pool = pool
        self.backend = backend
        self.plda = plda
        if calibration is not None and calibration.n_sys != 1:
            raise ValueError("the pipeline scores one system: its calibration must be fitted on one, not %r" % (calibration.n_sys,))
        self.calibration = calibration
        if score_norm is not None:
            score_norm.check_scorer(backend, plda)
        self.score_norm = score_norm
        # model front end: lmfe(signal, 16000, 0.025, 0.01, 40, 1024)  (load_data.py:64-70, Q14)
        self.spec = spec_from_seconds(c.SAMPLE_RATE, c.FRAME_LEN, c.FRAME_STEP, c.NUM_FFT, c.NUM_COEF, c.NUM_COEF,
                                      _lib.OUT_LMFE, preemph=preemph_cof is not None,
                                      preemph_cof=0.0 if preemph_cof is None else preemph_cof,
                                      input_scale=float(pcm_scale))
        assert crop_rng in ("reference", "device")
        self.crop_rng, self.crop_seed = crop_rng, int(crop_seed)
        self.bad_clips = torch.zeros((1,), dtype=torch.int32, device=self.eng.device)
        # the reference seeds the global NumPy RNG at utils import (utils.py:15) and draws
        # the crop starts from it (utils.py:372); a private RandomState keeps that sequence
        self.rng = np.random.RandomState(crop_seed)
        self.last_stats = {}
        self.overlap_front = bool(overlap_front)
        self._stream_pair, self._buffers, self._packers = None, {}, None       # made on first use, kept across calls

    def refresh_model(self):
        """Re-snapshot the (BN-folded) inference weights after the model's state changed."""
        self.embedder = self.model.fused_inference()

    def chunks(self, n):
        """(lo, hi) micro-batches of ONE size where possible: the count is ceil(n / micro_batch),
        the size ceil(n / count), and the last one is shifted back to keep that size (it redoes
        a few clips of its neighbour): every launch sequence sees the same shapes."""
        if n <= 0:
            return []
        count = -(-n // clips_per_chunk(self.micro_batch, getattr(self, "cubes_per_clip", 1)))
        size = -(-n // count)
        spans = [(k * size, min(n, (k + 1) * size)) for k in range(count)]
        lo, hi = spans[-1]
        # (the host RNG of crop_rng="reference" is consumed in clip order: no re-done clips there)
        if hi - lo < size and n >= size and self.crop_rng != "reference":
            spans[-1] = (n - size, n)
        return spans

    # ---- stages ----------------------------------------------------------------------
    def ingest(self, pcm, fs_in, lengths=None):
        """Recordings at another rate / with several channels -> what `embed` takes: int16 mono at
        16 kHz on the device (+ lengths).  pcm: int16 [n, frames] or [n, frames, channels]
        (utils.py:170-173's `librosa.load(..., sr=16000, mono=True)`, batched; ingest.py)."""
        from . import ingest as _ingest
        return _ingest.resample_batch(pcm, fs_in, c.SAMPLE_RATE, lengths=lengths, out_dtype="i16", engine=self.eng)

    def voiced(self, pcm):
        """[n, L] int16 -> (packed voiced samples [n, L] int16, voiced_len [n] i32)."""
        if not self.use_vad:
            return pcm, None
        res = self._run_vad(pcm, compact=True)
        return res["voiced"], res["voiced_len"]

    def _run_vad(self, pcm, **kw):
        """The pipeline's VAD rule on its frame geometry: the absolute threshold, or the `vad=` the pipeline was built with."""
        kw.update(fs=c.SAMPLE_RATE, frame_ms=c.VAD_FRAME_MS, padding_ms=c.VAD_PADDING_MS)
        if self.adaptive_vad is not None:
            return self.eng.vad_adaptive(pcm, self.adaptive_vad, **kw)
        return self.eng.vad_energy(pcm, self.vad_threshold, **kw)

    def vad(self, pcm, lengths=None, offsets=None, longest=None):
        """The energy VAD WITHOUT the compaction copy: (voiced_len [n] i32, gather) where gather = (src_frame, frame_samples)
        lets the front end read the kept frames where they lie (`features(pcm, voiced_len, gather)`); (None, None) when the
        pipeline runs without VAD.  `voiced()` is the copying form (packed samples, for callers that want them)."""
        if not self.use_vad:
            return (None if lengths is None else lengths), None
        res = self._run_vad(pcm, lengths=lengths, offsets=offsets, compact="index", longest=longest)
        return res["voiced_len"], (res["src_frame"], res["frame_samples"])

    def features(self, pcm, lengths=None, gather=None):
        """-> (feature rows, n_frames): [n, T, 40], or [n, 3, T, 40] for a three-channel model (static, delta, delta-delta,
        each CMVN-normalised by itself with `normalize`: utils.py:385-395) -- statistics and planes straight from the static
        features, no delta plane in between."""
        feat, n_frames, _ = self.eng.features(pcm, self.spec, lengths=lengths, gather=gather)
        if self.channels == 3:
            stats = self.eng.delta_cmvn_stats(feat, n_frames, variance=True) if self.normalize else None
            return self.eng.delta_planes(feat, n_frames, stats=stats), n_frames
        if self.normalize:                                 # utils.CMVN with c.NORMALIZE (utils.py:394-395)
            self.eng.cmvn_(feat, n_frames, variance=True)
        return feat, n_frames

    def draw_crops(self, n_frames_host):
        """idx = randint(T - 80, size=20) per utterance, in order (utils.py:372, Q15) -> [n, 20]; with K = cubes_per_clip > 1
        that draw K times per utterance, clip-major (draw[u, 0], then draw[u, 1], ...) -> [n, K, 20]."""
        K = self.cubes_per_clip
        out = np.empty((len(n_frames_host), K, c.CUBE_CROPS), dtype=np.int32)
        for i, T in enumerate(n_frames_host):
            if T - c.CUBE_FRAMES <= 0:
                raise ValueError(f"utterance {i} has {T} feature frames; FeatureCube needs more than "
                                 f"{c.CUBE_FRAMES} (numpy randint: low >= high)")
            for k in range(K):
                out[i, k] = self.rng.randint(int(T) - c.CUBE_FRAMES, size=c.CUBE_CROPS)
        return out[:, 0] if K == 1 else out

    def cubes(self, feat, crop_idx, stats=None):
        """feature rows + crop starts -> cubes [n, channels, 20, 80, 40].  Three-channel model: `feat` is either the planes
        `features` returns ([n, 3, T, 40]: only rows move -- the planes read as 3 n clips, each clip's starts three times) or
        STATIC features [n, T, 40] (+ `stats` of delta_cmvn_stats): the channels are formed for the cropped rows only.
        Crop starts [n, K, 20] -> [n, K, channels, 20, 80, 40] by the same gather kernels on the table read as [n, 20 K]: a view
        for one channel, one permute for three."""
        if getattr(crop_idx, "ndim", 2) == 3:
            idx = self.eng.to_device(crop_idx, torch.int32)
            n, K = idx.shape[0], idx.shape[1]
            if K < 1:
                raise ValueError("crop starts [n, K, 20] need K >= 1")
            wide = self.cubes(feat, idx.reshape(n, K * idx.shape[2]), stats)       # [n, channels, 20 K, 80, 40]
            wide = wide.view(n, self.channels, K, idx.shape[2], c.CUBE_FRAMES, wide.shape[-1])
            return wide.view(n, K, 1, *wide.shape[3:]) if self.channels == 1 else wide.permute(0, 2, 1, 3, 4, 5)
        if self.channels == 1:
            return self.eng.cube_gather(feat, crop_idx, c.CUBE_FRAMES, stats=stats)
        if feat.dim() == 3:
            return self.eng.cube_gather_delta(feat, crop_idx, c.CUBE_FRAMES, stats=stats)
        if stats is not None:
            raise ValueError("statistics apply to static features; planes are normalised already")
        n, ch, T, cols = feat.shape
        idx = self.eng.to_device(crop_idx, torch.int32).repeat_interleave(ch, dim=0)
        return self.eng.cube_gather(feat.reshape(n * ch, T, cols), idx, c.CUBE_FRAMES).view(n, ch, idx.shape[1], c.CUBE_FRAMES, cols)

    def crops_and_cubes(self, pcm, first_utt=0, want_cubes=True):
        """The crop starts `embed` would draw for `pcm` ([n, 20] int32 on the host) and, with `want_cubes`, the
        20 x 80 x 40 cubes themselves ([n, 1, 20, 80, 40], or [n, 3, 20, 80, 40] for a three-channel model; device) -- VAD, front end, CMVN, crop draw and gather only, no
        network: what BatchNorm calibration and the parity legs feed to the CPU oracle.  With cubes_per_clip = K > 1: crop starts
        [n, K, 20] and cubes [n, K, channels, 20, 80, 40]."""
        pcm = self.eng.to_device(pcm)
        crops, cubes, done = [], [], 0
        for lo, hi in self.chunks(pcm.shape[0]):
            feat, _, idx = self._front(pcm[lo:hi], first_utt + lo)
            if lo < done:                              # the shifted last chunk redoes clips lo .. done - 1: its rows replace them
                crops[-1] = crops[-1][:len(crops[-1]) - (done - lo)]
                if want_cubes:
                    cubes[-1] = cubes[-1][:len(cubes[-1]) - (done - lo)]
            done = hi
            if want_cubes:
                cubes.append(self.cubes(feat, idx))
            crops.append(idx.cpu().numpy() if hasattr(idx, "cpu") else np.asarray(idx))
        empty = (0, c.CUBE_CROPS) if self.cubes_per_clip == 1 else (0, self.cubes_per_clip, c.CUBE_CROPS)
        crops = np.concatenate(crops).astype(np.int32) if crops else np.zeros(empty, np.int32)
        return (crops, torch.cat(cubes)) if want_cubes else crops

    def embed_cubes(self, cubes):
        """[n, channels, 20, 80, 40] cubes -> [n, 128]: the cube read as feature rows by the first-block kernel (no copy)."""
        return self.embedder(cubes)

    def _pool_flag(self):
        return self.pool == "mean_l2"

    def embed_features(self, feat, crop_idx):
        """features + crop starts -> embeddings.  The cube is never materialised: `svk_c3d2_stage1` reads the
        feature rows and crop starts itself; the other six kernels follow (model.FusedEmbedder.embed_features).  Crop starts
        [n, K, 20]: K cubes per clip, pooled to one row per clip."""
        multi = getattr(crop_idx, "ndim", 2) == 3
        pool = self.pool if multi else None
        if self.kernel_events is None:
            return self.embedder.embed_features(feat, crop_idx, pool=pool)
        events = {"cubes": feat.shape[0] * (crop_idx.shape[1] if multi else 1)}
        out = self.embedder.embed_features(feat, crop_idx, partial(_timed, events), pool=pool)
        self.kernel_events.append(events)
        return out

    def _crop_starts(self, n_frames, first, crop_idx=None):
        """Crop starts of a micro-batch whose row 0 is clip `first`: the caller's `crop_idx` (host) if given, else drawn on
        the device keyed by the global clip index, else from the host RNG in clip order."""
        if crop_idx is not None:
            return np.asarray(crop_idx, dtype=np.int32)
        if self.crop_rng == "device":
            K = self.cubes_per_clip         # 20 K starts per clip, keyed by (seed, clip, c): the first 20 are the one-cube draw
            idx = self.eng.draw_crops(n_frames, K * c.CUBE_CROPS, c.CUBE_FRAMES, self.crop_seed, first, self.bad_clips)
            return idx if K == 1 else idx.view(-1, K, c.CUBE_CROPS)
        return self.draw_crops(n_frames.to("cpu").numpy())      # tiny D2H: T per utterance

    def _front(self, chunk, first, crop_idx=None):
        """The front step of a [n, L] device chunk of uniform clips whose row 0 is clip `first`: VAD (index form, nothing
        copied) -> front end -> CMVN (three-channel model: + the delta planes) -> crop starts.  Returns (feat, n_frames, crop starts)."""
        vlen, gather = self.vad(chunk)
        feat, n_frames = self.features(chunk, vlen, gather)
        return feat, n_frames, self._crop_starts(n_frames, first, crop_idx)

    # ---- whole path ---------------------------------------------------------------------
    def embed(self, pcm, crop_idx=None, return_intermediates=False, first_utt=0):
        """[n, L] int16 PCM (NumPy or CUDA tensor) -> [n, 128] float32 embeddings (device).
        `crop_idx` [n, 20] (one cube per clip) or [n, K, 20] (K cubes, pooled) overrides the RNG draw (parity tests feed both
        sides the same crops); `first_utt` is the global index of row 0 (keys the device-side crop draw)."""
        pcm = self.eng.to_device(pcm)
        emb = torch.empty((pcm.shape[0], 128), dtype=torch.float32, device=self.eng.device)
        inter = []
        spans = self.chunks(pcm.shape[0])
        if (self.overlap_front and crop_idx is None and self.crop_rng == "device" and not return_intermediates
                and len(spans) > 1):
            return self._embed_overlapped(pcm, spans, emb, first_utt)
        for lo, hi in spans:
            chunk, given = pcm[lo:hi], None if crop_idx is None else crop_idx[lo:hi]
            if return_intermediates:                       # the packed voiced samples are part of what is handed back
                voiced, vlen = self.voiced(chunk)
                feat, n_frames = self.features(voiced, vlen)
                idx = self._crop_starts(n_frames, first_utt + lo, given)
                cube = self.cubes(feat, idx)
                if cube.dim() == 6:               # [n, K, channels, 20, 80, 40]: every cube through the network, then the pool
                    each = self.embed_cubes(cube.reshape((-1,) + tuple(cube.shape[2:])))
                    emb[lo:hi] = self.eng.embedding_pool(each, rows_per_seg=cube.shape[1], l2_rows=self._pool_flag())
                else:
                    emb[lo:hi] = self.embed_cubes(cube)
                inter.append({"lo": lo, "hi": hi, "voiced": voiced, "voiced_len": vlen, "feat": feat,
                              "n_frames": n_frames, "crop_idx": idx, "cube": cube})
            else:
                feat, _, idx = self._front(chunk, first_utt + lo, given)
                emb[lo:hi] = self.embed_features(feat, idx)
        return (emb, inter) if return_intermediates else emb

    def _embed_overlapped(self, pcm, spans, emb, first_utt):
        """Two HIP streams: the side stream turns micro-batch k+1 into features + crop starts (HBM / VALU work) while the
        main stream runs the MFMA-bound network on micro-batch k."""
        main = torch.cuda.current_stream(self.eng.device)
        side = self._streams()[1]
        side.wait_stream(main)                     # whatever produced `pcm` is ordered before the side stream

        def stage(k):
            lo, hi = spans[k]
            with torch.cuda.stream(side):
                # The front step of micro-batch k runs beside the network of k - 1 and no further ahead: it waits for what the
                # main stream holds when it is queued (the network of k - 2).  Without this the side stream ran as far ahead
                # as the queue let it -- all front steps back to back when the call started behind a busy main stream -- and the
                # last micro-batch then missed the one-stream bits in 58 of 80 calls on the MI355X (a few feature rows of a
                # few clips; 0 of 40 with the wait).  Why running further ahead goes wrong is not known.
                side.wait_stream(main)
                feat, _, idx = self._front(pcm[lo:hi], first_utt + lo)
                done = torch.cuda.Event()
                done.record(side)
            return (feat, idx), done

        nxt = stage(0)
        for k, (lo, hi) in enumerate(spans):
            data, done = nxt
            if k + 1 < len(spans):
                nxt = stage(k + 1)
            main.wait_event(done)
            for t in data:
                t.record_stream(main)              # allocated on the side stream, consumed on the main one
            emb[lo:hi] = self.embed_features(*data)
        side.wait_stream(main)
        return emb

    def _ragged_batches(self, lengths, max_batch_samples, max_feature_bytes=1 << 30, max_padding=2.0):
        """Clip indices sorted by length and cut into batches of at most `micro_batch` clips and `max_batch_samples`
        samples (16-byte-aligned clip slots): a batch costs its own samples, not n x the longest clip -- up to a point: the
        front end enumerates clips x tiles-of-the-LONGEST-clip and the feature buffer is sized the same way, so a batch also
        ends where its padded size (clips x longest) would pass `max_padding` (2 by default) x its real size (the long tail of a VoxCeleb-like
        length distribution otherwise makes one batch of 12 .. 145 s clips that is 88 % padding).  NumPy throughout: the plan
        of 2 048 clips takes ~0.1 ms (a Python loop over clips took 1 ms, with the GPU idle)."""
        lengths = np.asarray(lengths, dtype=np.int64)
        n = lengths.size
        if not n:
            return []
        per_batch = clips_per_chunk(self.micro_batch, getattr(self, "cubes_per_clip", 1))
        order = np.argsort(lengths, kind="stable")
        slots = (lengths[order] + 7) // 8 * 8
        cum = np.concatenate([[0], np.cumsum(slots)])                   # cum[k] = samples of the first k sorted clips
        out, pos = [], 0
        while pos < n:
            hi = min(n, pos + per_batch)
            # the sample cap: the largest hi with cum[hi] - cum[pos] <= max_batch_samples (at least one clip)
            hi = max(pos + 1, min(hi, int(np.searchsorted(cum, cum[pos] + max_batch_samples, side="right")) - 1))
            # the padding cap: (k - pos) * slots[k - 1] <= max_padding * (cum[k] - cum[pos]) holds at k = pos + 1; take the
            # largest such k up to hi (clips are sorted, so the padded size is clips x the last one)
            k = np.arange(pos + 1, hi + 1)
            ok = (k - pos) * slots[k - 1] <= max_padding * (cum[k] - cum[pos])
            hi = int(k[np.nonzero(ok)[0][-1]])
            out.append((order[pos:hi].tolist(), int(cum[hi] - cum[pos])))
            pos = hi
        # the longest clips would otherwise end up as batches of a handful: a dozen-workgroup front end for a few clips, and every
        # batch has fixed costs (measured, `tools/time_ragged_front.py`: the ONE 145 s clip of the benchmark's 2 048 cost 0.15 ms
        # of VAD + front end + CMVN, as much as 300 clips of 7 s).  A last batch of fewer than 64 clips joins its predecessor
        # (repeatedly) -- when the merged batch stays within `micro_batch` clips, 1.5 x the sample cap, a feature buffer (clips x
        # the LONGEST clip's frames x 40 floats) of `max_feature_bytes` (joining 145 s clips to a full batch of 20 s ones would
        # multiply that buffer), and either the padding cap or a padded size no larger than a full batch's REAL size: tiles past
        # a clip's end leave the front end at once, and a small batch's padding is cheaper than a batch of its own
        while len(out) >= 2 and len(out[-1][0]) < 64:
            merged = len(out[-2][0]) + len(out[-1][0])
            longest = int(lengths[out[-1][0][-1]])
            feat_bytes = merged * max(1, longest // 160) * 40 * 4
            total = out[-2][1] + out[-1][1]
            padded = merged * ((longest + 7) // 8 * 8)
            if (merged <= per_batch and total <= max_batch_samples * 3 // 2 and feat_bytes <= max_feature_bytes
                    and (padded <= max_padding * total or padded <= max_batch_samples)):
                tail = out.pop()
                out[-1] = (out[-1][0] + tail[0], out[-1][1] + tail[1])
            else:
                break
        return out

    @staticmethod
    def _upload_groups(offsets, lengths, n_samples, max_batch_samples):
        """A host arena cut into upload pieces: clips in arena order, a piece closed where the next clip would take it past
        `max_batch_samples` (a single longer clip is a piece of its own).  Returns (groups of clip indices, [lo, hi) sample
        ranges): the ranges tile [0, n_samples) and every clip lies wholly inside its group's range -- also when clips
        OVERLAP in the arena (windows over one recording): a piece ends at the furthest end of its clips, and a clip that
        starts before that point belongs to the same piece."""
        by_pos = np.argsort(offsets, kind="stable")
        starts = offsets[by_pos].astype(np.int64)
        ends = starts + lengths[by_pos]
        groups, pieces, lo, first, reach = [], [], 0, 0, 0
        for q in range(len(by_pos)):
            reach = max(reach, int(ends[q]))
            last = q + 1 == len(by_pos)
            # the next clip may open a new piece only if it starts at or past everything this piece's clips cover
            if last or (int(starts[q + 1]) >= reach and int(ends[q + 1]) - int(starts[first]) > max_batch_samples):
                hi = n_samples if last else int(starts[q + 1])
                groups.append(by_pos[first:q + 1])
                pieces.append((lo, hi))
                lo, first = hi, q + 1
        return groups, pieces

    def _ragged_front(self, dev_buf, offs, lens, longest, rows, spans=None, crops=None, cubes_per_clip=1):
        """VAD -> front end -> CMVN statistics -> crop draw of one batch of clips addressed through offsets / lengths (device
        slices) into `dev_buf`; `longest`: the batch's longest clip in samples (host int); rows: the clips' global indices
        (they key the crop draw).  Returns (RAW features [n, T, 40], crop starts [n, 20], CMVN statistics or None): the VAD
        copies nothing (the front end reads the kept frames where they lie, svk_frontend_run's d_src_chunk) and the
        normalisation (utils.py:382-397) is applied by the cube gather to the 20 x 80 rows the network reads, not to every row
        of a clip.  A three-channel model gets the same RAW static features and the statistics of its three channels
        ([n, 3, 2, 40], svk_delta_cmvn_stats): the gather forms the delta channels for the rows it copies, and no per-clip
        plane is ever written.  Nothing here touches the host.  With K = cubes_per_clip cubes per clip the crop starts are
        [n, 20 K] (clip-major: cube k of a clip is columns 20 k .. 20 k + 19); `crops`: the caller's starts in that shape (device)
        instead of a draw."""
        timed = partial(_timed, spans)
        dev_lens, gather = lens, None
        if self.use_vad:
            dev_lens, gather = timed("vad", lambda: self.vad(dev_buf, lengths=lens, offsets=offs, longest=longest))
        # (at least one crop's worth of rows: the gathers refuse a feature buffer shorter than a crop, and a batch may hold
        # nothing but clips that are too short to crop -- their starts are -1, their cubes zeros, rows past n_frames are zeros)
        max_frames = max(self.spec.num_frames(int(longest)), c.CUBE_FRAMES)
        feat, n_frames, _ = timed("frontend", lambda: self.eng.features(dev_buf, self.spec, lengths=dev_lens, offsets=offs,
                                                                         max_frames=max_frames, gather=gather))
        cmvn_stats = self.eng.delta_cmvn_stats if self.channels == 3 else self.eng.cmvn_stats
        stats = timed("cmvn", lambda: cmvn_stats(feat, n_frames, variance=True)) if self.normalize else None
        idx = crops if crops is not None else timed("crops", lambda: self.eng.draw_crops(
            n_frames, cubes_per_clip * c.CUBE_CROPS, c.CUBE_FRAMES, self.crop_seed, 0, self.bad_clips, utt_index=rows))
        return feat, idx, stats

    class _CubeRing:
        """Length-sorted batches are what the front end wants (their feature buffers are sized by the longest clip) and what
        the network does NOT want: the batch of the longest clips is a few dozen cubes, and a persistent kernel that works on
        16-cube groups leaves most of the chip idle there (measured: 0.45 ms of fixed cost per such batch).  So every batch
        leaves only its gathered cubes (the 20 x 80 rows the network will read: 256 KB per clip, utils.py:351-379) in a RING
        of 2 x `step` cubes, and the network runs over `step` cubes as soon as that many have gathered; the first block reads
        the ring as feature rows with crop starts 0, 80, 160 ...  Memory is O(step), whatever the number of clips.
        With K cubes per clip a clip leaves K consecutive cubes (crop starts [n, 20 K]: the gather's [n, C, 20 K, 80, 40] is
        [n K, 1, 20, 80, 40] as it lies for one channel, one permuting copy away for three); `step` is rounded up to a multiple
        of K so that no clip straddles the ring's end, and `emb` / `order_dev` are per CUBE."""

        def __init__(self, pipe, step, emb, order_dev, spans, cubes_per_clip=1):
            self.K = int(cubes_per_clip)
            step = -(-int(step) // self.K) * self.K
            self.pipe, self.step, self.cap = pipe, step, 2 * step
            self.emb, self.order, self.spans = emb, order_dev, spans
            self.channels = getattr(pipe, "channels", 1)       # 3: the ring holds three-channel cubes
            hit = getattr(pipe, "_ring_buf", None)
            if hit is None or tuple(hit.shape[:2]) != (self.cap, self.channels):
                hit = pipe._ring_buf = torch.empty((self.cap, self.channels, c.CUBE_CROPS, c.CUBE_FRAMES, c.NUM_COEF),
                                                   dtype=torch.float32, device=pipe.eng.device)
            self.cubes = hit
            # what the first block reads: [cap, 1 600, 40] rows, [cap, 3, 1 600, 40] for a three-channel model
            self.rows = hit.view((self.cap,) + ((3,) if self.channels == 3 else ()) + (c.CUBE_CROPS * c.CUBE_FRAMES, c.NUM_COEF))
            self.at = self.done = 0            # cubes gathered / handed to the network so far (absolute counts)

        def push(self, feat, idx, stats=None):
            n, K = feat.shape[0], self.K
            assert n * K <= self.step, "a batch must not exceed the network step"
            w = self.at % self.cap
            first = min(n, (self.cap - w) // K)           # clips in front of the ring's end

            # three-channel model: the static rows become the three-channel cube on the way (svk_cube_gather_delta)
            cube_gather = self.pipe.eng.cube_gather_delta if self.channels == 3 else self.pipe.eng.cube_gather
            if K > 1 and self.channels == 3:
                def cube_gather(f, i, frames, out, stats):      # [m, 3, 20 K, 80, 40] -> the ring's [m K, 3, 20, 80, 40]
                    wide = self.pipe.eng.cube_gather_delta(f, i, frames, stats=stats)
                    out.view(f.shape[0], K, 3, c.CUBE_CROPS, frames, wide.shape[-1]).copy_(
                        wide.view(f.shape[0], 3, K, c.CUBE_CROPS, frames, wide.shape[-1]).permute(0, 2, 1, 3, 4, 5))

            def gather():
                cube_gather(feat[:first], idx[:first], c.CUBE_FRAMES, out=self.cubes[w:w + first * K],
                            stats=None if stats is None else stats[:first])
                if first < n:                    # the batch wraps around the end of the ring
                    cube_gather(feat[first:], idx[first:], c.CUBE_FRAMES, out=self.cubes[:(n - first) * K],
                                stats=None if stats is None else stats[first:])
            _timed(self.spans, "gather", gather)
            self.at += n * K
            while self.at - self.done >= self.step:
                self._network(self.step)

        def _network(self, n):
            lo = self.done % self.cap              # a multiple of `step`: [lo, lo + n) never wraps

            def network():
                out = self.pipe.embed_features(self.rows[lo:lo + n], self.pipe.embedder.crop_starts(n, self.cubes.device))
                self.emb[self.order[self.done:self.done + n]] = out
            _timed(self.spans, "network", network)
            self.done += n

        def finish(self):
            if self.at > self.done:
                self._network(self.at - self.done)

    def _streams(self):
        """(upload stream, side stream), made on first use: every host -> device copy of the pipeline runs on the first, the
        front steps of the overlap form on the second."""
        if self._stream_pair is None:
            self._stream_pair = (torch.cuda.Stream(device=self.eng.device), torch.cuda.Stream(device=self.eng.device))
        return self._stream_pair

    def _staging(self, numel, pinned=False):
        """Two 1-D int16 buffers of at least `numel` samples, on the device or in pinned host memory: the upload of batch
        k + 1 fills one while the kernels read batch k from the other.  Kept across calls, grown when a call needs more."""
        bufs = self._buffers.get(pinned)
        if bufs is None or bufs[0].numel() < numel:
            bufs = self._buffers[pinned] = [torch.empty((numel,), dtype=torch.int16, pin_memory=True) if pinned else
                                            torch.empty((numel,), dtype=torch.int16, device=self.eng.device) for _ in range(2)]
        return bufs

    def _ragged_loop(self, emb, plan, offsets, lengths, step, first_utt, spans, fetch, release=None, crop_idx=None):
        """The body of both ragged forms.  plan: the clip indices of every batch, in the order they run; offsets / lengths:
        per clip, into the buffer fetch(k) returns for batch k once the current stream is ordered behind its upload;
        release(k): batch k's buffer has been read.  Embeddings land in emb[clip index].  crop_idx: the caller's crop starts,
        [n, 20] or [n, K, 20] in clip order (host), instead of the draw.  K cubes per clip: the ring and the network work on
        cubes, whose embeddings [n K, 128] are pooled to `emb` at the end."""
        dev = self.eng.device
        K = self.cubes_per_clip
        if crop_idx is not None:
            crop_idx = np.asarray(crop_idx, dtype=np.int32)
            if crop_idx.ndim not in (2, 3) or crop_idx.shape[0] != len(lengths) or crop_idx.shape[-1] != c.CUBE_CROPS:
                raise ValueError("crop_idx must be [n, 20] or [n, K, 20] for the n = %d clips" % len(lengths))
            K = crop_idx.shape[1] if crop_idx.ndim == 3 else 1
            if K < 1:
                raise ValueError("crop starts [n, K, 20] need K >= 1")
        pooled = K > 1 or (crop_idx is not None and crop_idx.ndim == 3)
        # the whole schedule goes up ONCE, before the loop: a host array handed to a launch is a synchronous copy that waits
        # for everything queued before it
        order = np.concatenate(plan).astype(np.int64)
        order_dev = torch.from_numpy(order).to(dev)
        keys_dev = order_dev + int(first_utt)
        offs_dev = torch.from_numpy(offsets[order]).to(dev)
        lens_dev = torch.from_numpy(lengths[order].astype(np.int32)).to(dev)
        crops_dev = None if crop_idx is None else torch.from_numpy(crop_idx[order].reshape(len(order), -1)).to(dev)
        if pooled:              # cube K u + k of clip u: its embedding lands in row K u + k
            emb_cubes = torch.empty((len(lengths) * K, 128), dtype=torch.float32, device=dev)
            order_cubes = (order_dev[:, None] * K + torch.arange(K, device=dev)[None, :]).reshape(-1)
        else:
            emb_cubes, order_cubes = emb, order_dev
        ring = self._CubeRing(self, max(step, K), emb_cubes, order_cubes, spans, K)
        pos = 0
        for k, ids in enumerate(plan):
            sl = slice(pos, pos + len(ids))
            feat, idx, stats = self._ragged_front(fetch(k), offs_dev[sl], lens_dev[sl], int(lengths[ids].max()), keys_dev[sl],
                                                  spans=spans, crops=None if crops_dev is None else crops_dev[sl],
                                                  cubes_per_clip=K)
            if release is not None:
                release(k)
            # the network runs as soon as a full step of cubes has gathered: its kernels then cover the host side of the
            # next batch
            ring.push(feat, idx, stats)
            pos += len(ids)
        ring.finish()
        if pooled:
            emb.copy_(_timed(spans, "pool", lambda: self.eng.embedding_pool(emb_cubes, rows_per_seg=K, l2_rows=self._pool_flag())))

    def embed_ragged(self, clips, max_batch_samples=64 * 1024 * 1024, first_utt=0, spans=None, crop_idx=None):
        """Clips of DIFFERENT lengths (VoxCeleb1 utterances run from 4 to 145 s): `clips` is a list of 1-D
        int16 arrays on the HOST.  They are sorted by length, packed back to back (16-byte aligned) into batches of
        at most `max_batch_samples` samples and `micro_batch` clips, uploaded, and addressed through the
        offsets / lengths form of the C-ABI.  Embeddings come back in the order of `clips`.  Needs crop_rng='device'.
        `spans`: a list that receives ("vad" | "frontend" | "cmvn" | "crops" | "gather" | "network", start, end) HIP events (bench.py).
        `crop_idx`: [n, 20] or [n, K, 20] crop starts in the order of `clips` (host) instead of the device draw."""
        if self.crop_rng != "device":
            raise ValueError("embed_ragged needs crop_rng='device'")
        dev = self.eng.device
        emb = torch.empty((len(clips), 128), dtype=torch.float32, device=dev)
        lengths = np.array([len(x) for x in clips], dtype=np.int64)
        batches = self._ragged_batches(lengths, max_batch_samples)
        if not batches:
            return emb
        offsets = np.empty_like(lengths)                   # of each clip in its batch's staging buffer
        for ids, _ in batches:
            slots = (lengths[ids] + 7) // 8 * 8
            offsets[ids] = np.cumsum(slots) - slots
        # Two pinned host buffers + two device buffers: batch k + 1 is packed by 8 host threads (np.copyto releases the
        # GIL) and copied on the upload stream while the GPU works on batch k -- the host-side np.zeros + clip-by-clip copy +
        # pageable upload of the first version was 8 x the GPU time of the whole workload.
        cap = max(total for _, total in batches)
        pinned, staged = self._staging(cap, pinned=True), self._staging(cap)
        threads = int(os.environ.get("SVK_RAGGED_THREADS", "8"))
        if self._packers is None or self._packers[0] != threads:
            self._packers = (threads, ThreadPoolExecutor(max_workers=threads))
        pool = self._packers[1]
        main = torch.cuda.current_stream(dev)
        upload = self._streams()[0]
        upload.synchronize()                               # a previous call's copies may still read the pinned buffers
        upload.wait_stream(main)
        copied = [torch.cuda.Event() for _ in range(2)]
        consumed = [torch.cuda.Event() for _ in range(2)]

        def fetch(k):                                      # host packing + H2D of batch k, under the kernels of batch k - 1
            ids, total = batches[k]
            slot = k & 1
            if k >= 2:
                consumed[slot].synchronize()               # the GPU is done with what this pinned / device pair held
            dst = pinned[slot].numpy()

            def put(lo, hi):
                for q in ids[lo:hi]:
                    src = np.asarray(clips[q], dtype=np.int16)
                    np.copyto(dst[offsets[q]:offsets[q] + src.size], src, casting="no")
            step = -(-len(ids) // threads)
            for job in [pool.submit(put, lo, lo + step) for lo in range(0, len(ids), step)]:
                job.result()
            with torch.cuda.stream(upload):
                staged[slot][:total].copy_(pinned[slot][:total], non_blocking=True)
                copied[slot].record(upload)
            main.wait_event(copied[slot])
            return staged[slot][:total]

        self._ragged_loop(emb, [ids for ids, _ in batches], offsets, lengths, self.micro_batch, first_utt, spans, fetch,
                          release=lambda k: consumed[k & 1].record(main), crop_idx=crop_idx)
        return emb

    def embed_ragged_resident(self, buf, offsets, lengths, max_batch_samples=64 * 1024 * 1024, first_utt=0, spans=None,
                              crop_idx=None):
        """`embed_ragged` for audio that is ALREADY in one buffer: `buf` is one 1-D int16 array holding every clip, clip k at
        samples [offsets[k], offsets[k] + lengths[k]) (offsets multiples of 8: 16-byte aligned; host arrays; clips may
        overlap, e.g. windows over one recording).
          * a DEVICE tensor: batches are lists of clip indices into that one buffer -- nothing is copied or packed, not even
            the voiced frames (the VAD hands the front end an index of them);
          * a HOST NumPy array (a loader that decodes into one arena): uploaded as it is, no per-clip packing on the host
            (the list form, `embed_ragged`, is bound by that packing: ~20 GB/s of host copy against 54 GB/s of pageable
            upload on the GPU box).  Arenas larger than two batches go up in pieces of ~`max_batch_samples` on the upload
            stream from a helper thread, and the clips of piece p run (length-sorted among themselves) while piece p + 1
            travels."""
        if self.crop_rng != "device":
            raise ValueError("embed_ragged_resident needs crop_rng='device'")
        offsets = np.asarray(offsets, dtype=np.int64)
        lengths = np.asarray(lengths, dtype=np.int32)
        if offsets.shape != lengths.shape or (offsets % 8).any():
            raise ValueError("offsets / lengths must have one entry per clip, offsets multiples of 8 samples")
        host = isinstance(buf, np.ndarray)
        if host:
            if buf.ndim != 1 or buf.dtype != np.int16:
                raise ValueError("buf must be a 1-D int16 array")
            buf = np.ascontiguousarray(buf)
            n_samples = buf.size
        else:
            buf = self.eng.to_device(buf)
            if buf.dim() != 1 or buf.dtype != torch.int16:
                raise ValueError("buf must be a 1-D int16 tensor")
            n_samples = buf.numel()
        if len(lengths) and int((offsets + lengths).max()) > n_samples:
            raise ValueError("a clip reaches past the end of buf")
        dev = self.eng.device
        emb = torch.empty((len(lengths), 128), dtype=torch.float32, device=dev)
        if not len(lengths):
            return emb
        # upload groups: clips by arena position, cut where a piece passes max_batch_samples (one group = everything when
        # the buffer is on the device already or small)
        groups, pieces = [np.arange(len(lengths))], [(0, n_samples)]
        if host and n_samples > 2 * max_batch_samples:
            groups, pieces = self._upload_groups(offsets, lengths, n_samples, max_batch_samples)
        plan, group_of = [], []                               # every group's batches, in group order
        for g, idx in enumerate(groups):
            for batch, _ in self._ragged_batches(lengths[idx], max_batch_samples):
                plan.append(idx[np.asarray(batch, dtype=np.int64)])
                group_of.append(g)
        # with pieces still travelling the network runs per micro-batch of gathered cubes (it covers the next piece's upload);
        # otherwise over micro-batches as large as the main path's
        step = self.micro_batch if len(groups) > 1 else max(self.micro_batch, 4096)
        if not host:
            self._ragged_loop(emb, plan, offsets, lengths, step, first_utt, spans, lambda k: buf, crop_idx=crop_idx)
            return emb
        src = torch.from_numpy(buf)
        buf = torch.empty((n_samples,), dtype=torch.int16, device=dev)
        with _Upload(self._streams()[0], [(buf[a:b], src[a:b]) for a, b in pieces]) as up:
            def fetch(k):                                     # the first batch of a piece waits for that piece
                if k == 0 or group_of[k] != group_of[k - 1]:
                    up.wait(group_of[k])
                return buf
            self._ragged_loop(emb, plan, offsets, lengths, step, first_utt, spans, fetch, crop_idx=crop_idx)
        return emb

    def embed_host(self, pcm_host, first_utt=0):
        """Host-fed variant of `embed`: `pcm_host` is a [n, L] int16 NumPy array (e.g. decoded WAVs) or a CPU torch
        tensor, pinned or not.  Micro-batches go through the upload stream and two device buffers, so the H2D copy of batch
        k + 1 overlaps the kernels of batch k (96 kB per 3 s clip over PCIe).  A HELPER THREAD issues the
        copies: a pageable upload holds its calling thread (the runtime stages it through its own pinned chunks, 54 GB/s on
        the GPU box -- faster than the 20 GB/s at which this process could copy into a pinned buffer of its own, the
        round-2 form), and the main thread keeps launching kernels."""
        if self.crop_rng != "device":
            raise ValueError("embed_host overlaps copies with compute and needs crop_rng='device'")
        src = pcm_host if isinstance(pcm_host, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pcm_host))
        if src.dtype != torch.int16 or src.dim() != 2 or src.is_cuda:
            raise ValueError("pcm_host must be a [n, L] int16 array in host memory")
        n, L = src.shape
        spans = self.chunks(n)
        emb = torch.empty((n, 128), dtype=torch.float32, device=self.eng.device)
        if not spans:
            return emb
        staged = self._staging(max(hi - lo for lo, hi in spans) * L)
        copies = [(staged[k & 1][:(hi - lo) * L].view(hi - lo, L), src[lo:hi]) for k, (lo, hi) in enumerate(spans)]
        with _Upload(self._streams()[0], copies, slots=2) as up:
            for k, (lo, hi) in enumerate(spans):
                up.wait(k)
                feat, _, idx = self._front(copies[k][0], first_utt + lo)
                emb[lo:hi] = self.embed_features(feat, idx)
                up.release(k)
        return emb

    def project(self, emb):
        """The rows as the scorers see them: through the back end and the PLDA projection, or unchanged without either."""
        return project_rows(self.eng, emb, self.backend, self.plda)

    def score(self, test_emb, enroll_emb, counts=None):
        """Every test row against every enrolled row: cosines, or with `plda` log-likelihood ratios.  counts (PLDA only): the
        utterances behind each enrolled row when those are mean models (`enroll_mean(..., l2=False)` with a model fitted
        with l2_in=False, whose projection is the mean of the projections; otherwise build the models with `Plda.enroll` and
        score them with `Plda.score`)."""
        if self.plda is None and counts is not None:
            raise ValueError("counts belong to PLDA scoring: the cosine does not use them")
        test_emb, enroll_emb = self.project(test_emb), self.project(enroll_emb)
        scores = self.eng.cosine_scores(test_emb, enroll_emb) if self.plda is None else \
            self.plda.score(test_emb, enroll_emb, counts=counts, engine=self.eng)
        if self.score_norm is not None:       # between the raw score and the calibration, in place
            self.score_norm.normalize(scores, *self.score_norm.side_moments(test_emb, enroll_emb, counts), out=scores)
        if self.calibration is not None:      # in place on the fresh scores
            self.calibration.apply(scores.reshape(-1), engine=self.eng, out=scores.reshape(-1))
        return scores

    def decide(self, llr, p_target, c_miss=1, c_fa=1):
        """Accept / reject calibrated LLRs at the Bayes threshold of an operating point -> a bool tensor, llr >=
        log(c_fa (1 - p_target) / (c_miss p_target)) (the threshold as float32, the precision of the scores)."""
        from .calibration import bayes_threshold
        return self.eng.to_device(llr, torch.float32) >= float(np.float32(bayes_threshold(p_target, c_miss, c_fa)))

    SEARCH_UPLOAD_BYTES = 1 << 30       # a host gallery above this is uploaded and searched in chunks of about this size

    def search(self, test_emb, enroll_emb, k=1, exclude_self=False, chunk_rows=None):
        """The k best enrolled rows of every test row by cosine score (`svk_cosine_topk`: the score matrix of `score` is
        never written) -> (scores float32 [n, k], indices int64 [n, k]) on the device, best first, -1 / -inf past the
        enrolled rows.  enroll_emb: a device tensor or a host array.  With chunk_rows, or for a host array above
        SEARCH_UPLOAD_BYTES, the gallery is uploaded and searched chunk by chunk into one set of lists (the accumulate flag):
        the same bits as one call.  exclude_self: the two sides are the same rows and row q is no candidate for query q.  With a
        back end both sides are projected first, a chunked gallery chunk by chunk (a row's projection depends on that row alone)."""
        if self.plda is not None:
            raise ValueError("search ranks by cosine score: top-k by PLDA log-likelihood ratio is not built (use score)")
        if self.calibration is not None:
            raise ValueError("search ranks by raw cosine score: calibrated top-k is `identify` (or use score)")
        if self.score_norm is not None:
            raise ValueError("search ranks by raw cosine score: top-k on normalised scores is `identify` (or use score)")
        return self._search(test_emb, enroll_emb, k, exclude_self, chunk_rows, None)

    def _search(self, test_emb, enroll_emb, k, exclude_self, chunk_rows, score_norm):
        """`search` (score_norm None: svk_cosine_topk) and `identify` (a ScoreNorm: svk_cosine_topk_norm, the test side's
        moments taken once, the enrolled side's per gallery chunk) over one chunking rule."""
        eng = self.eng
        n_gallery, dim = int(enroll_emb.shape[0]), int(enroll_emb.shape[1])
        query = self.project(eng.to_device(test_emb, torch.float32))
        exclude = None
        if exclude_self:
            if int(query.shape[0]) != n_gallery:
                raise ValueError("exclude_self wants the same rows on both sides (%d against %d)" % (query.shape[0], n_gallery))
            exclude = torch.arange(n_gallery, dtype=torch.int64, device=eng.device)
        if score_norm is None:
            def topk(rows, **kw):
                return eng.cosine_topk(query, rows, k, exclude=exclude, **kw)
        else:
            sides = score_norm.mode        # a side the mode does not use is not computed; _tables drops it
            test_moments = score_norm.moments(query, "test") if sides in ("t", "s") else None

            def topk(rows, **kw):
                row, col = score_norm._tables(test_moments, score_norm.moments(rows, "enroll") if sides in ("z", "s") else None)
                return eng.cosine_topk_norm(query, rows, k, query_moments=row, gallery_moments=col, exclude=exclude, **kw)
        on_host = not (isinstance(enroll_emb, torch.Tensor) and enroll_emb.is_cuda)
        if chunk_rows is None and on_host and 4 * n_gallery * dim > self.SEARCH_UPLOAD_BYTES:
            chunk_rows = max(1, self.SEARCH_UPLOAD_BYTES // (4 * dim))
        if chunk_rows is None or n_gallery == 0:
            return topk(self.project(enroll_emb))
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows must be at least 1")
        into = None
        for lo in range(0, n_gallery, chunk_rows):
            into = topk(self.project(enroll_emb[lo:lo + chunk_rows]), index_base=lo, into=into)
        return into

    def identify(self, test_emb, enroll_emb, k=1, exclude_self=False, chunk_rows=None):
        """The k best enrolled rows of every test row under the scores `score` gives -- the cosine through the back end, the
        score normalisation and the calibration -- without the test x enrolled matrix -> (scores float32 [n, k], indices int64
        [n, k]) on the device, best first, -1 / -inf past the enrolled rows.  Open-set identification: reject the returned
        scores at `calibration.bayes_threshold` (`decide`), a threshold that transfers between speakers and conditions where
        a raw cosine's does not.
        With `score_norm` the normalisation sits inside the selection (`svk_cosine_topk_norm`: for one test row the normalised
        score is no monotone function of the cosine across enrolled rows, so `search`'s lists cannot be re-ranked into
        these); the test side's cohort moments are taken once, the enrolled side's per gallery chunk (a row's moments depend
        on that row alone).  The scores are `svk_score_norm`'s bits on `svk_cosine_topk`'s raw bits.
        With `calibration` (one system, weight > 0) `calibration.apply` then runs on the returned [n, k] scores in place.  The
        map is increasing, so the ranking is the normalised score's: calibrated values are NON-INCREASING along a list, not
        strictly decreasing, and entries that the final rounding to float32 makes equal keep the order of their
        uncalibrated scores (which need not be index order).  A weight <= 0 (a decreasing map) or anything but an affine
        one-system calibration raises ValueError; so does a PLDA: top-k by log-likelihood ratio is not built.
        With neither normalisation nor calibration the result is `search`'s, byte for byte.  Chunking (chunk_rows, host
        galleries above SEARCH_UPLOAD_BYTES) and exclude_self behave as in `search`: the same bytes as one call."""
        if self.plda is not None:
            raise ValueError("identify ranks by cosine-based scores: top-k by PLDA log-likelihood ratio is not built (use score)")
        cal = self.calibration
        if cal is not None:
            weights = getattr(cal, "weights_", None)
            if weights is None or np.size(weights) != 2:
                raise ValueError("identify wants a fitted affine calibration of ONE system (weight, offset): a fusion of several "
                                 "systems or a step map does not rank by this pipeline's score")
            if not float(np.asarray(weights).reshape(-1)[0]) > 0.0:
                raise ValueError("identify wants a calibration weight > 0 (an increasing map keeps the ranking), got %r"
                                 % (float(np.asarray(weights).reshape(-1)[0]),))
        if self.score_norm is not None:
            self.score_norm.check_scorer(self.backend, self.plda)
        scores, indices = self._search(test_emb, enroll_emb, k, exclude_self, chunk_rows, self.score_norm)
        if cal is not None:
            cal.apply(scores.reshape(-1), engine=self.eng, out=scores.reshape(-1))
        return scores, indices

    def cluster(self, emb, *, k, threshold, min_shared=0, mutual=True, min_size=1, chunk_rows=None):
        """Pseudo-speaker labels for unlabelled rows: the self-search of `search` (exclude_self; with a back end the rows
        are projected first; chunk_rows as there) and `svk_knn_cluster` on its lists -> `clustering.Clustering(labels, roots,
        sizes, counts)` on the device.  Rows i and j are joined when each is among the other's k nearest with a cosine >=
        threshold (mutual=False: one direction is enough) and they share at least min_shared of their k neighbours; a cluster
        is a connected component of at least min_size rows, numbered by its smallest row, and the other rows are labelled -1.
        k (1 .. 32) and threshold have no default: nothing tuned is built in.  `clustering.segments` turns the labels into
        what `backend.solve` and `enroll_mean`'s pool take.  The lists are raw cosines: with a PLDA, a score normalisation or
        a calibration this raises, as `search` does."""
        from .clustering import Clustering
        if self.plda is not None:
            raise ValueError("cluster ranks by cosine score: top-k by PLDA log-likelihood ratio is not built (use score)")
        if self.calibration is not None:
            raise ValueError("cluster ranks by raw cosine score: calibrated top-k is `identify` (or use score)")
        if self.score_norm is not None:
            raise ValueError("cluster ranks by raw cosine score: top-k on normalised scores is `identify` (or use score)")
        scores, indices = self._search(emb, emb, k, True, chunk_rows, None)
        return Clustering(*self.eng.knn_cluster(scores, indices, threshold=threshold, min_shared=min_shared, mutual=mutual,
                                                min_size=min_size))

    def _raw_cosine_rows(self, what, emb):
        """The rows as `cluster` searched them (through the back end), for the calls that go on from its labels; they raise
        where `cluster` does, in its words."""
        if self.plda is not None:
            raise ValueError("%s ranks by cosine score: top-k by PLDA log-likelihood ratio is not built (use score)" % what)
        if self.calibration is not None:
            raise ValueError("%s ranks by raw cosine score: calibrated top-k is `identify` (or use score)" % what)
        if self.score_norm is not None:
            raise ValueError("%s ranks by raw cosine score: top-k on normalised scores is `identify` (or use score)" % what)
        return self.project(self.eng.to_device(emb, torch.float32))

    def merge_clusters(self, emb, labels, **kw):
        """The second stage after `cluster` when k fragments a speaker: `clustering.merge_clusters` (which lists the
        keywords; `threshold` and `k` have no default) on the rows as `cluster` saw them -- projected through the back end
        first -> `clustering.Merged`.  Raises with a PLDA, a score normalisation or a calibration, as `cluster` does."""
        from .clustering import merge_clusters
        return merge_clusters(self.eng, self._raw_cosine_rows("merge_clusters", emb), labels, **kw)

    def adopt_rows(self, emb, labels, **kw):
        """The rows `cluster`'s min_size left at -1 join the nearest cluster centroid at `threshold` or above:
        `clustering.adopt_rows` on the rows as `cluster` saw them (projected first) -> `clustering.Adopted`.  Raises with a
        PLDA, a score normalisation or a calibration, as `cluster` does."""
        from .clustering import adopt_rows
        return adopt_rows(self.eng, self._raw_cosine_rows("adopt_rows", emb), labels, **kw)

    def diarize(self, pcm, **kw):
        """"Who spoke when": int16 PCM [n_rec, samples] of recordings with several speakers -> one list of
        `diarization.Turn(start_s, end_s, speaker)` per recording (`diarization.Diarizer.diarize`, which lists the keywords:
        `threshold` or `num_speakers` must be given under the default method="ahc"; method="spectral" counts the speakers from
        the eigengap and needs neither).  The Diarizer (1.5 s windows every 0.75 s) is made on first use."""
        if getattr(self, "_diarizer", None) is None:
            from .diarization import Diarizer
            self._diarizer = Diarizer(self)
        return self._diarizer.diarize(pcm, **kw)

    def score_trials(self, emb_a, idx_a, idx_b, emb_b=None, metric="cosine"):
        """One score per trial (emb_a[idx_a[p]] against emb_b[idx_b[p]], emb_b = emb_a when not given) through
        `svk_pair_scores` -> float32 [n_trials] on the device: a VoxCeleb-style trial list instead of the whole matrix of
        `score`.  On several GPUs call it on the all-gathered embeddings (`distributed.all_gather_embeddings`); every rank
        then holds the whole list's scores (the trial list itself is not sharded).  With `plda`: log-likelihood ratios through
        `svk_plda_pair_scores`, emb_a the test side and emb_b the enrolled side (one utterance each); `metric` must be left alone.
        With `score_norm`: emb_a's rows take the test side's cohort moments, emb_b's the enrolled side's."""
        return trial_scores(self.eng, emb_a, idx_a, idx_b, emb_b, metric, self.backend, self.plda, self.calibration,
                            score_norm=self.score_norm)


def project_rows(eng, emb, backend, plda):
    """emb through the back end and the PLDA projection, or unchanged without either."""
    if backend is not None:
        emb = backend.transform(emb, engine=eng)
    return emb if plda is None else plda.project(emb, engine=eng)


def trial_scores(eng, emb_a, idx_a, idx_b, emb_b=None, metric="cosine", backend=None, plda=None, calibration=None, bad_count=None,
                 score_norm=None):
    """The scoring chain of a trial list (`VerificationPipeline.score_trials`, `evaluation.evaluate_trials`): both sides through
    `project_rows`, PLDA log-likelihood ratios or `svk_pair_scores`, the score normalisation and the calibration in place ->
    float32 [n_trials] on the device.  emb_b None: both indices address emb_a.  bad_count: an int32 device counter of the
    indices outside their matrix.  score_norm: a fitted `score_norm.ScoreNorm` (for the same back end and PLDA; cosine metric):
    the cohort moments of every row of the a side as test rows and of the b side as enrolled rows, then svk_score_norm_pairs
    (every row of both sides, referenced by a trial or not; with emb_b None and the cosine, one table serves both sides)."""
    if plda is not None and metric != "cosine":
        raise ValueError("PLDA scores are log-likelihood ratios: metric does not apply")
    if score_norm is not None:
        score_norm.check_scorer(backend, plda)
        if metric != "cosine":
            raise ValueError("the cohort is scored by cosine or PLDA: metric %r cannot be normalised on it" % (metric,))
    u_a = project_rows(eng, emb_a, backend, plda)
    u_b = u_a if emb_b is None else project_rows(eng, emb_b, backend, plda)
    if plda is not None:
        scores = plda.score_trials(u_a, idx_a, idx_b, u_b=u_b, bad_count=bad_count, engine=eng)
    else:
        scores = eng.pair_scores(u_a, u_b, idx_a, idx_b, metric=metric, bad_count=bad_count)
    if score_norm is not None:
        test_moments, enroll_moments = score_norm.side_moments(u_a, u_b)
        score_norm.normalize_trials(scores, test_moments, idx_a, enroll_moments, idx_b, out=scores)
    if calibration is not None:
        calibration.apply(scores, engine=eng, out=scores)
    return scores


def enroll_last_utterance(embeddings, speaker_ids):
    """Speaker model = embedding of that speaker's LAST listed utterance: the reference
    overwrites `{id}.pt` on every utterance, no averaging (Q17, model.py:374-388).
    Returns (sorted unique ids, row index of each speaker's model)."""
    speaker_ids = np.asarray(speaker_ids)
    uniq = np.unique(speaker_ids)
    last = np.array([np.nonzero(speaker_ids == s)[0][-1] for s in uniq], dtype=np.int64)
    return uniq, last


def enroll_mean(embeddings, speaker_ids, l2=True):
    """Speaker model = the mean of the speaker's utterance embeddings (each L2-normalised first with `l2`), what the d-vector
    method describes; `enroll_last_utterance` is the reference's own behaviour.  One `svk_embedding_pool` launch over CSR
    segments (`speaker_segments`).  Returns (sorted unique ids, models [S, 128] float32 on the device)."""
    uniq, seg_start, row_index = speaker_segments(speaker_ids)
    eng = get_engine()
    emb = eng.to_device(embeddings, torch.float32)
    if emb.dim() != 2 or emb.shape[0] != row_index.size:
        raise ValueError("enroll_mean wants one embedding row per speaker id")
    return uniq, eng.embedding_pool(emb, seg_start=seg_start, row_index=row_index, l2_rows=l2)
