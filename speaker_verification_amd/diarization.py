"""Speaker diarization: "who spoke when" in recordings with several speakers.

The device path is the pipeline's own front (VAD in index form, log-mel features), then three libsvk entries of csrc/cluster.hip
around the multi-cube embedding call:

    pipeline.vad -> pipeline.features -> svk_window_crops -> embedder.embed_features(feat, crops[n, K, 20], pool=None)
    [-> pipeline.project with a back end] -> svk_segment_affinity -> svk_ahc
    or, with method="spectral" (INTEGRATION 11), which counts the speakers itself:
    ... -> svk_segment_affinity [-> svk_ahc down to 128 nodes] -> svk_spectral_embed -> svk_segment_affinity -> svk_ahc

One D2H then fetches labels, window spans and the VAD frame map, and the timeline -- a few hundred integers per recording -- is
built on the host.  The host helpers (window rule, timeline, RTTM, DER) need no GPU."""
from collections import namedtuple

import numpy as np

from . import constants as c

Turn = namedtuple("Turn", ["start_s", "end_s", "speaker"])


# ---- the window rule on the host (svk_window_crops states the same in a kernel) -------------------------------------
def num_windows(n_frames, win_frames, hop_frames, crop_frames):
    """Windows the rule asks for in a recording of n_frames feature frames."""
    T = max(int(n_frames), 0)
    if T < crop_frames:
        return 0
    if T < win_frames:
        return 1
    return (T - win_frames) // hop_frames + 1 + int((T - win_frames) % hop_frames != 0)


def window_table(n_frames, max_windows, win_frames=150, hop_frames=75, crop_frames=c.CUBE_FRAMES, n_crops=c.CUBE_CROPS):
    """-> (crop_idx int32 [max_windows, n_crops] with -1 in unused windows, n_windows, spans int32 [max_windows, 2] = (first
    frame, length) with (-1, 0) in unused ones, overflow: whether the recording needs more than max_windows)."""
    T = max(int(n_frames), 0)
    need = num_windows(T, win_frames, hop_frames, crop_frames)
    crops = np.full((max_windows, n_crops), -1, np.int32)
    spans = np.tile(np.array([-1, 0], np.int32), (max_windows, 1))
    for w in range(min(need, max_windows)):
        if T < win_frames:
            w0, length = 0, T
        elif w <= (T - win_frames) // hop_frames:
            w0, length = w * hop_frames, win_frames
        else:
            w0, length = T - win_frames, win_frames
        spans[w] = (w0, length)
        for k in range(n_crops):
            crops[w, k] = w0 + (k * (length - crop_frames)) // max(n_crops - 1, 1)
    return crops, min(need, max_windows), spans, need > max_windows


# ---- the timeline ---------------------------------------------------------------------------------------------------
def frame_labels(spans, labels, n_frames):
    """The label of every feature frame: that of the window whose centre is nearest, the earlier window on a tie.  spans
    [n_windows, 2] (first frame, length), labels [n_windows] -> int32 [n_frames]; -1 everywhere without a window.  In
    integers: frame f has its centre at f + 1/2, window (w0, len) at w0 + len / 2, both doubled."""
    spans = np.asarray(spans, np.int64).reshape(-1, 2)
    labels = np.asarray(labels, np.int32).reshape(-1)
    n_frames = max(int(n_frames), 0)
    if spans.shape[0] == 0:
        return np.full(n_frames, -1, np.int32)
    centre2 = 2 * spans[:, 0] + spans[:, 1]
    frame2 = 2 * np.arange(n_frames, dtype=np.int64) + 1
    nearest = np.argmin(np.abs(frame2[:, None] - centre2[None, :]), axis=1)      # argmin: the first among equals
    return labels[nearest].astype(np.int32)


def timeline(flabels, frame_stride, n_packed, src_frame=None, frame_samples=1, fs=c.SAMPLE_RATE):
    """Frame labels -> turns in ORIGINAL time.  Feature frame f stands for the packed samples [f stride, (f + 1) stride), the
    last frame for everything up to n_packed (the voiced samples of the recording).  Packed sample p lies in kept VAD frame
    q = p // frame_samples, whose place in the recording is src_frame[q] * frame_samples + p % frame_samples (src_frame None:
    nothing was dropped).  Runs of equal labels become turns; a turn never spans a VAD gap: it ends where the kept frames
    stop being consecutive.  Frames labelled -1 give no turn."""
    flabels = np.asarray(flabels).reshape(-1)
    n_packed = int(n_packed)
    turns = []
    if flabels.size == 0 or n_packed <= 0:
        return turns
    S = int(frame_samples)
    cuts = np.flatnonzero(np.diff(flabels)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [flabels.size]])
    for f0, f1 in zip(starts, ends):
        label = int(flabels[f0])
        p0 = int(f0) * frame_stride
        p1 = n_packed if f1 == flabels.size else int(f1) * frame_stride
        p0, p1 = min(p0, n_packed), min(p1, n_packed)
        if label < 0 or p1 <= p0:
            continue
        if src_frame is None:
            pieces = [(p0, p1)]
        else:
            pieces = []
            for q in range(p0 // S, (p1 - 1) // S + 1):
                a, b = max(p0, q * S), min(p1, (q + 1) * S)
                o = int(src_frame[q]) * S + (a - q * S)
                if pieces and pieces[-1][1] == o:
                    pieces[-1] = (pieces[-1][0], o + (b - a))
                else:
                    pieces.append((o, o + (b - a)))
        for a, b in pieces:
            if turns and turns[-1].speaker == label and turns[-1].end_s == a / fs:
                turns[-1] = Turn(turns[-1].start_s, b / fs, label)
            else:
                turns.append(Turn(a / fs, b / fs, label))
    return turns


# ---- RTTM -----------------------------------------------------------------------------------------------------------
def write_rttm(path, turns_by_file):
    """{file id: [Turn]} -> `SPEAKER file 1 start dur <NA> <NA> name <NA> <NA>` lines, one per turn."""
    with open(path, "w") as fh:
        for name, turns in turns_by_file.items():
            for t in turns:
                fh.write("SPEAKER %s 1 %.6f %.6f <NA> <NA> %s <NA> <NA>\n" % (name, t.start_s, t.end_s - t.start_s, t.speaker))


def read_rttm(path):
    """-> {file id: [Turn]} in file order.  A speaker name that reads as an integer comes back as one."""
    out = {}
    with open(path) as fh:
        for line in fh:
            parts = line.split()
            if not parts or parts[0] != "SPEAKER":
                continue
            if len(parts) < 8:
                raise ValueError("short RTTM line: %r" % (line,))
            start, dur, name = float(parts[3]), float(parts[4]), parts[7]
            try:
                name = int(name)
            except ValueError:
                pass
            out.setdefault(parts[1], []).append(Turn(start, round(start + dur, 6), name))
    return out


# ---- diarization error rate -----------------------------------------------------------------------------------------
DER_STEP_S = 0.01


def _grid(turns, names, n_cells):
    active = np.zeros((len(names), n_cells), bool)
    for t in turns:
        active[names.index(t.speaker), int(round(t.start_s / DER_STEP_S)):int(round(t.end_s / DER_STEP_S))] = True
    return active


def der(reference, hypothesis, collar=0.0):
    """Diarization error rate of one recording: (missed speech + false alarm + speaker confusion) / reference speech, on a
    10 ms grid, under the speaker map that maximises the matched time (scipy.optimize.linear_sum_assignment).  Cells within
    `collar` seconds of a reference turn boundary are not scored.  Overlapped reference speech counts once per speaker."""
    from scipy.optimize import linear_sum_assignment
    ref_names = sorted({t.speaker for t in reference}, key=str)
    hyp_names = sorted({t.speaker for t in hypothesis}, key=str)
    end = max([t.end_s for t in reference] + [t.end_s for t in hypothesis] + [0.0])
    n_cells = int(round(end / DER_STEP_S))
    ref, hyp = _grid(reference, ref_names, n_cells), _grid(hypothesis, hyp_names, n_cells)
    scored = np.ones(n_cells, bool)
    if collar > 0:
        half = int(round(collar / DER_STEP_S))
        for t in reference:
            for edge in (t.start_s, t.end_s):
                k = int(round(edge / DER_STEP_S))
                scored[max(0, k - half):k + half] = False
    ref, hyp = ref[:, scored], hyp[:, scored]
    n_ref, n_hyp = ref.sum(0), hyp.sum(0)
    total = int(n_ref.sum())
    if total == 0:
        raise ValueError("the reference holds no scored speech")
    matched = 0
    if ref_names and hyp_names:
        overlap = ref.astype(np.int64) @ hyp.astype(np.int64).T
        rows, cols = linear_sum_assignment(-overlap)
        matched = int(overlap[rows, cols].sum())
    miss = int(np.maximum(n_ref - n_hyp, 0).sum())
    false_alarm = int(np.maximum(n_hyp - n_ref, 0).sum())
    confusion = int(np.minimum(n_ref, n_hyp).sum()) - matched
    return (miss + false_alarm + confusion) / total


# ---- the device path ------------------------------------------------------------------------------------------------
class Diarizer:
    def __init__(self, pipeline, window_s=1.5, hop_s=0.75):
        """pipeline: a `VerificationPipeline`; its VAD, front end, embedder and back end are used as they are.  Windows of
        window_s seconds every hop_s seconds of VOICED signal, one embedding each (20 crops of 80 frames spread over the
        window).  PLDA, calibration and score normalisation are not built into the affinity: ValueError."""
        self.pipeline = pipeline
        self._check_scorer()
        self.win_frames = int(round(window_s / c.FRAME_STEP))
        self.hop_frames = int(round(hop_s / c.FRAME_STEP))
        if self.win_frames < c.CUBE_FRAMES or self.hop_frames < 1:
            raise ValueError("a window holds at least %d frames (%.2f s) and the hop at least one"
                             % (c.CUBE_FRAMES, c.CUBE_FRAMES * c.FRAME_STEP))

    def _check_scorer(self):
        for what in ("plda", "calibration", "score_norm"):
            if getattr(self.pipeline, what, None) is not None:
                raise ValueError("diarization clusters cosine affinities: `%s` inside diarize is not built (a `backend` is "
                                 "supported)" % what)

    def _windows(self, pcm, lengths):
        """PCM -> per-window embeddings of every recording (projected when the pipeline has a back end) and what the
        timeline needs, all on the device."""
        import torch
        self._check_scorer()
        from .pipeline import clips_per_chunk
        pipe = self.pipeline
        eng = pipe.eng
        pcm = eng.to_device(pcm)
        if pcm.dim() != 2:
            raise ValueError("diarize wants PCM [n_rec, samples] (pad to the longest; `lengths` holds the samples of each)")
        n_rec, longest = int(pcm.shape[0]), int(pcm.shape[1])
        if lengths is not None and not isinstance(lengths, torch.Tensor):
            lengths = np.asarray(lengths, np.int32)
        lens = None if lengths is None else eng.to_device(lengths, torch.int32)
        vlen, gather = pipe.vad(pcm, lengths=lens)
        feat, n_frames = pipe.features(pcm, vlen, gather)
        # the window count of the longest recording bounds every recording's (the VAD only shortens): no host round trip
        K = max(1, num_windows(pipe.spec.num_frames(longest), self.win_frames, self.hop_frames, c.CUBE_FRAMES))
        bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
        crops, n_win, spans = eng.window_crops(n_frames, K, self.win_frames, self.hop_frames, c.CUBE_FRAMES, c.CUBE_CROPS, bad)
        step = clips_per_chunk(pipe.micro_batch, K)
        parts = [pipe.embedder.embed_features(feat[lo:lo + step], crops[lo:lo + step], pool=None) for lo in range(0, n_rec, step)]
        emb = torch.cat(parts) if len(parts) != 1 else parts[0]
        if pipe.backend is not None:
            emb = pipe.project(emb.reshape(n_rec * K, -1)).view(n_rec, K, -1)
        packed = vlen if vlen is not None else torch.full((n_rec,), longest, dtype=torch.int32, device=eng.device)
        return {"emb": emb, "n_windows": n_win, "spans": spans, "n_frames": n_frames, "packed": packed,
                "src_frame": None if gather is None else gather[0], "frame_samples": 1 if gather is None else int(gather[1])}

    def affinity(self, pcm, lengths=None):
        """-> (affinity float32 [n_rec, K, K], n_windows int32 [n_rec]) on the device: the cosines `diarize` clusters, for tuning
        a threshold on a development set.  Entries of unused windows are zero."""
        win = self._windows(pcm, lengths)
        return self.pipeline.eng.segment_affinity(win["emb"], win["n_windows"]), win["n_windows"]

    METHODS = ("ahc", "spectral")
    NEIGHBOURS = (2, 32, 2)      # a SEARCH RANGE (lo, hi, step) for the neighbour count, not a tuned value
    MAX_SPEAKERS = 8             # how far the eigengap is looked for under `spectral` when the caller sets no bound

    @staticmethod
    def _arguments(method, threshold, num_speakers):
        """The argument rules of `diarize` that need no engine."""
        if method not in Diarizer.METHODS:
            raise ValueError("unknown method %r: diarize clusters with %s" % (method, " or ".join(map(repr, Diarizer.METHODS))))
        if method == "spectral":
            if threshold is not None:
                raise ValueError("`threshold` stops agglomerative merging: method='spectral' counts the speakers from the "
                                 "eigengap and takes none")
        elif threshold is None and num_speakers is None:
            raise ValueError("diarize needs `threshold` or `num_speakers`: no affinity threshold has been measured for any "
                             "checkpoint, and none is assumed (method='spectral' needs neither)")

    def _spectral(self, eng, aff, n_win, target, min_speakers, max_speakers, neighbours):
        """affinities -> (window labels, speaker counts, the tensors behind them): svk_ahc down to the node limit where the
        window stride exceeds it, svk_spectral_embed, the cosines of the embedding rows, svk_ahc to the counted speakers, and
        the node labels gathered through the groups."""
        limit = eng.spectral_limits()[0]
        group = None
        if int(aff.shape[1]) > limit:
            group, _ = eng.ahc(aff, n_win, threshold=None, max_clusters=limit)
        embed, n_nodes, n_spk, chosen = eng.spectral_embed(aff, n_win, group=group, neighbours=neighbours, min_speakers=min_speakers,
                                                           max_speakers=max_speakers, target=target)
        node_labels, count = eng.ahc(eng.segment_affinity(embed, n_nodes), n_nodes, target=n_spk)
        labels = node_labels
        if group is not None:
            # rows move, nothing is computed: window -> its node's label (dead windows, group -1, stay -1)
            import torch
            labels = torch.gather(node_labels, 1, group.clamp(min=0).long()).masked_fill(group < 0, -1)
        return labels, count, {"group": group, "embedding": embed, "n_nodes": n_nodes, "neighbours": chosen, "node_labels": node_labels}

    def diarize(self, pcm, lengths=None, threshold=None, num_speakers=None, min_speakers=1, max_speakers=None,
                return_device=False, method="ahc", neighbours=None):
        """pcm int16 [n_rec, samples] -> one list of Turn(start_s, end_s, speaker) per recording, in original time.
        method="ahc" (the default): either `threshold` (merging stops when no pair of clusters reaches this cosine; it has NO
        default: tune it on a development set with `affinity`) or `num_speakers` (an int, or one per recording) must be given;
        min_speakers / max_speakers bound the cluster count under a threshold.
        method="spectral": neither is needed.  The speakers are counted from the largest eigengap of a nearest-neighbour
        graph of the windows, between min_speakers and max_speakers (default 8); `neighbours` is the graph's neighbour count,
        an int or a (lo, hi, step) range searched by the normalised maximum eigengap -- the default (2, 32, 2) is a search
        range, not a tuned value.  num_speakers, where given, replaces the count; `threshold` is refused.  Recordings with more
        windows than svk_spectral_limits()[0] are first merged down to that many nodes by svk_ahc.
        return_device: also the dict of device tensors behind the result."""
        self._arguments(method, threshold, num_speakers)
        import torch
        eng = self.pipeline.eng
        win = self._windows(pcm, lengths)
        n_rec, K = int(win["emb"].shape[0]), int(win["emb"].shape[1])
        target = None
        if num_speakers is not None:
            target = np.broadcast_to(np.asarray(num_speakers, np.int32), (n_rec,)).copy()
            if (target < 1).any():
                raise ValueError("num_speakers must be at least 1")
        aff = eng.segment_affinity(win["emb"], win["n_windows"])
        extra = {}
        if method == "spectral":
            labels, count, extra = self._spectral(eng, aff, win["n_windows"], target, min_speakers,
                                                  self.MAX_SPEAKERS if max_speakers is None else max_speakers,
                                                  self.NEIGHBOURS if neighbours is None else neighbours)
        else:
            labels, count = eng.ahc(aff, win["n_windows"], threshold=threshold, min_clusters=min_speakers, max_clusters=max_speakers,
                                    target=target)
        # ONE D2H: labels, spans, counts and the VAD frame map as one int32 row per recording
        cols = [labels, win["spans"].reshape(n_rec, 2 * K), win["n_windows"][:, None], win["n_frames"][:, None],
                win["packed"][:, None], count[:, None]]
        if win["src_frame"] is not None:
            cols.append(win["src_frame"])
        host = torch.cat(cols, dim=1).cpu().numpy()
        out = []
        stride = self.pipeline.spec.frame_stride
        for r in range(n_rec):
            row = host[r]
            n_win, n_frames, packed = int(row[3 * K]), int(row[3 * K + 1]), int(row[3 * K + 2])
            fl = frame_labels(row[K:3 * K].reshape(K, 2)[:n_win], row[:n_win], n_frames)
            src = row[3 * K + 4:] if win["src_frame"] is not None else None
            out.append(timeline(fl, stride, packed, src, win["frame_samples"]))
        if return_device:
            win.update(affinity=aff, labels=labels, n_clusters=count, **extra)
            return out, win
        return out
