"""evaluation.py drop-in (`/root/reference/evaluation.py`): `get_eer_auc`,
`get_and_plot_k_eer_auc`, `Evaluation(...).compute_Similarity(...)`,
`evaluate()`.

The reference scores one (utterance, speaker) pair per sklearn call inside a
Python double loop (evaluation.py:67-84, 112-134); here the whole score matrix
is one MFMA kernel launch (`svk_cosine_scores`), and the embeddings behind it
come from the libsvk network kernels (`model.C3D2.forward` in eval mode on the
device; `dataset_embeddings` for the file-driven entry points).  By default
ROC / EER / AUC and the top-1 count stay on the host exactly as the reference
computes them (sklearn + scipy, evaluation.py:47-52, 112-134).  `device=True`
(`get_and_plot_k_eer_auc`, `evaluate`) keeps the score matrix on the GPU:
`svk_top1` for the argmax, hits and one-hot labels, ONE `svk_roc_k` call for the
k splits and their ROC curves; `get_eer_auc_device` is the single-split form.

Trial lists (the `label utterance_a utterance_b` protocols of VoxCeleb1, which the reference does not read): `read_trials` /
`make_trials` build the index pairs, `evaluate_trials` scores them with `svk_pair_scores` and reports EER, AUC, minDCF and the
thresholds (`svk_roc_dcf`; `get_min_dcf` is the host form of the same definition).
"""
import os

import numpy as np
import torch

from .engine import get_engine


def get_eer_auc(label, distance):
    """(eer, auc, fpr, tpr) from flat labels and scores (evaluation.py:47-52)."""
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq
    from sklearn.metrics import roc_auc_score, roc_curve
    fpr, tpr, thresholds = roc_curve(label, distance, pos_label=1)
    auc = roc_auc_score(label, distance)
    eer = brentq(lambda x: 1. - x - interp1d(fpr, tpr)(x), 0., 1.)
    return eer, auc, fpr, tpr


def get_eer_auc_device(label, distance, curve=False):
    """(eer, auc) like `get_eer_auc`, computed on the GPU (radix sort + scans + one pass over the ROC
    points): for score sets that should not travel to the host (dev-set scale, 1.8e8 pairs).
    Accepts NumPy arrays or CUDA tensors of any shape.  curve=True: (eer, auc, fpr, tpr), the shape
    `get_eer_auc` returns -- fpr / tpr bit-identical to sklearn's roc_curve (svk_roc_k, k = 1), which
    also raises, as sklearn does, for NaN or infinite scores."""
    if curve:
        return get_engine().roc_k(distance, label, k=1, curve=True)[0]
    return get_engine().roc_eer(distance, label)


DEFAULT_OPERATING_POINTS = ((0.01, 1, 1), (0.05, 1, 1))      # (p_target, c_miss, c_fa): the two VoxCeleb results quote


def get_min_dcf(label, distance, p_target, c_miss=1, c_fa=1):
    """(min_dcf, threshold, p_miss, p_fa) on the host, float64 NumPy over sklearn's roc_curve(drop_intermediate=False): the
    candidates are the curve's origin (reject everything, threshold +inf) and one point per distinct score in descending
    order; cost = c_miss p_target (1 - tpr) + c_fa (1 - p_target) fpr; min_dcf = the smallest cost / min(c_miss p_target,
    c_fa (1 - p_target)); among equal costs the first point (the highest threshold) wins.  Accept when score >= threshold."""
    from sklearn.metrics import roc_curve
    if not (0.0 < p_target < 1.0 and c_miss > 0 and c_fa > 0):
        raise ValueError("need 0 < p_target < 1 and c_miss, c_fa > 0")
    fpr, tpr, thresholds = roc_curve(np.asarray(label).reshape(-1), np.asarray(distance).reshape(-1), pos_label=1,
                                     drop_intermediate=False)
    a, b = float(c_miss) * float(p_target), float(c_fa) * (1.0 - float(p_target))
    cost = a * (1.0 - tpr) + b * fpr
    j = int(np.argmin(cost))                         # the first of equal minima
    threshold = float("inf") if j == 0 else float(thresholds[j])
    return float(cost[j] / min(a, b)), threshold, float(1.0 - tpr[j]), float(fpr[j])


def read_trials(path_or_lines):
    """A trial list -- lines of `label name_a name_b`, label 1 = same speaker, 0 = different; blank lines and lines starting
    with `#` are skipped -- from a path or an iterable of lines.  Returns (labels uint8 [n], idx_a int64 [n], idx_b int64 [n],
    names): the indices point into `names`, every distinct name once, in order of first appearance (the row order the
    embeddings are wanted in).  ValueError names the line for a malformed line or a label other than 0 or 1."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines) as fh:
            return read_trials(fh.readlines())
    index, names, labels, ia, ib = {}, [], [], [], []
    for number, line in enumerate(path_or_lines, 1):
        text = line.strip()
        if not text or text.startswith("#"):
            continue
        parts = text.split()
        if len(parts) != 3:
            raise ValueError("trial list line %d: want `label name_a name_b`, got %r" % (number, text))
        if parts[0] not in ("0", "1"):
            raise ValueError("trial list line %d: label must be 0 or 1, got %r" % (number, parts[0]))
        labels.append(int(parts[0]))
        for name, dst in ((parts[1], ia), (parts[2], ib)):
            if name not in index:
                index[name] = len(names)
                names.append(name)
            dst.append(index[name])
    return np.array(labels, dtype=np.uint8), np.array(ia, dtype=np.int64), np.array(ib, dtype=np.int64), names


def make_trials(speaker_ids, n_target, n_nontarget, seed):
    """A seeded trial list for a corpus without an official one: n_target pairs (i, j) of the same speaker and n_nontarget
    of different speakers, i != j, no unordered pair twice.  Returns (labels uint8, idx_a int64, idx_b int64), targets
    first.  ValueError when the corpus holds fewer such pairs than asked for."""
    ids = np.asarray(speaker_ids)
    n = int(ids.size)
    _, inv = np.unique(ids, return_inverse=True)
    sizes = np.bincount(inv) if n else np.zeros(0, dtype=np.int64)
    have_t = int(np.sum(sizes * (sizes - 1) // 2))
    have_n = n * (n - 1) // 2 - have_t
    if n_target < 0 or n_nontarget < 0 or n_target > have_t or n_nontarget > have_n:
        raise ValueError("make_trials: %d target / %d non-target pairs asked for, the %d utterances hold %d / %d"
                         % (n_target, n_nontarget, n, have_t, have_n))
    rng = np.random.default_rng(seed)
    members = [np.nonzero(inv == s)[0] for s in range(sizes.size) if sizes[s] >= 2]
    small = 1 << 22                                   # up to here every candidate pair is listed and the draw is a choice

    def sample(pairs, count):
        return pairs[rng.choice(pairs.shape[0], size=count, replace=False)]

    def reject(count, propose):
        seen, out = set(), []
        while len(out) < count:
            i, j = propose()
            key = (min(i, j), max(i, j))
            if key not in seen:
                seen.add(key)
                out.append((i, j))
        return np.array(out, dtype=np.int64).reshape(-1, 2)

    def same():
        m = members[int(rng.choice(len(members), p=weights))]
        i, j = rng.choice(m.size, size=2, replace=False)
        return int(m[i]), int(m[j])

    def differ():
        while True:
            i, j = (int(v) for v in rng.integers(0, n, size=2))
            if inv[i] != inv[j]:
                return i, j

    if n_target == 0:
        tgt = np.zeros((0, 2), dtype=np.int64)
    elif have_t <= small:
        tgt = sample(np.concatenate([np.stack([m[a] for a in np.triu_indices(m.size, 1)], axis=1) for m in members]), int(n_target))
    else:
        weights = np.array([m.size * (m.size - 1) / 2.0 for m in members])
        weights /= weights.sum()
        tgt = reject(int(n_target), same)
    if n_nontarget == 0:
        non = np.zeros((0, 2), dtype=np.int64)
    elif n * (n - 1) // 2 <= small:
        i, j = np.triu_indices(n, 1)
        keep = inv[i] != inv[j]
        non = sample(np.stack([i[keep], j[keep]], axis=1), int(n_nontarget))
    else:
        non = reject(int(n_nontarget), differ)
    idx = np.concatenate([tgt, non]).astype(np.int64)
    labels = np.r_[np.ones(int(n_target), dtype=np.uint8), np.zeros(int(n_nontarget), dtype=np.uint8)]
    return labels, np.ascontiguousarray(idx[:, 0]), np.ascontiguousarray(idx[:, 1])


def evaluate_trials(embeddings, labels, idx_a, idx_b, metric="cosine", operating_points=DEFAULT_OPERATING_POINTS, device=True,
                    backend=None, plda=None, calibration=None, score_norm=None, rocch=False):
    """Verification over a trial list: trial p compares embeddings[idx_a[p]] with embeddings[idx_b[p]] (`svk_pair_scores`,
    metric "cosine" or "l2"), labels[p] = 1 for the same speaker.  Returns a dict: eer, auc, eer_threshold, and per operating
    point (p_target, c_miss, c_fa) the lists min_dcf, threshold, p_miss, p_fa; scores = the float32 trial scores on the device.
    device=True: one `svk_roc_dcf` call; device=False: the same device scores, metrics on the host (`get_eer_auc`,
    `get_min_dcf`; eer_threshold by the same rule, the first point of the curve where 1 - fpr - tpr <= 0).  An index outside
    the embeddings raises ValueError.  backend: a fitted `backend.EmbeddingBackend`; the embeddings go through it first.
    plda: a fitted `plda.Plda` (fitted behind the back end, if any): the rows are projected and the scores are PLDA
    log-likelihood ratios (`svk_plda_pair_scores`, idx_a the test side); metric must then be left at its default.
    calibration: a fitted one-system `calibration.Calibration`: the trial scores go through it before the metrics (scores = the
    calibrated LLRs) and the dict gains cllr and the list act_dcf, the cost of deciding at each operating point's Bayes
    threshold (`svk_decision_counts`; min_dcf <= act_dcf, the gap is the calibration loss).  None (the default) changes nothing.
    score_norm: a `score_norm.ScoreNorm` fitted on a cohort for the same back end and PLDA: the trial scores are normalised
    (between the raw score and the calibration) before the metrics, and scores = the normalised scores.  None (the default)
    changes nothing.
    rocch=True (with device=True): the metrics come from ONE `svk_rocch` call instead of `svk_roc_dcf` -- the same values, bit
    for bit -- and the dict gains min_cllr and rocch_eer (the ROC convex hull, `calibration.min_cllr_of`); with a calibration
    also calibration_loss = cllr - min_cllr.  False (the default) changes nothing."""
    from .pipeline import trial_scores
    if rocch and not device:
        raise ValueError("evaluate_trials: rocch=True takes the hull from the device ROC (device=True)")
    eng = get_engine()
    if calibration is not None and calibration.n_sys != 1:
        raise ValueError("evaluate_trials scores one system: the calibration must be fitted on one, not %r" % (calibration.n_sys,))
    bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    emb = eng.to_device(embeddings, torch.float32)
    scores = trial_scores(eng, emb, idx_a, idx_b, None, metric, backend, plda, calibration, bad, score_norm=score_norm)
    if int(bad.item()):
        raise ValueError("evaluate_trials: %d trials index outside the %d embeddings" % (int(bad.item()), emb.shape[0]))
    labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
    if labels.size != scores.numel():
        raise ValueError("one label per trial")
    ops = [tuple(float(v) for v in op) for op in operating_points]
    if device:
        res = eng.rocch(scores, labels, ops) if rocch else eng.roc_dcf(scores, labels, ops)
        out = {k: res[k] for k in ("eer", "auc", "eer_threshold", "min_dcf", "threshold", "p_miss", "p_fa")}
        if rocch:
            out["min_cllr"], out["rocch_eer"] = res["min_cllr"], res["rocch_eer"]
    else:
        from sklearn.metrics import roc_curve
        sc = scores.cpu().numpy()
        eer, auc, _, _ = get_eer_auc(labels, sc)
        fpr, tpr, thr = roc_curve(labels, sc, pos_label=1, drop_intermediate=False)
        at = int(np.nonzero(1.0 - fpr - tpr <= 0)[0][0])
        rows = [get_min_dcf(labels, sc, *op) for op in ops]
        out = {"eer": float(eer), "auc": float(auc), "eer_threshold": float(thr[at]),
               "min_dcf": [r[0] for r in rows], "threshold": [r[1] for r in rows], "p_miss": [r[2] for r in rows],
               "p_fa": [r[3] for r in rows]}
    if calibration is not None:
        from . import calibration as cal
        out["cllr"] = cal.cllr(scores, labels, engine=eng)
        out["act_dcf"] = cal.act_dcf(scores, labels, ops, engine=eng)[0]
        if rocch:
            out["calibration_loss"] = out["cllr"] - out["min_cllr"]
    out["scores"] = scores
    return out


def get_and_plot_k_eer_auc(label, scores, k=1, plot_path='eer_auc.png', device=False):
    """Mean EER / AUC over k consecutive equal slices, printed in percent, ROC
    curves saved to `plot_path` when matplotlib is importable (evaluation.py:11-44).
    Returns (mean_eer, mean_auc) in addition to the reference's prints.
    device=True: one `svk_roc_k` call on the GPU for all k splits (labels / scores may be CUDA
    tensors; the curves of the plot come from the device too)."""
    eers, aucs, curves = np.zeros((k, 1)), np.zeros((k, 1)), []
    if device:
        for split_num, res in enumerate(get_engine().roc_k(scores, label, k=k, curve=bool(plot_path))):
            eers[split_num], aucs[split_num] = res[0], res[1]
            curves.append(res[2:])
    else:
        step = int(label.shape[0] / float(k))
        for split_num in range(k):
            lo, hi = split_num * step, (split_num + 1) * step
            eers[split_num], aucs[split_num], fpr, tpr = get_eer_auc(label[lo:hi], scores[lo:hi])
            curves.append((fpr, tpr))
    print("EER=", np.mean(eers) * 100)
    print("AUC=", np.mean(aucs) * 100)
    if plot_path:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            fig = plt.figure()
            ax = fig.gca()
            for split_num, (fpr, tpr) in enumerate(curves):
                plt.setp(plt.plot(fpr, tpr, label='{} split'.format(split_num)), linewidth=2)
            ax.set_xticks(np.arange(0, 1.1, 0.1))
            ax.set_yticks(np.arange(0, 1.1, 0.1))
            plt.title('ROC with {}-fold cross validation'.format(k))
            plt.xlabel('False Positive Rate')
            plt.ylabel('True Positive Rate')
            plt.grid()
            plt.savefig(plot_path)
            plt.close(fig)
        except ImportError:
            pass
    return float(np.mean(eers)), float(np.mean(aucs))


def score_matrix(test_embeddings, enroll_embeddings):
    """[Nt, D] x [Ns, D] -> [Nt, Ns] float32 cosine scores on the device."""
    return get_engine().cosine_scores(test_embeddings, enroll_embeddings)


class Evaluation:
    """Same constructor and `compute_Similarity` as evaluation.py:55-84.
    `speaker_models_path` may be a directory of `{speaker_id}.pt` tensors (the
    reference's format, Q17) or a dict {speaker_id: (1, D) tensor}."""

    def __init__(self, background_model, speaker_models_path):
        self.model = background_model
        self.speaker_models = {}
        if isinstance(speaker_models_path, dict):
            for key, value in speaker_models_path.items():
                self.speaker_models[key] = torch.as_tensor(value)
        else:
            for file in sorted(os.listdir(speaker_models_path)):          # explicit order
                if file.endswith('.pt'):
                    self.speaker_models[file.replace('.pt', '')] = torch.load(
                        os.path.join(speaker_models_path, file), map_location="cpu", weights_only=True)
        self._enroll = None

    def _enroll_matrix(self):
        if self._enroll is None:
            eng = get_engine()
            rows = [m.detach().reshape(1, -1).to(torch.float32) for m in self.speaker_models.values()]
            self._enroll = eng.to_device(torch.cat(rows, dim=0))
        return self._enroll

    def embed(self, utterance):
        """`self.model(utterance, development=False)` in eval mode on the device (evaluation.py:68-69): for a `model.C3D2`
        that is the seven libsvk network kernels (the cube read as feature rows, model.C3D2.forward)."""
        eng = get_engine()
        self.model.eval()
        self.model.to(eng.device)
        with torch.no_grad():
            return self.model(eng.to_device(utterance, torch.float32), development=False)

    def compute_Similarity(self, utterance, type='cosine_similarity'):
        """(similarity_vec, assigned_speaker_vec), both float64 of length n_speakers."""
        speaker_features = self.embed(utterance)
        if type == 'cosine_similarity':
            scores = get_engine().cosine_scores(speaker_features[:1], self._enroll_matrix())
            similarity_vec = scores[0].to("cpu").numpy().astype(np.float64)
            assigned_speaker_vec = np.zeros(len(self.speaker_models))
            assigned_speaker_vec[np.argmax(similarity_vec)] = 1
            return similarity_vec, assigned_speaker_vec

    def score_all(self, cubes, batch=256):
        """[N, 1, 20, 80, 40] cubes -> [N, n_speakers] float32 scores (device), batched."""
        outs = []
        for lo in range(0, len(cubes), batch):
            outs.append(get_engine().cosine_scores(self.embed(cubes[lo:lo + batch]), self._enroll_matrix()))
        return torch.cat(outs, dim=0)


def labels_from_ids(test_ids, speaker_ids):
    """One-hot truth rows like evaluation.py:130-132."""
    speaker_ids = list(speaker_ids)
    labels = np.zeros((len(test_ids), len(speaker_ids)))
    for i, sid in enumerate(test_ids):
        labels[i, speaker_ids.index(sid)] = 1
    return labels


def _read_batch(dataset, lo, hi):
    """Files [lo, hi) of an `AudioDataset` as ONE arena + 16-byte-aligned clip offsets + lengths.  16 kHz mono 16-bit files
    (what the reference's tree holds, vad.py:10-22) are read straight into an int16 arena -- no float copy on the host, the
    `/ 32768` of `librosa.load` (utils.py:170-173) is folded into the front end's filterbank weights; a batch with any other
    rate / channel count falls back to `load_signal`'s float32 (resampled on the device)."""
    import wave
    from . import constants as c
    paths = [os.path.join(dataset.audio_dir, dataset.sound_files[i]) for i in range(lo, hi)]
    heads = []
    for path in paths:
        with wave.open(path, "rb") as wf:
            heads.append((wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()))
    plain = all(h[:3] == (1, 2, c.SAMPLE_RATE) for h in heads)
    if plain:
        lens = np.array([h[3] for h in heads], dtype=np.int32)
        align = 8
    else:
        sigs = [np.asarray(dataset.load_signal(i), dtype=np.float32) for i in range(lo, hi)]
        lens = np.array([x.size for x in sigs], dtype=np.int32)
        align = 4
    slots = (lens.astype(np.int64) + align - 1) // align * align
    offs = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64)
    buf = np.zeros(int(slots.sum()), dtype=np.int16 if plain else np.float32)
    for k, path in enumerate(paths):
        if plain:
            with wave.open(path, "rb") as wf:
                buf[offs[k]:offs[k] + lens[k]] = np.frombuffer(wf.readframes(int(lens[k])), dtype=np.int16)
        else:
            buf[offs[k]:offs[k] + lens[k]] = sigs[k]
    return buf, offs, lens, plain


def dataset_embeddings(dataset, model, batch=256):
    """Embeddings [len(dataset), 128] (device) of every file of a `load_data.AudioDataset`, in order:
    the per-item chain of the reference (load_data.py:50-87 `load_wav` -> `lmfe`; utils.py:382-397 CMVN;
    utils.py:351-379 FeatureCube with crop starts from the GLOBAL NumPy RNG, drawn in file order;
    `model(cube, development=False)`) run `batch` files at a time: one ragged front-end launch, one CMVN and the seven
    libsvk network kernels per batch -- the cube is never built (`svk_c3d2_stage1` reads feature rows + crop starts).
    With `constants.DERIVATIVE` (a `C3D2(n, 3)` model, utils.py:325-348 FeatureCube3C): one statistics pass over the static
    features (`svk_delta_cmvn_stats`) and one pass that writes the three normalised channel planes (`svk_delta_planes`),
    then `svk_c3d2_stage1_c3` on those planes."""
    from . import _lib
    from . import constants as c
    from .engine import spec_from_seconds
    eng = get_engine()
    model = model.to(eng.device).eval()
    n = len(dataset)
    out = torch.empty((n, 128), dtype=torch.float32, device=eng.device)
    specs = {plain: spec_from_seconds(c.SAMPLE_RATE, c.FRAME_LEN, c.FRAME_STEP, c.NUM_FFT, c.NUM_COEF, c.NUM_COEF, _lib.OUT_LMFE,
                                      input_scale=1.0 / 32768.0 if plain else 1.0) for plain in (True, False)}
    embed = model.fused_inference()
    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        buf, offs, lens, plain = _read_batch(dataset, lo, hi)
        spec = specs[plain]
        frames = [spec.num_frames(int(v)) for v in lens]
        feat, n_frames, _ = eng.features(buf, spec, lengths=lens, offsets=offs, max_frames=max(frames))
        if c.DERIVATIVE:
            # utils.py:385-391: static, delta and the delta of delta (extract_derivative_feature, Q11 included), then CMVN per
            # channel; [n, 3, T, 40] is the layout svk_c3d2_stage1_c3 reads (FeatureCube3C's crops of it)
            stats = eng.delta_cmvn_stats(feat, n_frames, delta=2, variance=True) if c.NORMALIZE else None
            feat = eng.delta_planes(feat, n_frames, delta=2, stats=stats)
        elif c.NORMALIZE:
            eng.cmvn_(feat, n_frames, variance=True)
        # utils.py:372, one draw per file in file order (numpy raises for clips of <= 80 frames, as there)
        idx = np.stack([np.random.randint(T - c.CUBE_FRAMES, size=c.CUBE_CROPS) for T in frames]).astype(np.int32)
        out[lo:hi] = embed.embed_features(feat, idx)
    return out


def load_indexed_labels(path):
    """{speaker id: class index} for `create_dataset`.  The reference keeps it as a PICKLED dict inside
    `50_first_ids.npy` (`np.load(..., allow_pickle=True).item()`, evaluation.py:100, model.py:360); unpickling runs
    whatever the file says, so this build never does it.  Sources, in order: a `.json` file of the same stem; else the
    id list of the same stem (`50_first_ids.txt`, which carries the same information): speaker id = the first 7
    characters of each path (load_data.py:73), class index = rank among the sorted ids.  The labels only ride along
    in the dataset items; enrolment and evaluation key on the ids themselves."""
    import json
    stem = os.path.splitext(path)[0]
    if os.path.exists(stem + '.json'):
        with open(stem + '.json') as fh:
            return json.load(fh)
    if os.path.exists(stem + '.txt'):
        ids = sorted({str(line)[0:7] for line in np.atleast_1d(np.genfromtxt(stem + '.txt', dtype='str'))})
        return {sid: k for k, sid in enumerate(ids)}
    raise FileNotFoundError(f"{stem}.json / {stem}.txt not found ({path} is a pickle: not loaded)")


def _true_columns(test_ids, speaker_ids):
    """Column of each test id among the enrolled speaker ids (labels_from_ids' one-hot as an index), -1 for an id that
    was never enrolled."""
    col = {}
    for j, sid in enumerate(speaker_ids):
        col.setdefault(sid, j)
    return np.array([col.get(t, -1) for t in test_ids], dtype=np.int32)


def _device_top1_roc(scores, test_ids, speaker_ids, k, plot_path, print_lines):
    """The device half of `evaluate(device=True)`: argmax / hits / one-hot labels (svk_top1), the reference's per-utterance
    line from the argmax indices (print_lines: the file-driven form prints them, as the host path does), EER / AUC
    (svk_roc_k).  scores: the device score matrix."""
    amax, correct, labels = get_engine().top1(scores, _true_columns(test_ids, speaker_ids), want_labels=True)
    amax = amax.cpu().numpy() if print_lines else ()
    for i in range(len(amax)):
        current_id = test_ids[i]
        print('correct speaker {} , the speaker was closer to {}'.format(current_id, speaker_ids[int(amax[i])]))
    eer, auc = get_and_plot_k_eer_auc(labels.reshape(-1), scores.reshape(-1), k=k, plot_path=plot_path, device=True)
    return eer, auc, correct, labels


def _evaluate_files(k, plot_path, device=False):
    """evaluation.py:90-146 as written: checkpoint, id list, id table, WAV tree and enrolled models
    under `constants.ROOT` / `constants.DATA_ORIGIN`."""
    from . import constants as c
    from .model import C3D2
    from .utils import create_dataset
    model_path = os.path.join(c.ROOT, 'Models/model_14_percent_best_so_far.pt')
    checkpoint = torch.load(model_path, map_location="cpu", weights_only=True)
    model = C3D2(100, 1).load_checkpoint(checkpoint)
    dir_path = os.path.join(c.ROOT, 'speaker_models')
    test_set = os.path.join(c.ROOT, '50_first_ids.txt')
    indexed_labels = load_indexed_labels(c.ROOT + '/50_first_ids.npy')
    dataset = create_dataset(indexed_labels=indexed_labels, origin_file_path=test_set)
    ev = Evaluation(model, dir_path)
    speaker_model_ids = list(ev.speaker_models.keys())
    emb = dataset_embeddings(dataset, model)
    if device:
        test_ids = [f[0:7] for f in dataset.sound_files]
        scores = get_engine().cosine_scores(emb, ev._enroll_matrix())
        eer, auc, correct, labels = _device_top1_roc(scores, test_ids, speaker_model_ids, k, plot_path, True)
        accuracy = correct * 100 / len(dataset)
        print(f'Accuracy: {accuracy}%')
        return {"eer": eer, "auc": auc, "accuracy": accuracy, "scores": scores, "labels": labels,
                "speaker_ids": speaker_model_ids, "test_ids": test_ids}
    scores = get_engine().cosine_scores(emb, ev._enroll_matrix()).to("cpu").numpy().astype(np.float64)
    labels = np.zeros_like(scores)
    correct = 0
    ids = np.array(speaker_model_ids)
    for i in range(len(dataset)):
        current_id = dataset.sound_files[i][0:7]
        closest = speaker_model_ids[int(np.argmax(scores[i]))]
        print('correct speaker {} , the speaker was closer to {}'.format(current_id, closest))
        correct += int(current_id == closest)
        labels[i][np.where(current_id == ids)] = 1                   # an id that was never enrolled: all zeros
    eer, auc = get_and_plot_k_eer_auc(labels.flatten(), scores.flatten(), k=k, plot_path=plot_path)
    accuracy = correct * 100 / len(dataset)
    print(f'Accuracy: {accuracy}%')
    return {"eer": eer, "auc": auc, "accuracy": accuracy, "scores": scores, "labels": labels,
            "speaker_ids": speaker_model_ids, "test_ids": [f[0:7] for f in dataset.sound_files]}


def create_speaker_models(model=None, cubes=None, speaker_ids=None, save_dir=None, batch=256, enroll="last"):
    """`model.create_speaker_models` (model.py:351-388) under this module's name: enroll="last" keeps each speaker's last
    listed utterance, as the reference does (Q17); enroll="mean" takes the mean of the speaker's L2-normalised utterance
    embeddings (`pipeline.enroll_mean`).  `evaluate(..., enroll_cubes=, enroll_ids=, enroll=)` enrols through it."""
    from .model import create_speaker_models as _create
    return _create(model, cubes, speaker_ids, save_dir, batch, enroll=enroll)


def evaluate(model=None, cubes=None, test_ids=None, speaker_models=None, k=1, plot_path='eer_auc.png', device=False,
             enroll="last", enroll_cubes=None, enroll_ids=None):
    """`evaluate()` -- no arguments, like evaluation.py:90-146: read the checkpoint, the id list, the WAVs and
    the enrolled `{id}.pt` models from the paths in `constants`, score every utterance against every
    enrolled speaker (one batched front end + network + ONE cosine launch instead of the reference's
    per-utterance, per-speaker loop), print the reference's lines, save the ROC plot.
    `evaluate(model, cubes, test_ids, speaker_models)` is the same loop on in-memory data.
    Returns a dict (the reference returns None): eer, auc, accuracy, scores, labels -- float64 NumPy arrays.
    device=True: the score matrix never leaves the GPU.  Accuracy comes from `svk_top1`, EER / AUC from ONE `svk_roc_k`
    call, the labels from the enrolled column of each test id (-1, an all-zero row, for an id never enrolled); the
    per-utterance lines are printed from the argmax indices.  `scores` and `labels` are then the DEVICE tensors
    (float32 [n_test, n_speakers], uint8 one-hot).
    Without `speaker_models`, the in-memory form enrols `enroll_cubes` / `enroll_ids` itself through
    `create_speaker_models(..., enroll=enroll)`: "last" (the reference, the default) or "mean"."""
    if enroll not in ("last", "mean"):
        raise ValueError("enroll must be 'last' or 'mean', got %r" % (enroll,))
    if model is None and cubes is None:
        return _evaluate_files(k, plot_path, device)
    if speaker_models is None:
        if enroll_cubes is None or enroll_ids is None:
            raise ValueError("evaluate needs speaker_models, or enroll_cubes and enroll_ids to enrol from")
        speaker_models = create_speaker_models(model, enroll_cubes, enroll_ids, enroll=enroll)
    ev = Evaluation(model, speaker_models)
    speaker_ids = list(ev.speaker_models.keys())
    if device:
        scores = ev.score_all(cubes)
        eer, auc, correct, labels = _device_top1_roc(scores, list(test_ids), speaker_ids, k, plot_path, False)
        accuracy = correct * 100 / max(1, len(test_ids))
        print(f'Accuracy: {accuracy}%')
        return {"eer": eer, "auc": auc, "accuracy": accuracy, "scores": scores, "labels": labels}
    scores = ev.score_all(cubes).to("cpu").numpy().astype(np.float64)
    labels = labels_from_ids(test_ids, speaker_ids)
    correct = int(sum(speaker_ids[int(np.argmax(scores[i]))] == test_ids[i] for i in range(len(test_ids))))
    eer, auc = get_and_plot_k_eer_auc(labels.flatten(), scores.flatten(), k=k, plot_path=plot_path)
    accuracy = correct * 100 / max(1, len(test_ids))
    print(f'Accuracy: {accuracy}%')
    return {"eer": eer, "auc": auc, "accuracy": accuracy, "scores": scores, "labels": labels}


def identification_accuracy(model, data, labels=None, topk=(1, 5), batch=4096):
    """train.py:104-119's accuracy pass as a function: which of the model's n_labels training speakers each input is.
    `data`: cubes [n, C, 20, 80, 40] (tensor or array) with `labels` [n] (class indices), or a `load_data.AudioDataset`, whose
    labels are `indexed[sound_files[i][0:7]]` (load_data.py:73) and whose embeddings come from `dataset_embeddings` (the same
    crop draws from NumPy's global RNG).  The head runs through `C3D2.identify` (svk_c3d2_head on the device, no probability
    matrix).  Returns {"top1": %, "top5": % (one key per entry of `topk`), "predicted": int32 [n] top-1 labels, "n": n}."""
    k = max(topk)
    device = next(model.parameters()).device
    model.eval()
    if hasattr(data, "sound_files"):
        true = np.array([data.indexed[f[0:7]] for f in data.sound_files], dtype=np.int32)
        emb = dataset_embeddings(data, model)
        chunks = [(emb[lo:lo + batch], true[lo:lo + batch]) for lo in range(0, len(true), batch)]
    else:
        if labels is None:
            raise ValueError("identification_accuracy on cubes needs their labels")
        true = np.asarray(labels, dtype=np.int32).reshape(-1)
        if len(true) != len(data):
            raise ValueError("one label per cube")
        chunks = ((torch.as_tensor(data[lo:lo + batch], dtype=torch.float32).to(device), true[lo:lo + batch])
                  for lo in range(0, len(true), batch))
    n = len(true)
    hits = np.zeros(k, dtype=np.int64)
    predicted = []
    for x, t in chunks:
        top, h = model.identify(x, k=k, true_idx=t)
        hits += np.asarray(h, dtype=np.int64)
        predicted.append(top[:, 0].cpu().numpy().astype(np.int32))
    out = {"top%d" % r: (100.0 * float(hits[r - 1]) / n if n else 0.0) for r in topk}
    out["predicted"] = np.concatenate(predicted) if predicted else np.zeros(0, dtype=np.int32)
    out["n"] = n
    return out


def rank_speakers(test_embeddings, enroll_embeddings, speaker_ids, k=5, threshold=None, pipeline=None):
    """The k nearest enrolled speakers of every test utterance (`svk_cosine_topk`: no score matrix) -> {"ids": [n][k] lists of
    speaker ids, best first, "scores": float32 [n, k], "indices": int64 [n, k]} (NumPy).  speaker_ids[j] names row j of
    enroll_embeddings.  threshold: open-set rejection -- an entry whose score is below it (or a slot past the enrolled rows,
    index -1) is reported as None; a NaN score is never below a threshold.
    pipeline: a `VerificationPipeline`; ranks, scores and the rejection are then `pipeline.identify`'s -- the scores of its
    back end, score normalisation and calibration.  On calibrated scores the threshold of an operating point is
    `calibration.bayes_threshold(p_target, c_miss, c_fa)`, which, unlike a raw cosine threshold, transfers between speakers."""
    speaker_ids = list(speaker_ids)
    if len(speaker_ids) != int(enroll_embeddings.shape[0]):
        raise ValueError("one speaker id per enrolled row")
    if pipeline is None:
        scores, indices = get_engine().cosine_topk(test_embeddings, enroll_embeddings, k)
    else:
        scores, indices = pipeline.identify(test_embeddings, enroll_embeddings, k=k)
    scores, indices = scores.cpu().numpy(), indices.cpu().numpy()
    keep = indices >= 0
    if threshold is not None:
        keep &= ~(scores < np.float32(threshold))
    ids = [[speaker_ids[j] if ok else None for j, ok in zip(row, row_ok)] for row, row_ok in zip(indices, keep)]
    return {"ids": ids, "scores": scores, "indices": indices}


def topk_hits(indices, true_columns):
    """hits int64 [k] from top-k lists indices [n, k] (best first, -1 = empty slot) and the true column of every row [n]
    (-1 = not enrolled): hits[r] = the rows whose true column is among their first r + 1 entries -- the meaning of
    svk_c3d2_head's h_hits; -1 never counts.  Pure NumPy; 100 hits[r] / n is the rank-(r + 1) accuracy."""
    indices = np.asarray(indices)
    true_columns = np.asarray(true_columns).reshape(-1)
    if indices.ndim != 2 or indices.shape[0] != true_columns.size:
        raise ValueError("topk_hits wants indices (n, k) and one true column per row")
    match = (indices == true_columns[:, None]) & (indices >= 0)
    return np.cumsum(match, axis=1).astype(bool).sum(axis=0).astype(np.int64)
