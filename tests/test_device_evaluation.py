"""Device-side evaluation: the native radix-sort ROC of csrc/roc.hip (svk_roc_eer, svk_roc_k), k-fold splits, roc_curve on
the device, svk_top1, and `evaluate(device=True)` against the host path, sklearn and the reference's goldens."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "speaker_verification_amd", "libsvk.so")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    if not os.path.exists(LIB):
        entry.build()
    from speaker_verification_amd import _lib
    return _lib.load()


# ---- CPU ------------------------------------------------------------------------------------------------------
def test_no_library_sort_in_libsvk(lib):
    """The ROC's sort, scan and select are the library's own kernels: no rocPRIM / hipCUB code in libsvk.so."""
    src = open(os.path.join(REPO, "speaker_verification_amd", "csrc", "roc.hip")).read()
    assert not re.search(r"#\s*include\s*[<\"](hipcub|rocprim|thrust)", src)
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm is needed to list libsvk.so's symbols"
    syms = subprocess.run([nm, "-C", LIB], check=True, capture_output=True, text=True).stdout
    assert syms.count("svk_roc_k") >= 1
    hits = [line for line in syms.splitlines() if re.search(r"rocprim|hipcub", line, re.I)]
    assert not hits, hits[:5]


def test_new_entry_points_reject_a_null_context(lib):
    from speaker_verification_amd import _lib
    out = (C.c_double * 4)()
    assert lib.svk_roc_k(None, None, None, 100, 1, None, 0, None, out) == _lib.SVK_ERR_BAD_ARG
    assert lib.svk_roc_k(None, None, None, 100, 1, None, 0, None, None) == _lib.SVK_ERR_BAD_ARG
    corr = C.c_int64(-7)
    assert lib.svk_top1(None, None, 4, 4, None, None, None, C.byref(corr)) == _lib.SVK_ERR_BAD_ARG
    assert corr.value == -7
    for n, k in ((2, 1), (100, 3), (148642 * 1211, 10), ((1 << 32) - 1, 7)):
        assert lib.svk_roc_k_workspace_bytes(n, k) > 0
        assert lib.svk_roc_k_workspace_bytes(n, k) <= lib.svk_roc_workspace_bytes(n)
    assert lib.svk_roc_k_workspace_bytes(3, 2) == 0 and lib.svk_roc_k_workspace_bytes(10, 0) == 0


def test_split_step_is_the_references_slicing():
    """evaluation.py:13 slices with int(n / float(k)); split_step (and svk_roc_k's n / k) must give the same splits."""
    from speaker_verification_amd.engine import split_step
    rng = np.random.default_rng(3)
    ns = [2, 3, 10, 11, 99, 1000, 148642 * 1211, (1 << 31) + 12345, (1 << 32) - 1] + list(rng.integers(2, 1 << 32, 200))
    for n in ns:
        for k in (1, 2, 3, 5, 7, 10, 13, 64, 1000):
            step = int(n / float(k))
            assert split_step(n, k) == step
            x = np.arange(min(int(n), 50))
            assert [list(x[s * step:(s + 1) * step]) for s in range(k)] == \
                   [list(x[s * split_step(n, k):(s + 1) * split_step(n, k)]) for s in range(k)]


# ---- GPU ------------------------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return get_engine(0)


def sk_roc(labels, scores):
    from sklearn.metrics import roc_curve
    fpr, tpr, _ = roc_curve(np.asarray(labels), np.asarray(scores), pos_label=1)
    return fpr, tpr


def curve_of_counts(f, t):
    """roc_curve's drop_intermediate + origin on the distinct-score counts (int64 NumPy), as sklearn 1.7 writes it."""
    if f.size > 2:
        keep = np.r_[True, np.logical_or(np.diff(f, 2), np.diff(t, 2)), True]
        f, t = f[keep], t[keep]
    return np.r_[0, f], np.r_[0, t]


def torch_counts(sc, lb):
    """The distinct-score (fps, tps) counts by torch on the GPU: sort + cumsum + tie-group ends (the oracle)."""
    s = torch.where(sc == 0, torch.zeros_like(sc), sc)
    s, order = torch.sort(s, descending=True, stable=True)
    tps = torch.cumsum(lb[order].to(torch.int64), 0)
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[:-1] != s[1:]
    idx = torch.nonzero(last).squeeze(1)
    t = tps[idx]
    return (idx + 1 - t).cpu().numpy(), t.cpu().numpy()


def eer_auc_of_points(f, t):
    """EER (linear root of 1 - fpr - tpr) and trapezoid AUC of a curve in counts, float64 NumPy."""
    f, t = np.r_[0, f].astype(np.float64), np.r_[0, t].astype(np.float64)
    x, y = f / f[-1], t / t[-1]
    auc = float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5))
    g = 1.0 - x - y
    j = np.nonzero((g[:-1] > 0) & (g[1:] <= 0))[0]
    eer = float(x[j[0]] + (x[j[0] + 1] - x[j[0]]) * g[j[0]] / (g[j[0]] - g[j[0] + 1])) if j.size else 0.0
    return eer, auc


def assert_curve_is_sklearns(eng, lab, sc, k=1):
    """svk_roc_k per split: fpr / tpr bit-identical to sklearn's roc_curve, eer / auc within 1e-9 of sklearn + brentq."""
    from oracle import scoring_ref
    got = eng.roc_k(sc, lab, k=k, curve=True)
    step = lab.size // k
    for s, (eer, auc, fpr, tpr) in enumerate(got):
        ls, ss = lab[s * step:(s + 1) * step], sc[s * step:(s + 1) * step]
        want_fpr, want_tpr = sk_roc(ls, ss)
        np.testing.assert_array_equal(fpr, want_fpr)
        np.testing.assert_array_equal(tpr, want_tpr)
        w_eer, w_auc, _, _ = scoring_ref.get_eer_auc(ls, ss)
        assert eer == pytest.approx(w_eer, abs=1e-9) and auc == pytest.approx(w_auc, abs=1e-9)
    return got


@pytest.mark.gpu
def test_curve_equals_the_references_golden(eng, golden):
    from speaker_verification_amd import evaluation
    g = golden["scoring"]
    eer, auc, fpr, tpr = evaluation.get_eer_auc_device(g["labels"], g["sims"].astype(np.float32), curve=True)
    assert fpr.dtype == np.float64 and tpr.dtype == np.float64
    np.testing.assert_array_equal(fpr, g["fpr"])
    np.testing.assert_array_equal(tpr, g["tpr"])
    assert eer == pytest.approx(float(g["eer"][0]), abs=1e-9) and auc == pytest.approx(float(g["auc"][0]), abs=1e-9)


@pytest.mark.gpu
def test_curve_bit_identical_to_sklearn(eng):
    rng = np.random.default_rng(10)
    lab = (rng.random(2_000_000) < 0.03).astype(np.uint8)        # the heavy-ties case of test_device_roc_eer
    sc = np.round(rng.standard_normal(2_000_000) + 0.8 * lab, 2).astype(np.float32)
    assert_curve_is_sklearns(eng, lab, sc)
    rng = np.random.default_rng(11)
    lab = (rng.random(1_000_003) < 0.4).astype(np.uint8)         # continuous scores: about one point per pair
    sc = (rng.standard_normal(1_000_003) + lab).astype(np.float32)
    assert_curve_is_sklearns(eng, lab, sc)


@pytest.mark.gpu
def test_curve_edge_inputs(eng):
    rng = np.random.default_rng(12)
    cases = []
    lab = (rng.random(5000) < 0.5).astype(np.uint8)
    lab[:2] = (0, 1)
    cases.append((lab, np.full(5000, 0.25, np.float32)))                                    # all equal
    pm0 = rng.choice(np.array([0.0, -0.0, 0.5, -0.5], np.float32), 7001)                    # +-0.0 one tie group
    cases.append(((rng.random(7001) < 0.3).astype(np.uint8), pm0))
    den = rng.choice(np.array([1e-45, -1e-45, 3e-39, -3e-39, 0.0, -0.0, 1e-38], np.float32), 4099)   # denormals
    cases.append(((rng.random(4099) < 0.5).astype(np.uint8), den))
    cases.append(((rng.random(2049) < 0.2).astype(np.uint8), -rng.random(2049).astype(np.float32) - 1.0))   # all negative
    cases.append((np.array([0, 1], np.uint8), np.array([0.1, 0.3], np.float32)))             # n = 2
    cases.append((np.array([1, 0, 1], np.uint8), np.array([0.2, 0.1, 0.3], np.float32)))     # n = 3
    cases.append((np.array([1, 0, 1], np.uint8), np.array([0.2, 0.2, 0.2], np.float32)))
    for n in (5, 255, 257, 2047, 2049, 4097 + 13, 100_003, 300_007):                      # not a multiple of any tile
        lb = (rng.random(n) < 0.5).astype(np.uint8)
        lb[:2] = (0, 1)
        cases.append((lb, rng.integers(-40, 40, n).astype(np.float32) / 8))
    for lab, sc in cases:
        eer, auc = eng.roc_eer(sc, lab)                                  # the existing entry point on the native sort
        want = assert_curve_is_sklearns(eng, lab, sc)[0]
        assert eer == pytest.approx(want[0], abs=1e-12) and auc == pytest.approx(want[1], abs=1e-12)


@pytest.mark.gpu
def test_non_finite_scores(eng):
    from speaker_verification_amd import _lib
    rng = np.random.default_rng(13)
    lab = (rng.random(10_000) < 0.5).astype(np.uint8)
    sc = rng.standard_normal(10_000).astype(np.float32)
    for bad in (np.inf, -np.inf, np.nan):
        x = sc.copy()
        x[77] = bad
        with pytest.raises(ValueError):
            sk_roc(lab, x)                                             # sklearn rejects them ...
        with pytest.raises(_lib.SvkError, match="split 0.*non-finite"):
            eng.roc_k(x, lab)                                          # ... and so does svk_roc_k
    # svk_roc_eer keeps accepting +-inf: against the torch restatement of the ROC
    x = sc.copy()
    x[::97] = np.inf
    x[5::89] = -np.inf
    f, t = torch_counts(eng.to_device(x), eng.to_device(lab))
    w_eer, w_auc = eer_auc_of_points(f, t)
    eer, auc = eng.roc_eer(x, lab)
    assert eer == pytest.approx(w_eer, abs=1e-12) and auc == pytest.approx(w_auc, abs=1e-12)


@pytest.mark.gpu
def test_k_fold_matches_the_oracle(eng):
    from oracle import scoring_ref
    from speaker_verification_amd import _lib, evaluation
    rng = np.random.default_rng(14)
    n = 100_003                                                       # n % 3 and n % 10 != 0
    lab = (rng.random(n) < 0.1).astype(np.uint8)
    sc = np.round(rng.standard_normal(n) + lab, 3).astype(np.float32)
    for k in (1, 3, 10):
        got = assert_curve_is_sklearns(eng, lab, sc, k=k)
        assert len(got) == k
        w_eer, w_auc = scoring_ref.k_fold_eer_auc(lab, sc, k=k)
        eer, auc = evaluation.get_and_plot_k_eer_auc(lab, sc, k=k, plot_path=None, device=True)
        assert eer == pytest.approx(w_eer, abs=1e-9) and auc == pytest.approx(w_auc, abs=1e-9)
        assert eer == pytest.approx(np.mean([g[0] for g in got]), abs=1e-15)
        plain = eng.roc_k(sc, lab, k=k)
        for p, q in zip(plain, got):                                  # the AUC sums in float64 atomics: order-free to 1e-15
            assert p[0] == pytest.approx(q[0], abs=1e-15) and p[1] == pytest.approx(q[1], abs=1e-15)
    e1, a1 = eng.roc_k(sc, lab, k=1)[0]
    e0, a0 = eng.roc_eer(sc, lab)
    assert e1 == pytest.approx(e0, abs=1e-12) and a1 == pytest.approx(a0, abs=1e-12)
    one = lab.copy()
    one[n // 3:2 * (n // 3)] = 0                                     # split 1 of 3 holds no positive
    with pytest.raises(_lib.SvkError, match="split 1 has only one class"):
        eng.roc_k(sc, one, k=3)
    bad = sc.copy()
    bad[2 * (n // 3) + 5] = np.nan
    with pytest.raises(_lib.SvkError, match="split 2"):
        eng.roc_k(bad, lab, k=3)
    bad[-1] = np.nan                                                  # ... while the ignored tail is never read
    bad[2 * (n // 3) + 5] = 0.0
    eng.roc_k(bad, lab, k=3)
    with pytest.raises(_lib.SvkError):
        eng.roc_k(sc[:5], lab[:5], k=3)                               # step < 2


@pytest.mark.gpu
def test_dev_set_scale(eng):
    """148 642 x 1 211 scores of seeded unit-norm embeddings: the device curves (k = 1, 5) equal the torch-on-GPU
    restatement in counts; eer / auc agree with the float64 NumPy evaluation of that curve to 1e-12."""
    g = torch.Generator(device=eng.device).manual_seed(20)
    test = torch.nn.functional.normalize(torch.randn(148642, 128, device=eng.device, generator=g), dim=1)
    enroll = torch.nn.functional.normalize(torch.randn(1211, 128, device=eng.device, generator=g), dim=1)
    scores = eng.cosine_scores(test, enroll)
    true = torch.randint(-1, 1211, (148642,), device=eng.device, generator=g).to(torch.int32)
    _, _, labels = eng.top1(scores, true, want_labels=True)
    sc, lb = scores.reshape(-1), labels.reshape(-1)
    for k in (1, 5):
        got = eng.roc_k(sc, lb, k=k, curve=True)
        step = sc.numel() // k
        for s, (eer, auc, fpr, tpr) in enumerate(got):
            f, t = torch_counts(sc[s * step:(s + 1) * step], lb[s * step:(s + 1) * step])
            cf, ct = curve_of_counts(f, t)
            np.testing.assert_array_equal(fpr, cf / cf[-1])
            np.testing.assert_array_equal(tpr, ct / ct[-1])
            w_eer, w_auc = eer_auc_of_points(f, t)
            assert eer == pytest.approx(w_eer, abs=1e-12) and auc == pytest.approx(w_auc, abs=1e-12)


@pytest.mark.gpu
def test_past_two_to_the_31_pairs(eng):
    """n = 2^31 + 12 345 pairs (byte offsets past 2^32 in every buffer): 1 000 quantised levels, labels a fixed function
    of the index, so the exact curve follows from per-level counts (torch.bincount)."""
    n = (1 << 31) + 12345
    sc = torch.empty(n, dtype=torch.float32, device=eng.device)
    lb = torch.empty(n, dtype=torch.uint8, device=eng.device)
    tot = torch.zeros(1000, dtype=torch.int64, device=eng.device)
    pos = torch.zeros(1000, dtype=torch.int64, device=eng.device)
    chunk = 1 << 28
    for lo in range(0, n, chunk):
        i = torch.arange(lo, min(n, lo + chunk), dtype=torch.int64, device=eng.device)
        lvl = (i * 7919 + (i >> 9)) % 1000
        y = (((i * 2654435761) >> 13) % 5 == 0) ^ (lvl > 700)
        sc[lo:lo + i.numel()] = (lvl - 500).to(torch.float32) / 64
        lb[lo:lo + i.numel()] = y.to(torch.uint8)
        tot += torch.bincount(lvl, minlength=1000)
        pos += torch.bincount(lvl, weights=y.to(torch.float64), minlength=1000).to(torch.int64)
        del i, lvl, y
    tot, pos = tot.cpu().numpy()[::-1], pos.cpu().numpy()[::-1]       # descending score = descending level
    t = np.cumsum(pos)
    f = np.cumsum(tot) - t
    cf, ct = curve_of_counts(f, t)
    w_eer, w_auc = eer_auc_of_points(f, t)
    eer, auc, fpr, tpr = eng.roc_k(sc, lb, k=1, curve=True)[0]
    np.testing.assert_array_equal(fpr, cf / cf[-1])
    np.testing.assert_array_equal(tpr, ct / ct[-1])
    assert eer == pytest.approx(w_eer, abs=1e-9) and auc == pytest.approx(w_auc, abs=1e-9)
    e0, a0 = eng.roc_eer(sc, lb)
    assert e0 == pytest.approx(w_eer, abs=1e-9) and a0 == pytest.approx(w_auc, abs=1e-9)


@pytest.mark.gpu
def test_top1(eng):
    from speaker_verification_amd import evaluation
    rng = np.random.default_rng(15)
    for rows, cols in ((1000, 1211), (37, 1), (5, 64), (300, 65), (64, 3000)):
        s = np.round(rng.standard_normal((rows, cols)), 1).astype(np.float32)    # ties
        s[rng.random((rows, cols)) < 0.002] = np.nan
        if cols > 2:
            s[3 % rows, :] = np.nan
        s[1 % rows, :] = -np.inf
        true = rng.integers(-1, cols, rows).astype(np.int32)
        amax, correct, labels = eng.top1(s, true, want_labels=True)
        want = np.argmax(s, axis=1)
        np.testing.assert_array_equal(amax.cpu().numpy(), want)
        assert correct == int(np.sum((true >= 0) & (want == true)))
        ids = [f"s{j}" for j in range(cols)]
        test_ids = [ids[t] if t >= 0 else "never" for t in true]
        lab = labels.cpu().numpy()
        ok = true >= 0
        np.testing.assert_array_equal(lab[ok], evaluation.labels_from_ids([t for t, o in zip(test_ids, ok) if o], ids))
        assert not lab[~ok].any()
        np.testing.assert_array_equal(evaluation._true_columns(test_ids, ids), true)
        a2, c2 = eng.top1(s, true)
        assert c2 == correct and torch.equal(a2, amax)


@pytest.mark.gpu
def test_file_driven_evaluate_on_the_device(eng, golden, tmp_path, monkeypatch, capsys):
    """evaluate() with no arguments, device=True against device=False on the synthetic tree of
    test_file_driven_enrol_and_evaluate: same accuracy and printed lines, EER within 1e-9, and the reference's EER."""
    from speaker_verification_amd import constants, evaluation, model as model_mod, synth
    g = golden["round2"]
    root = str(tmp_path)
    data_dir, rel, state = synth.write_verification_tree(root)
    monkeypatch.setattr(constants, "ROOT", root)
    monkeypatch.setattr(constants, "DATA_ORIGIN", data_dir)
    monkeypatch.chdir(tmp_path)
    np.random.seed(int(g["eval_seeds"][0]))
    model_mod.create_speaker_models()
    capsys.readouterr()
    np.random.seed(int(g["eval_seeds"][1]))
    host = evaluation.evaluate()
    out_host = capsys.readouterr().out
    os.remove(tmp_path / "eer_auc.png")
    np.random.seed(int(g["eval_seeds"][1]))
    dev = evaluation.evaluate(device=True)
    out_dev = capsys.readouterr().out
    assert os.path.exists(tmp_path / "eer_auc.png")
    assert isinstance(dev["scores"], torch.Tensor) and dev["scores"].is_cuda and dev["scores"].dtype == torch.float32
    assert dev["labels"].is_cuda and dev["labels"].dtype == torch.uint8
    np.testing.assert_allclose(dev["scores"].cpu().numpy().astype(np.float64), host["scores"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(dev["labels"].cpu().numpy(), host["labels"])
    lines = lambda out: [ln for ln in out.splitlines() if ln.startswith("correct speaker")]   # noqa: E731
    assert lines(out_dev) == lines(out_host) and len(lines(out_dev)) == len(rel)
    assert dev["accuracy"] == host["accuracy"]
    assert dev["eer"] == pytest.approx(host["eer"], abs=1e-9) and dev["auc"] == pytest.approx(host["auc"], abs=1e-9)
    flat = np.sort(g["eval_scores"].flatten())
    if np.diff(flat).min() > 4e-5:
        assert dev["eer"] * 100 == pytest.approx(float(g["eval_eer_pct"][0]), abs=1e-6)


@pytest.mark.gpu
def test_in_memory_evaluate_on_the_device(eng, tmp_path, capsys):
    from speaker_verification_amd import evaluation
    from speaker_verification_amd.model import create_speaker_models, seeded_model
    model = seeded_model(5, n_labels=8).to(eng.device)
    cubes = np.random.default_rng(16).standard_normal((9, 1, 20, 80, 40)).astype(np.float32)
    ids = ["id10001", "id10002", "id10003"] * 3
    create_speaker_models(model, cubes[:3] + 0.5 * cubes[3:6], ids[:3], save_dir=str(tmp_path))
    host = evaluation.evaluate(model, cubes, ids, str(tmp_path), k=3, plot_path=None)
    dev = evaluation.evaluate(model, cubes, ids, str(tmp_path), k=3, plot_path=None, device=True)
    out = capsys.readouterr().out
    np.testing.assert_array_equal(dev["scores"].cpu().numpy().astype(np.float64), host["scores"])
    np.testing.assert_array_equal(dev["labels"].cpu().numpy(), host["labels"])
    assert dev["accuracy"] == host["accuracy"]
    assert dev["eer"] == pytest.approx(host["eer"], abs=1e-9) and dev["auc"] == pytest.approx(host["auc"], abs=1e-9)
    assert "correct speaker" not in out                                # the in-memory host path prints none either
