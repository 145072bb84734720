"""C3D2's classification head on libsvk (`svk_c3d2_head`, csrc/head.hip): PReLU5 -> FC6 -> softmax of model.py:170-174, the
top-k of those probabilities and the hit counts of train.py:104-119's accuracy pass; `C3D2.fused_head`, `C3D2.identify`,
`head_kernels` routing and `evaluation.identification_accuracy`.  The float64 restatement of the head lives here."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CHECKPOINT = os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt")


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_head_symbol_in_header_binding_and_library():
    from speaker_verification_amd import _lib
    with open(os.path.join(REPO, "include", "svk.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint svk_c3d2_head\(", header)
    assert int(re.search(r"#define SVK_VERSION (\d+)", header).group(1)) == _lib.VERSION == 114
    assert "svk_c3d2_head" in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "svk_c3d2_head")
    assert _lib.load().svk_version() == 114


@pytest.mark.parametrize("n_labels", [1211, 100])
def test_fused_head_tables_round_trip(n_labels):
    from speaker_verification_amd.model import C3D2
    torch.manual_seed(n_labels)
    model = C3D2(n_labels, 1).eval()
    with torch.no_grad():
        model.PReLu5.weight.fill_(0.171875)
    w6, b6, slope = model.fused_head().tables()
    assert w6.dtype == b6.dtype == torch.float32 and tuple(w6.shape) == (n_labels, 128)
    assert torch.equal(w6, model.FC6.weight.detach()) and torch.equal(b6, model.FC6.bias.detach())
    assert slope == float(model.PReLu5.weight.detach())


def test_head_cache_follows_fc6_not_conv_weights():
    from speaker_verification_amd.model import C3D2
    model = C3D2(100, 1).eval()
    head = model.fused_head()
    assert model.fused_head() is head
    with torch.no_grad():
        model.conv1_1.weight.mul_(2.0)                  # the embedder's business, not the head's
    assert model.fused_head() is head
    with torch.no_grad():
        model.FC6.weight.add_(1.0)
    rebuilt = model.fused_head()
    assert rebuilt is not head and torch.equal(rebuilt.w6, model.FC6.weight.detach())
    with torch.no_grad():
        model.PReLu5.weight.fill_(0.5)
    assert model.fused_head() is not rebuilt and model.fused_head().slope == 0.5


def test_head_kernels_off_by_default():
    from speaker_verification_amd.model import C3D2
    assert C3D2.head_kernels is False and C3D2(10, 1).head_kernels is False


def test_identify_torch_fallback_on_host():
    """On host tensors identify takes torch's softmax and a stable sort: ties to the lower label."""
    from speaker_verification_amd.model import C3D2
    model = C3D2(6, 1).eval()
    with torch.no_grad():
        model.FC6.weight.zero_()
        model.FC6.bias.copy_(torch.tensor([0.0, 2.0, 1.0, 2.0, -1.0, 1.0]))
    emb = torch.randn(3, 128)
    top, hits = model.identify(emb, k=4, true_idx=[3, -1, 7])
    assert top.dtype == torch.int32 and top.tolist() == [[1, 3, 2, 5]] * 3
    assert hits == [0, 1, 1, 1]


# ---- GPU ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _tables(n_labels, seed, dev, slope=0.23):
    g = torch.Generator().manual_seed(seed)
    w = (0.1 * torch.randn(n_labels, 128, generator=g)).to(dev)
    b = (0.5 * torch.randn(n_labels, generator=g)).to(dev)
    return w, b, slope


def _emb(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 128, generator=g).to(dev)


def _f64_probs(emb, tables):
    w, b, slope = tables
    x = emb.double()
    z = torch.where(x > 0, x, slope * x)
    return torch.softmax(z @ w.double().t() + b.double(), dim=1)


def _torch_probs(emb, tables):
    w, b, slope = tables
    z = torch.nn.functional.prelu(emb, torch.tensor([slope], device=emb.device))
    return torch.softmax(torch.nn.functional.linear(z, w, b), dim=1)


def _stable_topk(p, k):
    return torch.sort(p, dim=1, descending=True, stable=True)[1][:, :k].to(torch.int32)


def _check_rule1(p, emb, tables, tag):
    """max |kernel - f64| / max p <= 2 max |torch f32 - f64| / max p + 2^-24, and rows sum to 1 within 1e-6."""
    ref = _f64_probs(emb, tables)
    scale = float(ref.max())
    err_k = float((p.double() - ref).abs().max()) / scale
    err_t = float((_torch_probs(emb, tables).double() - ref).abs().max()) / scale
    assert err_k <= 2 * err_t + 2.0 ** -24, (tag, err_k, err_t)
    assert float((p.double().sum(1) - 1).abs().max()) <= 1e-6, tag
    return err_k, err_t


@pytest.mark.gpu
@pytest.mark.parametrize("n_labels", [1, 2, 17, 100, 1211, 1251, 5994, 65536])
def test_head_against_float64(eng, n_labels):
    dev = eng.device
    tables = _tables(n_labels, n_labels, dev)
    k = min(5, n_labels)
    for n in (0, 1, 15, 16, 17, 4874):
        emb = _emb(n, 1000 + n, dev)
        p, top, hits = eng.c3d2_head(emb, tables, probs=True, k=k)
        assert hits is None and p.shape == (n, n_labels) and top.shape == (n, k)
        p2, top2, _ = eng.c3d2_head(emb, tables, probs=False, k=k)
        assert p2 is None and torch.equal(top, top2)
        if n == 0:
            continue
        err_k, err_t = _check_rule1(p, emb, tables, (n_labels, n))
        assert torch.equal(top, _stable_topk(p, k))
        if n == 4874:
            print("n_labels %5d: max error / max p %.2e (kernel) vs %.2e (torch f32)" % (n_labels, err_k, err_t))


@pytest.mark.gpu
def test_head_edges(eng):
    dev = eng.device
    w, b, slope = _tables(40, 7, dev)
    w[11] = w[3]                                       # exact duplicates: equal logits, equal p
    b[11] = b[3]
    w[30] = w[3]
    b[30] = b[3]
    b[3] += 20.0                                       # make that triple the top three
    b[11] += 20.0
    b[30] += 20.0
    emb = _emb(64, 8, dev)
    p, top, _ = eng.c3d2_head(emb, (w, b, slope), k=8)
    assert torch.equal(p[:, 3], p[:, 11]) and torch.equal(p[:, 3], p[:, 30])
    assert top[:, :3].tolist() == [[3, 11, 30]] * 64
    assert torch.equal(top, _stable_topk(p, 8))

    # saturating finite logits: exact one-hot, as torch gives
    bs = torch.full((50,), -1e4, device=dev)
    bs[17] = 1e4
    ws = _tables(50, 9, dev)[0]
    p, top, _ = eng.c3d2_head(emb, (ws, bs, slope), k=3)
    want = torch.zeros_like(p)
    want[:, 17] = 1.0
    assert torch.equal(p, want) and torch.equal(p, _torch_probs(emb, (ws, bs, slope)))
    assert top.tolist() == [[17, 0, 1]] * 64

    # a NaN embedding row: a NaN probability row, top-1 its first NaN (torch.argmax), the other rows untouched
    e = emb.clone()
    e[5, 9] = float("nan")
    p, top, _ = eng.c3d2_head(e, (w, b, slope), k=4)
    p0, top0, _ = eng.c3d2_head(emb, (w, b, slope), k=4)
    assert bool(torch.isnan(p[5]).all()) and int(torch.argmax(p[5])) == int(top[5, 0]) == 0
    assert top[5].tolist() == [0, 1, 2, 3] and torch.equal(top, _stable_topk(p, 4))
    rest = torch.arange(64, device=dev) != 5
    assert torch.equal(p[rest], p0[rest]) and torch.equal(top[rest], top0[rest])

    # one label: p = 1
    p, top, hits = eng.c3d2_head(emb, (w[:1].contiguous(), b[:1].contiguous(), slope), k=1, true_idx=[0] * 63 + [-1])
    assert bool((p == 1).all()) and bool((top == 0).all()) and hits == [63]

    # hits: -1 and out-of-range labels never count
    p, top, _ = eng.c3d2_head(emb, (w, b, slope), k=5)
    true = top[:, 2].clone()
    true[:4] = -1
    true[4:8] = 40
    true[8:10] = 1 << 20
    true[10] = top[10, 0]
    _, _, hits = eng.c3d2_head(emb, (w, b, slope), probs=False, k=5, true_idx=true)
    assert hits == [1, 1, 54, 54, 54]


@pytest.mark.gpu
def test_head_refused_arguments(eng):
    from speaker_verification_amd import _lib
    lib, ctx = eng.lib, eng.ctx
    dev = eng.device
    w, b, slope = _tables(10, 3, dev)
    emb = _emb(4, 3, dev)
    top = torch.empty((4, 16), dtype=torch.int32, device=dev)
    tr = torch.zeros(4, dtype=torch.int32, device=dev)
    hits = (ctypes.c_int64 * 16)()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(n=4, n_labels=10, wp=w, bp=b, k=1, tp=top, trp=None, hp=hits):
        return lib.svk_c3d2_head(ctx, P(emb), n, n_labels, slope, P(wp), P(bp), None, k, P(tp), P(trp), hp)

    assert call() == _lib.SVK_OK
    assert call(k=11) == _lib.SVK_ERR_BAD_ARG                       # k > n_labels
    assert call(k=0) == _lib.SVK_ERR_BAD_ARG
    assert call(k=0, tp=None, trp=tr) == _lib.SVK_ERR_BAD_ARG
    assert call(wp=None) == _lib.SVK_ERR_BAD_ARG
    assert call(bp=None) == _lib.SVK_ERR_BAD_ARG
    assert call(n=-1) == _lib.SVK_ERR_BAD_ARG
    assert call(n_labels=0) == _lib.SVK_ERR_BAD_ARG
    assert call(trp=tr, hp=None) == _lib.SVK_ERR_BAD_ARG
    assert call(k=9, n_labels=10) == _lib.SVK_ERR_UNSUPPORTED       # k > 8
    assert call(n_labels=65537) == _lib.SVK_ERR_UNSUPPORTED
    assert call(k=0, tp=None) == _lib.SVK_OK                        # nothing ranked: k is not read
    assert call(n=0, trp=tr) == _lib.SVK_OK and hits[0] == 0        # n = 0: no launch, hits zeroed
    with pytest.raises(_lib.SvkError):
        eng.c3d2_head(emb, (w, b, slope), k=9)


@pytest.mark.gpu
def test_head_deterministic_and_batch_independent(eng):
    dev = eng.device
    tables = _tables(1211, 5, dev)
    emb = _emb(4874, 6, dev)
    true = torch.randint(-1, 1211, (4874,), generator=torch.Generator().manual_seed(1)).to(dev)
    p, top, hits = eng.c3d2_head(emb, tables, k=8, true_idx=true)
    p2, top2, hits2 = eng.c3d2_head(emb, tables, k=8, true_idx=true)
    assert torch.equal(p, p2) and torch.equal(top, top2) and hits == hits2
    for a, b_ in ((0, 1), (1, 17), (17, 33), (1000, 4874), (4873, 4874), (37, 2000)):
        pa, ta, _ = eng.c3d2_head(emb[a:b_], tables, k=8)
        assert torch.equal(pa, p[a:b_]) and torch.equal(ta, top[a:b_]), (a, b_)
    _, t3, _ = eng.c3d2_head(emb, tables, probs=False, k=3)
    assert torch.equal(t3, top[:, :3])
    got = torch.zeros(8, dtype=torch.int64)
    for lo in range(0, 4874, 1000):
        got += torch.tensor(eng.c3d2_head(emb[lo:lo + 1000], tables, probs=False, k=8, true_idx=true[lo:lo + 1000])[2])
    assert got.tolist() == hits


def _golden_c3d2_model(g, channels):
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    model = seeded_model(int(g["init_seed"][0]), int(g["n_labels"][0]), channels)
    model.load_state_dict(perturb_inference_state(model.state_dict(), int(g["perturb_seed"][0])))
    return model.eval()


@pytest.mark.gpu
def test_head_kernels_reference_parity(eng):
    from speaker_verification_amd.model import C3D2
    dev = eng.device
    # c3d2_embed.npz: the seeded one-channel model, softmax row 0's first eight
    g = np.load(os.path.join(GOLDEN, "c3d2_embed.npz"), allow_pickle=False)
    model = _golden_c3d2_model(g, 1).to(dev)
    model.head_kernels = True
    cubes = (np.random.default_rng(int(g["cube_seed"][0])).standard_normal((3, 1, 20, 80, 40)) * 2.0 - 6.0).astype(np.float32)
    x = torch.from_numpy(cubes).to(dev)
    assert model.runs_on_kernels(x)
    with torch.no_grad():
        probs = model(x)
    emb = model.fused_inference()(x)
    assert torch.equal(probs, model.fused_head()(emb, k=None)[0])
    np.testing.assert_allclose(probs.cpu().numpy()[0, :8], g["softmax_row0_top"], rtol=1e-3, atol=1e-7)
    # c3d2_3c.npz: the reference's full [3, 1211] softmax of the three-channel model
    g3 = np.load(os.path.join(GOLDEN, "c3d2_3c.npz"), allow_pickle=False)
    m3 = _golden_c3d2_model(g3, 3).to(dev)
    m3.three_channel_kernels = True
    m3.head_kernels = True
    x3 = torch.from_numpy((np.random.default_rng(int(g3["cube_seed"][0])).standard_normal((3, 3, 20, 80, 40)) * 2.0 - 6.0
                           ).astype(np.float32)).to(dev)
    with torch.no_grad():
        p3 = m3(x3)
    np.testing.assert_allclose(p3.cpu().numpy(), g3["softmax"], rtol=1e-3, atol=1e-7)
    # round4.npz: the trained checkpoint
    from speaker_verification_amd import synth
    from speaker_verification_amd.pipeline import VerificationPipeline
    g4 = np.load(os.path.join(GOLDEN, "round4.npz"), allow_pickle=False)
    ck = torch.load(CHECKPOINT, map_location="cpu", weights_only=True)
    m4 = C3D2(100, 1).load_checkpoint(ck)
    m4.eval()
    m4.head_kernels = True
    pcm = np.stack([synth.speaker_clip(int(s), int(u)) for s, u in g4["clip_ids"]])
    pipe = VerificationPipeline(m4, use_vad=False, normalize=True, preemph_cof=0.98, micro_batch=3)
    _, inter = pipe.embed(pcm, crop_idx=g4["crop_idx"], return_intermediates=True)
    cubes4 = torch.cat([d["cube"] for d in inter])
    with torch.no_grad():
        p4 = m4(cubes4)
    np.testing.assert_allclose(p4.cpu().numpy()[:, :8], g4["softmax_top"], rtol=1e-3, atol=1e-6)


def _trained_model(dev):
    from speaker_verification_amd.model import C3D2
    ck = torch.load(CHECKPOINT, map_location="cpu", weights_only=True)
    model = C3D2(100, 1)
    model.load_state_dict(ck["state_dict"])
    return model.to(dev).eval()


def _near_ties(p, r):
    """Rows whose probability margin between rank r and r + 1 (0-based r) is under 1e-5 relative."""
    s = torch.sort(p, dim=1, descending=True, stable=True)[0]
    return ((s[:, r] - s[:, r + 1]) < 1e-5 * s[:, r]).cpu().numpy()


@pytest.mark.gpu
def test_identification_end_to_end(eng, tmp_path, monkeypatch):
    """The trained checkpoint on unseen recordings of its 100 training speakers (synth.speaker_clip from speaker 2000, the
    front end of checkpoints/c3d2_synth.json): kernel top-1 / top-5 against torch's softmax + sort on the same embeddings."""
    import json
    from speaker_verification_amd import evaluation, synth
    from speaker_verification_amd.pipeline import VerificationPipeline
    dev = eng.device
    with open(os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.json")) as fh:
        meta = json.load(fh)["meta"]
    assert meta["front_end"].startswith("energy VAD -> preemphasis(0.98)") and meta["front_end"].endswith("cmvn(variance)")
    model = _trained_model(dev)
    first, n_spk, utts = int(meta["first_speaker"]), int(meta["speakers"]), 3
    pcm = np.stack([synth.speaker_clip(first + s, 200 + u) for s in range(n_spk) for u in range(utts)])
    true = np.repeat(np.arange(n_spk, dtype=np.int32), utts)
    pipe = VerificationPipeline(model, use_vad=True, normalize=True, preemph_cof=0.98)
    emb = pipe.embed(pcm)
    top, hits = model.identify(emb, k=5, true_idx=true)
    with torch.no_grad():
        p = torch.softmax(model.FC6(model.PReLu5(emb)), dim=1)
    ref = _stable_topk(p, 5)
    t = torch.from_numpy(true).to(dev)
    loose1 = _near_ties(p, 0)
    loose5 = _near_ties(p, 4)
    d1 = (top[:, 0] != ref[:, 0]).cpu().numpy()
    d5 = np.array([set(a) != set(b) for a, b in zip(top.tolist(), ref.tolist())])
    assert not (d1 & ~loose1).any() and not (d5 & ~loose5).any()
    ref1 = int((ref[:, 0] == t).sum())
    ref5 = int((ref == t[:, None]).any(1).sum())
    assert abs(hits[0] - ref1) <= int(loose1.sum()) and abs(hits[4] - ref5) <= int(loose5.sum())
    print("identification, %d clips of %d training speakers: top-1 %.1f %%, top-5 %.1f %% (torch %.1f / %.1f %%); near ties "
          "at rank 1: %d, at rank 5: %d" % (len(true), n_spk, 100 * hits[0] / len(true), 100 * hits[4] / len(true),
                                             100 * ref1 / len(true), 100 * ref5 / len(true), loose1.sum(), loose5.sum()))
    assert hits[0] / len(true) > 0.1                     # 100 classes: chance is 1 %

    # the file-driven path (an AudioDataset over a written tree) equals the in-memory one on the same crop draws
    from speaker_verification_amd import constants
    from speaker_verification_amd.utils import create_dataset
    root = str(tmp_path)
    data_dir, rel, _ = synth.write_verification_tree(root, n_speakers=6, utts_per_speaker=3, n_samples=40000,
                                                     checkpoint=CHECKPOINT)
    monkeypatch.setattr(constants, "DATA_ORIGIN", data_dir)
    monkeypatch.setattr(constants, "NORMALIZE", True)
    indexed = evaluation.load_indexed_labels(os.path.join(root, "50_first_ids.npy"))
    ds = create_dataset(indexed_labels=indexed, origin_file_path=os.path.join(root, "50_first_ids.txt"))
    np.random.seed(5)
    acc = evaluation.identification_accuracy(model, ds, topk=(1, 5))
    np.random.seed(5)
    emb_f = evaluation.dataset_embeddings(ds, model)
    labels = np.array([indexed[f[0:7]] for f in ds.sound_files], dtype=np.int32)
    top_f, hits_f = model.identify(emb_f, k=5, true_idx=labels)
    assert acc["n"] == len(ds) == 18
    assert np.array_equal(acc["predicted"], top_f[:, 0].cpu().numpy())
    assert acc["top1"] == 100.0 * hits_f[0] / 18 and acc["top5"] == 100.0 * hits_f[4] / 18
    # and the cube form of identification_accuracy agrees with identify on cubes
    _, inter = pipe.embed(pcm[:40], return_intermediates=True)
    cubes = torch.cat([d["cube"] for d in inter])
    acc_c = evaluation.identification_accuracy(model, cubes, labels=true[:40], topk=(1, 5), batch=16)
    top_c, hits_c = model.identify(cubes, k=5, true_idx=true[:40])
    assert np.array_equal(acc_c["predicted"], top_c[:, 0].cpu().numpy()) and acc_c["top1"] == 100.0 * hits_c[0] / 40


@pytest.mark.gpu
def test_head_past_2_31_elements(eng):
    """n = 1 800 000 rows x 1 211 labels: 2.18e9 probabilities (8.7 GB), 64-bit offsets."""
    dev = eng.device
    n, n_labels = 1_800_000, 1211
    tables = _tables(n_labels, 9, dev)
    emb = _emb(n, 10, dev)
    true = torch.randint(-1, n_labels, (n,), generator=torch.Generator().manual_seed(2)).to(dev)
    p, top, hits = eng.c3d2_head(emb, tables, k=5, true_idx=true)
    assert n * n_labels > 2 ** 31
    _check_rule1(p[-4096:], emb[-4096:], tables, "last rows")
    idx = torch.arange(0, n, 439, device=dev)
    _check_rule1(p[idx], emb[idx], tables, "strided rows")
    assert torch.equal(top[-4096:], _stable_topk(p[-4096:], 5))
    del p
    torch.cuda.empty_cache()
    got = torch.zeros(5, dtype=torch.int64)
    for lo in range(0, n, 4096):
        _, t, h = eng.c3d2_head(emb[lo:lo + 4096], tables, probs=False, k=5, true_idx=true[lo:lo + 4096])
        assert torch.equal(t, top[lo:lo + 4096])
        got += torch.tensor(h)
    assert got.tolist() == hits
