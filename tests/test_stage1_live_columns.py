"""The 17-column form of the first block (flags bit 5 of svk_c3d2_stage1, svk_c3d2_stage1_c3 and their *_multi forms;
Engine.c3d2_stage1(live_cols=17)): pooled column 17 of the first block's output is read by nothing -- conv2_1 is 4 columns wide
and pool2 drops its 15th output column, so its last live column, 13, ends at pooled column 16 -- and the form neither computes nor
writes it.  Held here: columns 0 .. 16 are the bits of the 18-column call, column 17 keeps what the buffer held, the second block
gives the same bits whatever column 17 holds (a NaN that reached any product would show), and the embedder, which now asks for
17 columns, returns what the seven entries chained by hand behind the 18-column first block return.

Sizes: 1, 8 and 31 cubes = 34, 272 and 1 054 work items -- fewer than one grid of 256 workgroups, just over one, and a little
over four and no multiple of it: at 31 every workgroup runs the whole item pipeline (two items ahead plus a drawn ticket).
Input as tests/test_c3d2_bits.py builds it: feature rows [n, 120, 40] / [n, 3, 120, 40], crop starts in [0, 40], one start at
-5 and one at T - 10 (zero rows: patch_piece_issue's lane-by-lane branch)."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

N, T = 31, 120
SENTINEL = 0x7FC0BEEF             # a quiet NaN with a payload no arithmetic produces
SIZES = (1, 8, 31)
CHAIN = ("stage2", "conv31", "conv32t", "conv41", "conv42", "fc5")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def embedders(eng):
    """{False: the shipped one-channel checkpoint's embedder, True: a seeded three-channel one}; both allow either PReLU form."""
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    model = seeded_model(7, 8, 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), 11))
    out = {False: copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference(),
           True: model.eval().to(eng.device).fused_inference()}
    for fe in out.values():
        assert fe.stage1_tables()[6] is True and fe.stage2_tables()[6] is True, "the slopes must lie in [0, 1] for flags = 2 to be run"
    return out


@pytest.fixture(scope="module")
def inputs(eng):
    """{False: rows [N, T, 40], True: rows [N, 3, T, 40]}, crop starts [N, 20]; the two starts outside the clip are in cubes 0 and 6,
    so every size but the single cube has both."""
    rng = np.random.default_rng(20261021)
    feat3 = (rng.standard_normal((N, 3, T, 40)) * 2.0 - 6.0).astype(np.float32)
    crops = rng.integers(0, 41, (N, 20)).astype(np.int32)
    crops[0, 3] = -5
    crops[6, 11] = T - 10
    feat3, crops = torch.from_numpy(feat3).to(eng.device), torch.from_numpy(crops).to(eng.device)
    return {False: feat3[:, 0].contiguous(), True: feat3}, crops


@pytest.fixture(scope="module")
def full(eng, embedders, inputs):
    """(three, n, slope01, K) -> the 18-column first block's output through the Engine, items from the device-wide counter:
    computed once per key and never written to."""
    cache = {}

    def get(monkeypatch, three, n, slope01, K=None):
        key = (three, n, slope01, K)
        if key not in cache:
            monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)
            feat, crops = _case(inputs, three, n, K)
            cache[key] = eng.c3d2_stage1(feat, crops, _tables(embedders[three].stage1_tables(), slope01))
        return cache[key]
    return get


def _tables(tables, slope01):
    return tuple(tables[:6]) + (bool(slope01),)


def _case(inputs, three, n, K):
    """n cubes: the first n cubes' rows and starts, or (K given) n / K clips with K sets of starts each, [n / K, K, 20]."""
    feats, crops = inputs
    if K is None:
        return feats[three][:n].contiguous(), crops[:n].contiguous()
    return feats[three][:n // K].contiguous(), crops[:n].reshape(n // K, K, 20).contiguous()


def _live17(eng, feat, crops, tables, slope01, K=None):
    """The C entry itself with flags bit 5, on a buffer that holds SENTINEL in every word -> that buffer, [n, 16, 36, 18, 16] int32."""
    three = feat.dim() == 4
    n_clips = feat.shape[0]
    out = torch.full((n_clips * (K or 1), 16, 36, 18, 16), SENTINEL, dtype=torch.int32, device=eng.device)
    fn = getattr(eng.lib, "svk_c3d2_stage1" + ("_c3" if three else "") + ("_multi" if K else ""))
    eng._stream()
    rc = fn(eng.ctx, eng._ptr(feat), n_clips, T, 40, eng._ptr(crops), 20, 80, *(eng._ptr(t) for t in tables[:6]),
            32 | (2 if slope01 else 0), eng._ptr(out), *((K,) if K else ()))
    assert rc == 0, rc
    return out


def _hold_columns(got, want, what):
    want = want.view(torch.int32)
    assert got.shape == want.shape
    assert torch.equal(got[:, :, :, :17], want[:, :, :, :17]), what + ": columns 0 .. 16 differ from the 18-column call"
    assert bool((got[:, :, :, 17] == SENTINEL).all()), what + ": pooled column 17 was written"
    assert not bool((want[:, :, :, 17] == SENTINEL).any())        # (the 18-column call did write it)


def _static_items(monkeypatch, on):
    if on:
        monkeypatch.setenv("SVK_C3D2_STATIC_ITEMS", "1")      # read by the library at every call
    else:
        monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)


@pytest.mark.parametrize("static_items", (False, True), ids=("queued", "static-items"))
@pytest.mark.parametrize("three", (False, True), ids=("one-channel", "three-channel"))
@pytest.mark.parametrize("slope01", (True, False), ids=("slope01", "any"))
@pytest.mark.parametrize("n", SIZES)
def test_columns(eng, embedders, inputs, full, monkeypatch, n, slope01, three, static_items):
    want = full(monkeypatch, three, n, slope01)
    _static_items(monkeypatch, static_items)
    feat, crops = _case(inputs, three, n, None)
    got = _live17(eng, feat, crops, embedders[three].stage1_tables(), slope01)
    _hold_columns(got, want, "n %d" % n)


@pytest.mark.parametrize("static_items", (False, True), ids=("queued", "static-items"))
@pytest.mark.parametrize("three", (False, True), ids=("one-channel", "three-channel"))
@pytest.mark.parametrize("slope01", (True, False), ids=("slope01", "any"))
def test_columns_two_cubes_per_clip(eng, embedders, inputs, full, monkeypatch, slope01, three, static_items):
    """K = 2 cubes on each of 4 clips (the *_multi entries)."""
    want = full(monkeypatch, three, 8, slope01, 2)
    _static_items(monkeypatch, static_items)
    feat, crops = _case(inputs, three, 8, 2)
    got = _live17(eng, feat, crops, embedders[three].stage1_tables(), slope01, 2)
    _hold_columns(got, want, "4 clips x 2 cubes")


@pytest.mark.parametrize("two_kernels", (False, True), ids=("streamed", "two-kernels"))
@pytest.mark.parametrize("n", SIZES)
def test_second_block_does_not_read_column_17(eng, embedders, inputs, full, monkeypatch, n, two_kernels):
    """svk_c3d2_stage2 on the output whose column 17 is NaN in every word = svk_c3d2_stage2 on the whole output, bit for bit, by the
    streamed kernel and by the two-kernel reference path (which stages the column into LDS and multiplies none of it)."""
    fe = embedders[False]
    want1 = full(monkeypatch, False, n, True)
    feat, crops = _case(inputs, False, n, None)
    got1 = _live17(eng, feat, crops, fe.stage1_tables(), True).view(torch.float32)
    assert bool(torch.isnan(got1[:, :, :, 17]).all())
    if two_kernels:
        monkeypatch.setenv("SVK_C3D2_STAGE2_TWO_KERNELS", "1")
    else:
        monkeypatch.delenv("SVK_C3D2_STAGE2_TWO_KERNELS", raising=False)
    want = eng.c3d2_stage2(want1, fe.stage2_tables())
    got = eng.c3d2_stage2(got1, fe.stage2_tables())
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("case", ("one-channel", "three-channel", "two-cubes-per-clip"))
def test_embeddings(eng, embedders, inputs, monkeypatch, case):
    """FusedEmbedder.embed_features (17 live columns) = the seven entries chained by hand behind the 18-column first block."""
    monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)
    monkeypatch.delenv("SVK_C3D2_STAGE2_TWO_KERNELS", raising=False)
    three, K = case == "three-channel", 2 if case == "two-cubes-per-clip" else None
    n = N - 1 if K else N
    fe = embedders[three]
    feat, crops = _case(inputs, three, n, K)
    y = eng.c3d2_stage1(feat, crops, fe.stage1_tables())
    for k in CHAIN:
        y = getattr(eng, "c3d2_" + k)(y, getattr(fe, k + "_tables")())
    got = fe.embed_features(feat, crops)
    assert tuple(got.shape) == ((n // K, K, 128) if K else (n, 128)) and bool(torch.isfinite(got).all())
    assert torch.equal(got.reshape(n, 128), y)


def test_flags(eng):
    """Bits 1 and 5 are defined, alone or together; every other bit is SVK_ERR_BAD_ARG as before (n_utt = 0: nothing is launched)."""
    from speaker_verification_amd import _lib
    none6 = (None,) * 6
    for name in ("svk_c3d2_stage1", "svk_c3d2_stage1_c3", "svk_c3d2_stage1_multi", "svk_c3d2_stage1_c3_multi"):
        fn, extra = getattr(eng.lib, name), ((1,) if name.endswith("_multi") else ())
        for flags in (32, 34):
            assert fn(eng.ctx, None, 0, 100, 40, None, 20, 80, *none6, flags, None, *extra) == _lib.SVK_OK, (name, flags)
        for flags in (1, 4, 8, 16, 64, 33):
            assert fn(eng.ctx, None, 0, 100, 40, None, 20, 80, *none6, flags, None, *extra) == _lib.SVK_ERR_BAD_ARG, (name, flags)


def test_live_cols_argument(eng, embedders, inputs):
    """Engine.c3d2_stage1: live_cols is 18 or 17, anything else raises before any launch."""
    feat, crops = _case(inputs, False, 1, None)
    for bad in (0, 16, 19, None):
        with pytest.raises(ValueError, match="live_cols"):
            eng.c3d2_stage1(feat, crops, embedders[False].stage1_tables(), live_cols=bad)
