"""The streamed second block (c3d2_stage2h_kernel: conv2_1 handed to conv2_2 by depth through LDS) against the two kernels it
replaces (c3d2_conv21h_kernel + c3d2_conv22h_kernel through the d_act2 scratch, selected with SVK_C3D2_STAGE2_TWO_KERNELS, which
the library reads at every call).  Every output of both layers receives the same blocks in the same order from the bias on
either path, so the comparison is torch.equal throughout: no tolerance.

n = 1 is fewer items than workgroups, n = 75 is 525 items: on a 256-CU card some workgroup runs a third item, so the rings are
reused and one item's drain overlaps the next item's fill.  The one-plane inputs pin down ring-slot and column-halo indexing: a
(depth, column) plane of the input reaches conv2_1's output depths d - 2 .. d and columns w - 3 .. w only."""
import copy

import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_host_logic)

SWITCH = "SVK_C3D2_STAGE2_TWO_KERNELS"
STATIC = "SVK_C3D2_STATIC_ITEMS"
SIZES = (1, 2, 75)
PLANES = ((0, 0), (15, 17), (7, 4), (8, 5))


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def fe(eng):
    return copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()


@pytest.fixture(scope="module")
def inputs(eng):
    """{(distribution, n): the kernel's input [n, 16, 36, 18, 16] on the device}: N(0, 1) and N(-6, 2), made once."""
    gen = torch.Generator().manual_seed(2207)
    out = {}
    for name, mean, std in (("N(0,1)", 0.0, 1.0), ("N(-6,2)", -6.0, 2.0)):
        x = torch.randn((max(SIZES), 16, 36, 18, 16), generator=gen) * std + mean
        for n in SIZES:
            out[name, n] = x[:n].contiguous().to(eng.device)
    return out


def _tables(fe, slope01):
    t = list(fe.stage2_tables())
    assert len(t) == 7 and isinstance(t[6], bool)
    t[6] = slope01
    return t


def _run(eng, fe, xk, slope01, monkeypatch, two_kernels, static=False):
    for name, on in ((SWITCH, two_kernels), (STATIC, static)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    out = eng.c3d2_stage2(xk, _tables(fe, slope01))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def two_kernel_outputs():
    """The two-kernel outputs, computed once per (distribution, n, slope flag) and left unchanged."""
    return {}


def _reference(cache, key, eng, fe, xk, slope01, monkeypatch):
    if key not in cache:
        cache[key] = _run(eng, fe, xk, slope01, monkeypatch, two_kernels=True)
    return cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("static", (False, True), ids=("queued", "static"))
@pytest.mark.parametrize("slope01", (True, False), ids=("slope01", "any-slope"))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", ("N(0,1)", "N(-6,2)"))
def test_streamed_equals_two_kernels(eng, fe, inputs, two_kernel_outputs, monkeypatch, dist, n, slope01, static):
    xk = inputs[dist, n]
    want = _reference(two_kernel_outputs, (dist, n, slope01), eng, fe, xk, slope01, monkeypatch)
    got = _run(eng, fe, xk, slope01, monkeypatch, two_kernels=False, static=static)
    assert tuple(got.shape) == (n, 12, 15, 7, 32)
    assert bool(want.abs().max() > 0)
    assert torch.equal(got, want), "%d of %d elements differ" % (int((got != want).sum()), got.numel())


@pytest.mark.gpu
@pytest.mark.parametrize("slope01", (True, False), ids=("slope01", "any-slope"))
@pytest.mark.parametrize("plane", PLANES, ids=["d%d-w%d" % p for p in PLANES])
def test_one_plane_inputs(eng, fe, monkeypatch, plane, slope01):
    """Zero except one (depth, column) plane of the input: still bit-equal, and where it differs says which ring slot or halo column."""
    d, w = plane
    gen = torch.Generator().manual_seed(100 * d + w)
    x = torch.zeros((2, 16, 36, 18, 16))
    x[:, d, :, w, :] = torch.randn((2, 36, 16), generator=gen)
    xk = x.to(eng.device)
    want = _run(eng, fe, xk, slope01, monkeypatch, two_kernels=True)
    got = _run(eng, fe, xk, slope01, monkeypatch, two_kernels=False)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, "first differing [cube, depth, row, column, channel]: %s (%d in all)" % (bad[0].tolist(), bad.shape[0])


def _call(eng, fe, xk, act2, out):
    """svk_c3d2_stage2 itself, with the scratch pointer as given (None = NULL) -> its status."""
    args = eng._c3d2_layers(_tables(fe, True), ((2, 6, 2, 64, 8), (2, 24, 2, 64, 8)), torch.float16, 32)
    eng._stream()
    rc = eng.lib.svk_c3d2_stage2(eng.ctx, eng._ptr(xk), xk.shape[0], *args, None if act2 is None else eng._ptr(act2), eng._ptr(out))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
def test_scratch_is_never_touched(eng, fe, inputs, monkeypatch):
    from speaker_verification_amd import _lib
    xk = inputs["N(0,1)", 2]
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(STATIC, raising=False)
    sentinel = torch.full((2, 14, 36, 14, 32), -12345.0, device=eng.device)
    out_a, out_b = (torch.empty((2, 12, 15, 7, 32), device=eng.device) for _ in range(2))
    assert _call(eng, fe, xk, sentinel, out_a) == _lib.SVK_OK
    assert bool((sentinel == -12345.0).all()), "the streamed path wrote to d_act2"
    assert _call(eng, fe, xk, None, out_b) == _lib.SVK_OK
    assert torch.equal(out_a, out_b)
    monkeypatch.setenv(SWITCH, "1")
    assert _call(eng, fe, xk, None, out_b) == _lib.SVK_ERR_BAD_ARG
    assert _call(eng, fe, xk, sentinel, out_b) == _lib.SVK_OK
    assert torch.equal(out_a, out_b) and not bool((sentinel == -12345.0).all())


@pytest.mark.gpu
def test_streamed_repeats(eng, fe, inputs, monkeypatch):
    """Two streamed calls on the same input give the same bits: a missing barrier between ring slots shows here."""
    xk = inputs["N(-6,2)", 75]
    a = _run(eng, fe, xk, True, monkeypatch, two_kernels=False)
    b = _run(eng, fe, xk, True, monkeypatch, two_kernels=False)
    assert torch.equal(a, b)
