"""The first and second block on oddly placed buffers.  The second block's producers fetch their input through a wave-uniform
base and per-lane 32-bit offsets computed once per kernel; the first block's patch DMA adds a lane's constant part to a piece's
wave-uniform base (as one scalar-base instruction in tools/experiments/stage1_patch_fetch_scalar_base.patch).  In either form
nothing may depend on where a buffer starts beyond the alignment the C-ABI asks for: 16 bytes for svk_c3d2_stage2's buffers, 8
bytes for d_feat of the first block.  Every comparison is torch.equal: the same call on the same data elsewhere in memory gives
the same bits.

  * second block: input [n, 16, 36, 18, 16] and output as views 16 bytes into larger allocations (16-aligned, not 64-aligned), the
    streamed kernel against SVK_C3D2_STAGE2_TWO_KERNELS on the same views; n = 3 (21 items: a workgroup gets none or one), queued
    and static items, both slope flags; n = 75 (525 items: a third item for some workgroup of a 256-CU card) with one flag.
  * first block: feature rows of max_frames = 120 as a view 8 bytes into a larger allocation against a fresh 256-byte-aligned copy,
    for svk_c3d2_stage1, svk_c3d2_stage1_c3 and both with cubes_per_clip = 2 (the _multi entries); crop starts 0, 40 (the patch's
    last row is the clip's last row), 41 (one row past the clip), -1 and 119 (the lane-by-lane path) among ordinary ones.  The
    one-channel output on the view also passes reference (A) of tests/c3d2_f64_ref.py, as tests/test_c3d2_float64.py applies it."""
import copy

import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_host_logic)

SWITCH = "SVK_C3D2_STAGE2_TWO_KERNELS"
STATIC = "SVK_C3D2_STATIC_ITEMS"
T = 120                           # max_frames of the first-block cases
SPECIAL_STARTS = (0, 40, 41, -1, 119)


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def fe(eng):
    return copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()


@pytest.fixture(scope="module")
def fe3(eng):
    """A three-channel model with non-trivial BatchNorm statistics and slopes (no trained three-channel checkpoint ships)."""
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    model = seeded_model(31, 4, 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), 32))
    return model.eval().to(eng.device).fused_inference()


def _offset_view(eng, shape, offset_floats, fill=None):
    """-> (buffer, view): `view` of `shape` starts offset_floats floats into `buffer`, which has four guard floats behind it."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.empty(offset_floats + numel + 4, dtype=torch.float32, device=eng.device)
    if fill is not None:
        buf.fill_(fill)
    assert buf.data_ptr() % 256 == 0
    view = buf[offset_floats:offset_floats + numel].view(shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * offset_floats
    return buf, view


# ---- second block ---------------------------------------------------------------------------------------------------------
def _stage2(eng, fe, xk, out, slope01, scratch):
    tables = list(fe.stage2_tables())
    tables[6] = slope01
    args = eng._c3d2_layers(tables, ((2, 6, 2, 64, 8), (2, 24, 2, 64, 8)), torch.float16, 32)
    eng._stream()
    rc = eng.lib.svk_c3d2_stage2(eng.ctx, eng._ptr(xk), xk.shape[0], *args, eng._ptr(scratch), eng._ptr(out))
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def stage2_views(eng):
    """{n: (input buffer, input view, output buffer, output view)}: N(0, 1) inputs, made once; both views 16 bytes into their
    allocations."""
    gen = torch.Generator().manual_seed(1208)
    x = torch.randn((75, 16, 36, 18, 16), generator=gen)
    out = {}
    for n in (3, 75):
        ibuf, iview = _offset_view(eng, (n, 16, 36, 18, 16), 4, fill=-7.0)
        iview.copy_(x[:n])
        obuf, oview = _offset_view(eng, (n, 12, 15, 7, 32), 4)
        assert iview.data_ptr() % 64 == 16 and oview.data_ptr() % 64 == 16
        out[n] = (ibuf, iview, obuf, oview)
    return out


@pytest.fixture(scope="module")
def stage2_two_kernel_outputs():
    """The two-kernel outputs on the views, computed once per (n, slope flag) and left unchanged."""
    return {}


def _stage2_case(eng, fe, views, cache, monkeypatch, n, slope01, static):
    from speaker_verification_amd import _lib
    _, xk, obuf, out = views[n]
    monkeypatch.delenv(STATIC, raising=False)
    if (n, slope01) not in cache:
        monkeypatch.setenv(SWITCH, "1")
        scratch = torch.empty((n, 14, 36, 14, 32), dtype=torch.float32, device=eng.device)
        assert _stage2(eng, fe, xk, out, slope01, scratch) == _lib.SVK_OK
        cache[n, slope01] = out.clone()
    want = cache[n, slope01]
    monkeypatch.delenv(SWITCH, raising=False)
    if static:
        monkeypatch.setenv(STATIC, "1")
    obuf.fill_(float("nan"))
    assert _stage2(eng, fe, xk, out, slope01, None) == _lib.SVK_OK
    assert bool(want.abs().max() > 0)
    assert torch.equal(out, want), "%d of %d elements differ" % (int((out != want).sum()), out.numel())
    assert bool(torch.isnan(obuf[:4]).all()) and bool(torch.isnan(obuf[-4:]).all()), "the kernel wrote outside its output"


@pytest.mark.gpu
@pytest.mark.parametrize("static", (False, True), ids=("queued", "static"))
@pytest.mark.parametrize("slope01", (True, False), ids=("slope01", "any-slope"))
def test_stage2_on_offset_views(eng, fe, stage2_views, stage2_two_kernel_outputs, monkeypatch, slope01, static):
    _stage2_case(eng, fe, stage2_views, stage2_two_kernel_outputs, monkeypatch, 3, slope01, static)


@pytest.mark.gpu
def test_stage2_on_offset_views_several_items_per_workgroup(eng, fe, stage2_views, stage2_two_kernel_outputs, monkeypatch):
    _stage2_case(eng, fe, stage2_views, stage2_two_kernel_outputs, monkeypatch, 75, True, False)


# ---- first block ----------------------------------------------------------------------------------------------------------
def _crop_starts(n_cubes):
    """[n_cubes, 20] int32: ordinary starts in [0, 40] with every special start in every cube, at positions that move from cube to
    cube (a position is a patch depth: another DMA wave, another depth half of the work item)."""
    gen = torch.Generator().manual_seed(77)
    crops = torch.randint(0, 41, (n_cubes, 20), generator=gen, dtype=torch.int32)
    for u in range(n_cubes):
        for a, s in enumerate(SPECIAL_STARTS):
            crops[u, (3 * u + 4 * a) % 20] = s
    return crops


def _cube_of(feat, crops):
    """The cube the kernel reads, [n, 1, 20, 80, 40]: rows crop .. crop + 79 of the clip; a start outside the clip gives a depth of
    zeros, rows past the clip's end are zeros (include/svk.h, svk_c3d2_stage1)."""
    n, frames, _ = feat.shape
    cube = torch.zeros((n, 1, 20, 80, 40), dtype=torch.float32)
    for u in range(n):
        for k in range(20):
            s = int(crops[u, k])
            if 0 <= s < frames:
                rows = min(80, frames - s)
                cube[u, 0, k, :rows] = feat[u, s:s + rows]
    return cube


@pytest.fixture(scope="module")
def stage1_data(eng):
    """{channels: (rows on a view 8 bytes into its allocation, the same rows in a fresh aligned allocation, CPU rows)}: 3 clips."""
    gen = torch.Generator().manual_seed(1209)
    out = {}
    for ch in (1, 3):
        shape = (3, T, 40) if ch == 1 else (3, 3, T, 40)
        rows = torch.randn(shape, generator=gen)
        buf, view = _offset_view(eng, shape, 2, fill=float("nan"))
        view.copy_(rows)
        assert view.data_ptr() % 16 == 8
        fresh = rows.to(eng.device).clone()
        assert fresh.data_ptr() % 256 == 0
        out[ch] = (buf, view, fresh, rows)
    return out


def _stage1(eng, tables, feat, crops, k, slope01):
    tables = list(tables)
    assert len(tables) == 7 and isinstance(tables[6], bool)
    tables[6] = tables[6] and slope01
    crops = crops.to(eng.device)
    if k > 1:
        crops = crops.view(feat.shape[0], k, 20)
    got = eng.c3d2_stage1(feat, crops, tables, cubes_per_clip=k)
    torch.cuda.synchronize()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("slope01", (True, False), ids=("own-slope-flag", "any-slope"))
@pytest.mark.parametrize("k", (1, 2), ids=("one-cube-per-clip", "two-cubes-per-clip"))
@pytest.mark.parametrize("channels", (1, 3), ids=("one-channel", "three-channels"))
def test_stage1_on_offset_features(eng, fe, fe3, stage1_data, channels, k, slope01):
    _, view, fresh, _ = stage1_data[channels]
    tables = (fe if channels == 1 else fe3).stage1_tables()
    crops = _crop_starts(3 * k)
    got = _stage1(eng, tables, view, crops, k, slope01)
    want = _stage1(eng, tables, fresh, crops, k, slope01)
    assert tuple(got.shape) == (3 * k, 16, 36, 18, 16)
    assert bool(torch.isfinite(want).all()) and bool(want.abs().max() > 0)
    assert torch.equal(got, want), "%d of %d elements differ" % (int((got != want).sum()), got.numel())


@pytest.mark.gpu
def test_stage1_on_offset_features_against_float64(eng, fe, stage1_data):
    """The one-channel output on the offset view within reference (A)'s element bound (c3d2_f64_ref.ref_a / check_a at its own
    lam, as tests/test_c3d2_float64.py::test_kernels_against_float64_on_trained_activations applies it to stage1)."""
    _, view, _, rows = stage1_data[1]
    crops = _crop_starts(3)
    got = R.from_kernel("stage1", _stage1(eng, fe.stage1_tables(), view, crops, 1, True)).cpu()
    ya, bound = R.ref_a("stage1", fe, _cube_of(rows, crops))
    ra, worst = R.check_a(got, ya, bound)
    print("stage1 on the offset view, (A): %.3f of the bound" % ra)
    assert ra <= 1.0, (ra, worst)
