"""svk_embedding_project (csrc/backend.hip) on every tile-count instance with both load widths, at the out_dims where the
instance changes (16|17, 32|33, 64|65, 128|129, 256|257) and at out_dim == dim == 512, where every tile of the 32-tile instance
is live.  70 rows: two workgroups, the second with 6 rows.  Inputs, reference and bounds are test_embedding_project.py's
(tests/backend_f64_ref.py): flags 0 and 1 within (dim + 8) 2^-24 sum_k (|x'_k| + |mu_k|) |W_kj| of float64, flags 2 and 3 the
float32 of the same call's un-normalised rows divided by their float64 norm, or its neighbour.

THREE LAYOUTS must give the same bytes: everything 16-byte aligned (16-byte loads), d_emb 4 bytes off, and ONLY d_mean 4 bytes
off -- each of the two selects the 4-byte-load instance on its own.  Zero padding to the next multiple of 4 (x and mu by
columns, W by rows and, where out_dim == dim, by columns) keeps ceil(dim / 16) and the tile count, so the first out_dim columns
keep every bit: the padded operands are zeros, and the unpadded run has 4-byte loads where the padded one has 16-byte loads."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backend_f64_ref import assert_f32_or_neighbour, l2_f32, project_ref, rows, same_bytes, unit_rows       # noqa: E402

N = 70
# (dim, out_dim, the tile-count instance NT it selects)
SHAPES = [(16, 16, 1), (20, 17, 2), (32, 32, 2), (36, 33, 4), (64, 64, 4), (68, 65, 8), (128, 128, 8), (132, 129, 16),
          (256, 256, 16), (260, 257, 32), (512, 512, 32)]
PAD_SHAPES = [(130, 130), (131, 40), (17, 17), (1, 1)]
LAYOUTS = ("aligned", "d_emb 4 bytes off", "d_mean 4 bytes off")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def off_by_one_float(eng, a):
    """`a` on the device through a view that starts one float past a 16-byte boundary."""
    t = eng.to_device(a)
    flat = torch.empty((t.numel() + 1,), dtype=torch.float32, device=eng.device)
    flat[1:] = t.reshape(-1)
    view = flat[1:].view(t.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def layouts(eng, x, mu):
    dx, dmu = eng.to_device(x), eng.to_device(mu)
    assert dx.data_ptr() % 16 == 0 and dmu.data_ptr() % 16 == 0
    return {"aligned": (dx, dmu), "d_emb 4 bytes off": (off_by_one_float(eng, x), dmu),
            "d_mean 4 bytes off": (dx, off_by_one_float(eng, mu))}


def project(eng, dx, dmu, dw, flags):
    return eng.embedding_project(dx, mean=dmu, w=dw, l2_in=bool(flags & 1), l2_out=bool(flags & 2)).cpu().numpy()


@pytest.mark.parametrize("dim,out_dim,nt", SHAPES)
def test_every_instance_both_load_widths(eng, dim, out_dim, nt):
    tiles = (out_dim + 15) // 16
    assert tiles <= nt and (nt == 1 or tiles > nt // 2), "the shape does not select the %d-tile instance" % nt
    x = rows(N, dim, N)
    mu = x.mean(0).astype(np.float32)
    w = (np.random.default_rng(100 + dim + out_dim).standard_normal((dim, out_dim)) / np.sqrt(dim)).astype(np.float32)
    dw = eng.to_device(w)
    lay = layouts(eng, x, mu)
    worst = 0.0
    for flags in (0, 1):
        got = project(eng, *lay["aligned"], dw, flags)
        assert got.shape == (N, out_dim) and got.dtype == np.float32
        ref, bound = project_ref(x, mu, w, flags)
        err = np.abs(got.astype(np.float64) - ref)
        worst = max(worst, float((err / bound).max()))
        print("dim %d -> %d (NT %d) flags %d: worst error / bound = %.4f" % (dim, out_dim, nt, flags, float((err / bound).max())))
        assert (err <= bound).all(), "flags %d: %d outside the bound" % (flags, int((err > bound).sum()))
        unit = project(eng, *lay["aligned"], dw, flags | 2)
        assert_f32_or_neighbour(unit, unit_rows(got), "dim %d -> %d flags %d" % (dim, out_dim, flags | 2))
        for name in LAYOUTS[1:]:
            same_bytes(project(eng, *lay[name], dw, flags), got, "dim %d -> %d flags %d, %s" % (dim, out_dim, flags, name))
            same_bytes(project(eng, *lay[name], dw, flags | 2), unit, "dim %d -> %d flags %d, %s" % (dim, out_dim, flags | 2, name))
    print("dim %d -> %d (NT %d): worst error / bound = %.4f" % (dim, out_dim, nt, worst))


@pytest.mark.parametrize("dim,out_dim", PAD_SHAPES)
def test_zero_padding_changes_no_bit(eng, dim, out_dim):
    dim_p = 4 * ((dim + 3) // 4)
    out_p = dim_p if out_dim == dim else out_dim
    assert (dim + 15) // 16 == (dim_p + 15) // 16 and (out_dim + 15) // 16 == (out_p + 15) // 16
    x = rows(N, dim, N + 1)
    mu = x.mean(0).astype(np.float32)
    w = (np.random.default_rng(200 + dim + out_dim).standard_normal((dim, out_dim)) / np.sqrt(dim)).astype(np.float32)
    xp, mup, wp = np.zeros((N, dim_p), np.float32), np.zeros(dim_p, np.float32), np.zeros((dim_p, out_p), np.float32)
    xp[:, :dim], mup[:dim], wp[:dim, :out_dim] = x, mu, w
    for flags in range(4):
        got = project(eng, eng.to_device(x), eng.to_device(mu), eng.to_device(w), flags)
        pad = project(eng, eng.to_device(xp), eng.to_device(mup), eng.to_device(wp), flags)
        assert got.shape == (N, out_dim) and pad.shape == (N, out_p)
        same_bytes(pad[:, :out_dim], got, "(%d, %d) padded to (%d, %d), flags %d" % (dim, out_dim, dim_p, out_p, flags))
        assert not pad[:, out_dim:].any(), "a padded output column is not zero"


@pytest.mark.parametrize("dim", (1, 128, 130, 512))
def test_identity_on_the_three_layouts(eng, dim):
    """NULL W: float32(x' - mu) exactly, l2_out by the neighbour rule; dim 130 has 4-byte loads on every layout."""
    x = rows(N, dim, N + 2)
    x[11] = 0.0
    mu = x.mean(0).astype(np.float32)
    lay = layouts(eng, x, mu)
    for flags in (0, 1):
        want = (l2_f32(x) if flags & 1 else x) - mu
        got = project(eng, *lay["aligned"], None, flags)
        same_bytes(got, want, "identity dim %d flags %d" % (dim, flags))
        unit = project(eng, *lay["aligned"], None, flags | 2)
        assert_f32_or_neighbour(unit, unit_rows(got), "identity dim %d flags %d" % (dim, flags | 2))
        for name in LAYOUTS[1:]:
            same_bytes(project(eng, *lay[name], None, flags), got, "identity dim %d flags %d, %s" % (dim, flags, name))
            same_bytes(project(eng, *lay[name], None, flags | 2), unit, "identity dim %d flags %d, %s" % (dim, flags | 2, name))
