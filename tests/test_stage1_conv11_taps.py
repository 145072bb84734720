"""conv1_1's taps inside the first block, one at a time: stage1 (svk_c3d2_stage1 and svk_c3d2_stage1_c3) on IMPULSE cubes --
zero everywhere but one feature -- against the float64 layers.  An impulse at cube (depth d, row r, column w) reaches conv1_1's
outputs (d - kd, r, w - kw) through tap (kd, kw) alone, so each of the 15 taps, its patch word and its weight are checked by
position: a wrong tap, column parity or (h, l) half in conv1_1's K order shows up at the outputs of that impulse.  The positions
cover both column parities, every tap (interior impulses reach all 15), both depth halves of a work item (q = 0: cube depths
0 - 11, q = 1: 8 - 19), the patch's first and last rows, the cube's edges, and for three channels every input channel."""
import copy
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_host_logic)

GOLDEN_3C = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3d2_3c.npz")

# (depth, row, column) of the impulse of each cube: interior columns of both parities (every tap of both parities), the
# depths of q = 0 only (0, 5), both halves (8 - 11) and q = 1 only (12, 19), rows 0 and 79 (the patch's first and last)
POSITIONS = [(0, 0, 0), (0, 79, 39), (5, 40, 20), (5, 41, 21), (8, 0, 17), (9, 79, 18), (10, 13, 2), (11, 66, 3),
             (12, 0, 36), (12, 79, 37), (15, 7, 10), (15, 8, 11), (19, 0, 1), (19, 79, 38), (3, 33, 4), (17, 50, 35)]
# f16(1.7) + 0.45 ulp: l = x - f16(x) is 2.6e-4 of h, so a dropped l-half product moves an output past the 1e-4 rtol
VALUE = 1.7001953125 + 0.45 * 2.0 ** -10


def _impulses(n_channels, channels):
    x = torch.zeros((len(POSITIONS) * len(channels), n_channels, 20, 80, 40), dtype=torch.float32)
    where = []
    for a, ch in enumerate(channels):
        for b, (d, r, w) in enumerate(POSITIONS):
            u = a * len(POSITIONS) + b
            x[u, ch, d, r, w] = VALUE if (u & 1) else -VALUE
            where.append((ch, d, r, w))
    return x, where


def _check(got, want, where, what):
    """got, want: NCDHW; the stage1 bar of the three-channel kernel's f32 test (rtol 1e-4, atol 4e-6 of the scale), per cube."""
    scale = float(want.abs().max())
    err = (got.double() - want).abs() - 1e-4 * want.abs()
    bad = []
    for u, pos in enumerate(where):
        e = float(err[u].max())
        if not e <= 4e-6 * scale:
            c, d, h, w = np.unravel_index(int(torch.argmax(err[u])), tuple(err[u].shape))
            bad.append("impulse (ch, d, r, w) = %s: %.2e of the scale at output (c, d, h, w) = (%d, %d, %d, %d)"
                       % (pos, e / scale, c, d, h, w))
    print("%s: max |err| / scale %.2e over %d impulses" % (what, float(err.max()) / scale, len(where)))
    assert not bad, bad


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.mark.gpu
def test_one_channel_impulses(eng):
    """svk_c3d2_stage1 with the trained checkpoint: (A) element by element (the kernel's own arithmetic in float64 within its
    bound) and the float64 layers with unfolded BatchNorm at the stage1 bar, impulse by impulse."""
    fe = copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()
    state = R.state_of(R.trained_model())
    x, where = _impulses(1, [0])
    xk = R.to_kernel("stage1", x).to(eng.device)
    got = R.from_kernel("stage1", R.run_kernel(eng, fe, "stage1", xk)).cpu()
    ya, bound = R.ref_a("stage1", fe, x)
    ra, worst = R.check_a(got, ya, bound)
    print("one channel, (A): %.3f of the bound" % ra)
    assert ra <= 1.0, (ra, np.unravel_index(worst, tuple(got.shape)))
    _check(got, R.ref_b("stage1", state, x), where, "one channel vs float64")


@pytest.mark.gpu
def test_three_channel_impulses(eng):
    """svk_c3d2_stage1_c3 with the golden three-channel model, an impulse in each input channel in turn (channel 0 comes
    through the patch buffer, channels 1 and 2 through the act1 tile): (A) element by element -- tight enough to see a lost or
    misplaced l-half product, which the float64 bar's rtol alone may not -- and the float64 layers at the stage1 bar."""
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    g = np.load(GOLDEN_3C, allow_pickle=False)
    model = seeded_model(int(g["init_seed"][0]), int(g["n_labels"][0]), 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), int(g["perturb_seed"][0])))
    model = model.eval()
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    fe = model.to(eng.device).fused_inference()
    x, where = _impulses(3, [0, 1, 2])
    n = x.shape[0]
    rows = x.reshape(n, 3, 1600, 40).to(eng.device)
    got = eng.c3d2_stage1(rows, fe.crop_starts(n, eng.device), fe.stage1_tables()).cpu().permute(0, 4, 1, 2, 3)
    ya, bound = R.ref_a("stage1", fe, x)
    ra, worst = R.check_a(got, ya, bound)
    print("three channels, (A): %.3f of the bound" % ra)
    assert ra <= 1.0, (ra, where[np.unravel_index(worst, tuple(got.shape))[0]])
    _check(got, R.ref_b("stage1", state, x), where, "three channels vs float64")
