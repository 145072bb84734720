"""conv1_2's depth chains inside the first block: stage1 (svk_c3d2_stage1 and svk_c3d2_stage1_c3) on cubes that are zero except
ONE cube depth, against the float64 layers.  A cube depth d reaches act1 (conv1_1's output) depths d - 2 .. d, and an act1 depth
reaches a conv1_2 output depth through exactly one kd: where a chain step multiplies an input depth's fragments into the wrong one
of its three accumulators, or with another kd's weights, the outputs of that cube are wrong by position.  Depths 0 .. 19 cover
the first and last output depth of every chain, both depth halves q of a work item, and (every row is filled) the stand-alone
tiles of rows 32 - 35.  The values are f16-exact h plus 0.45 ulp, so l is about 2.6e-4 of h and a dropped or misrouted l piece
breaks reference (A).  Work items drawn from the device-wide counter or at a fixed stride give the same bits."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_host_logic)

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN_3C = os.path.join(TESTS, "golden", "c3d2_3c.npz")


def _values(gen, shape):
    """Seeded values in the features' range (|x| in [0.5, 4)): h = an f16 value, x = h + 0.45 ulp_f16(h) away from zero:
    l = x - f16(x) is 2.2 - 4.4e-4 of h."""
    mag = (0.5 + 3.5 * torch.rand(shape, generator=gen)).half().float()
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 10)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    return sign * (mag + 0.45 * ulp)


def _one_depth_cubes(n_channels, depths, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.zeros((len(depths), n_channels, 20, 80, 40), dtype=torch.float32)
    for u, d in enumerate(depths):
        x[u, :, d] = _values(gen, (n_channels, 80, 40))
    return x, gen


def _check_b(got, want, names, what):
    """got, want: NCDHW in true units; the stage1 bar of tests/test_stage1_conv11_taps.py (rtol 1e-4, atol 4e-6 of the scale), per cube."""
    scale = float(want.abs().max())
    err = (got.double() - want).abs() - 1e-4 * want.abs()
    bad = []
    for u, name in enumerate(names):
        e = float(err[u].max())
        if not e <= 4e-6 * scale:
            c, d, h, w = np.unravel_index(int(torch.argmax(err[u])), tuple(err[u].shape))
            bad.append("%s: %.2e of the scale at output (c, d, h, w) = (%d, %d, %d, %d)" % (name, e / scale, c, d, h, w))
    print("%s: max |err| / scale %.2e over %d cubes" % (what, float(err.max()) / scale, len(names)))
    assert not bad, bad


def _check_a(got, ya, bound, names, what):
    ra, worst = R.check_a(got, ya, bound)
    print("%s, (A): %.3f of the bound" % (what, ra))
    where = np.unravel_index(worst, tuple(got.shape))
    assert ra <= 1.0, (ra, names[where[0]], where[1:])


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def one_channel(eng):
    """The 22 cubes (depths 0 .. 19, two random ones), the kernel's output on them and the trained model's tables: made once."""
    fe = copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()
    x, gen = _one_depth_cubes(1, list(range(20)), 12)
    x = torch.cat([x, 2.0 * torch.randn((2, 1, 20, 80, 40), generator=gen)])
    names = ["cube depth %d" % d for d in range(20)] + ["random cube 0", "random cube 1"]
    xk = R.to_kernel("stage1", x).to(eng.device)
    out = R.run_kernel(eng, fe, "stage1", xk)
    return fe, x, xk, out, names


@pytest.mark.gpu
def test_one_channel_one_depth_cubes(eng, one_channel):
    """svk_c3d2_stage1 with the trained checkpoint: (A) element by element and the float64 layers at the stage1 bar, cube by cube."""
    fe, x, _, out, names = one_channel
    got = R.from_kernel("stage1", out).cpu()
    ya, bound = R.ref_a("stage1", fe, x)
    _check_a(got, ya, bound, names, "one channel")
    _check_b(R.to_true(fe, "stage1", got), R.ref_b("stage1", R.state_of(R.trained_model()), x), names, "one channel vs float64")


@pytest.mark.gpu
def test_three_channel_one_depth_cubes(eng):
    """svk_c3d2_stage1_c3 with the golden three-channel model on cube depths 0, 9 and 19 (all three input channels filled): the
    same two checks."""
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    g = np.load(GOLDEN_3C, allow_pickle=False)
    model = seeded_model(int(g["init_seed"][0]), int(g["n_labels"][0]), 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), int(g["perturb_seed"][0])))
    model = model.eval()
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    fe = model.to(eng.device).fused_inference()
    depths = [0, 9, 19]
    x, _ = _one_depth_cubes(3, depths, 13)
    names = ["cube depth %d" % d for d in depths]
    rows = x.reshape(len(depths), 3, 1600, 40).to(eng.device)
    crops = fe.crop_starts(len(depths), eng.device)
    out = eng.c3d2_stage1(rows, crops, fe.stage1_tables())
    assert torch.equal(out, eng.c3d2_stage1(rows, crops, fe.stage1_tables()))
    got = out.cpu().permute(0, 4, 1, 2, 3)
    ya, bound = R.ref_a("stage1", fe, x)
    _check_a(got, ya, bound, names, "three channels")
    _check_b(R.to_true(fe, "stage1", got), R.ref_b("stage1", state, x), names, "three channels vs float64")


_CHILD = r'''
import copy, sys
import numpy as np
import torch
sys.path[:0] = [%r, %r]
import c3d2_f64_ref as R
from speaker_verification_amd.engine import get_engine
eng = get_engine(0)
fe = copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()
xk = torch.from_numpy(np.load(sys.argv[1])).to(eng.device)
np.save(sys.argv[2], R.run_kernel(eng, fe, "stage1", xk).cpu().numpy())
'''


@pytest.mark.gpu
def test_bits_repeat_and_do_not_depend_on_item_order(eng, one_channel, tmp_path):
    """The same input twice, and once in a fresh process that takes its work items at a fixed stride (SVK_C3D2_STATIC_ITEMS=1)
    instead of from the device-wide counter: all three outputs bit-equal."""
    fe, _, xk, out, _ = one_channel
    assert torch.equal(out, R.run_kernel(eng, fe, "stage1", xk))
    src, dst = str(tmp_path / "in.npy"), str(tmp_path / "out.npy")
    np.save(src, xk.cpu().numpy())
    env = dict(os.environ, SVK_C3D2_STATIC_ITEMS="1")
    proc = subprocess.run([sys.executable, "-c", _CHILD % (R.REPO, TESTS), src, dst], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=300)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    assert np.array_equal(np.load(dst).view(np.uint32), out.cpu().numpy().view(np.uint32))
