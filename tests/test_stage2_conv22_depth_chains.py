"""conv2_2's depth chains inside the second block: svk_c3d2_stage2 on inputs [16][36][18][16] that are zero except ONE depth,
against the float64 layers.  An input depth d reaches conv2_1's output depths d - 2 .. d, and each of those reaches a conv2_2
output depth through exactly one kd: a chain step that multiplies an input depth's fragments into the wrong one of its three
accumulators, or with another kd's taps, is wrong by position.  Depths 0 .. 15 cover the first and last output depth of every
chain and all three depth thirds of the work items.  Every value is random, so the two columns of output row 14 (the last
two positions of a plane, lanes 12 and 13 of the second plane tile) differ from each other and from every other row: the two
clamped lanes behind them (both at row 14, column 1) would pool to another maximum if one of them stored.  Work items drawn from
the device-wide counter or at a fixed stride give the same bits."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_host_logic)

TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def case(eng):
    """The 18 inputs (NCDHW, true units: depths 0 .. 15, two random ones), what the kernel reads and its output: made once."""
    fe = copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()
    gen = torch.Generator().manual_seed(22)
    x = torch.zeros((18, 16, 16, 36, 18), dtype=torch.float32)
    for d in range(16):
        x[d, :, d] = torch.randn((16, 36, 18), generator=gen)
    x[16:] = torch.randn((2, 16, 16, 36, 18), generator=gen)
    names = ["input depth %d" % d for d in range(16)] + ["random input 0", "random input 1"]
    xc = R.to_carried(fe, "stage2", x)
    xk = R.to_kernel("stage2", xc).to(eng.device)
    out = R.run_kernel(eng, fe, "stage2", xk)
    return fe, x, xc, xk, out, names


@pytest.mark.gpu
def test_one_depth_inputs(eng, case):
    """(A) element by element within its bound, and (B): max and RMS error / scale within the stage2 bar (c3d2_f64_ref.FACTOR
    x torch-CPU f32's + 2^-24), input by input and over all of them."""
    fe, x, xc, _, out, names = case
    got = R.from_kernel("stage2", out).cpu()
    assert tuple(got.shape) == (18, 32, 12, 15, 7)
    ya, bound = R.ref_a("stage2", fe, xc)
    ra, worst = R.check_a(got, ya, bound)
    print("stage2, (A): %.3f of the bound" % ra)
    where = np.unravel_index(worst, tuple(got.shape))
    assert ra <= 1.0, (ra, names[where[0]], where[1:])
    state = R.state_of(R.trained_model())
    yb = R.ref_b("stage2", state, x)
    y32 = R.ref_b_f32("stage2", state, x)
    true = R.to_true(fe, "stage2", got)
    bad = []
    for u, name in [(slice(None), "all inputs")] + [(slice(u, u + 1), n) for u, n in enumerate(names)]:
        eb, bar = R.errors_b(true[u], yb[u]), R.bar_b("stage2", R.errors_b(y32[u], yb[u]))
        if not (eb[0] <= bar[0] and eb[1] <= bar[1]):
            bad.append("%s: (max, rms) %s over %s" % (name, eb, bar))
        if name == "all inputs":
            print("stage2, (B): max %.2e rms %.2e of the scale; bars %.2e %.2e" % (eb + bar))
    assert not bad, bad


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
np.save(sys.argv[2], R.run_kernel(eng, fe, "stage2", xk).cpu().numpy())
'''


@pytest.mark.gpu
def test_bits_repeat_and_do_not_depend_on_item_order(eng, case, tmp_path):
    """The same input twice, and once in a fresh process that takes its work items at a fixed stride (SVK_C3D2_STATIC_ITEMS=1)
    instead of from the device-wide counter: all three outputs bit-equal."""
    fe, _, _, xk, out, _ = case
    assert torch.equal(out, R.run_kernel(eng, fe, "stage2", xk))
    src, dst = str(tmp_path / "in.npy"), str(tmp_path / "out.npy")
    np.save(src, xk.cpu().numpy())
    env = dict(os.environ, SVK_C3D2_STATIC_ITEMS="1")
    proc = subprocess.run([sys.executable, "-c", _CHILD % (R.REPO, TESTS), src, dst], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=300)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    assert np.array_equal(np.load(dst).view(np.uint32), out.cpu().numpy().view(np.uint32))
