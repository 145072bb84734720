"""The C3D2 network kernels on launches whose input, output or scratch exceeds 2^31 elements (8.6 GB of f32): the sizes
bench.py's launch sequences reach (up to 74 321 cubes).  One kernel at a time, device-random input in its own layout;
64-cube windows -- the first, the one straddling 2^31 elements of the crossing tensor, the one straddling 2^32 bytes, the last
(partial) -- must be bit-identical to the same window launched alone, and the window's first and last rows must match
reference (B) (tests/c3d2_f64_ref.py) within 4e-6 of the scale, the per-layer bar of tests/test_gpu_parity.py: on two
rows of N(0, 1) data torch-CPU f32's own error is too small a sample for the trained-activation bars (measured: conv3_2,
conv4_1 and conv4_2 at 1.7 - 3.3 x those bars on such rows, 0.9 - 1.9e-6 of the scale).  Then one embed_features of 13 000 cubes against 4 096-cube batches, bit for bit."""
import copy

import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu

# kernel, crossing tensor, n, input shape per cube, (floats per cube of the crossing tensor)
CASES = [
    ("stage1", "feature rows", 4000, (13500, 40), 540000),
    ("stage1", "output", 13000, (100, 40), 165888),
    ("stage2", "scratch", 13000, (16, 36, 18, 16), 225792),
    ("conv31", "output", 45000, (12, 15, 7, 32), 48000),
    ("conv32t", "input", 45000, (10, 8, 5, 15, 8), 48000),
    ("conv41", "input and output", 104005, (8, 8, 45, 8), 23040),
    ("conv42", "input", 104005, (6, 16, 27, 8), 20736),
    ("fc5", "input", 467037, (4, 16, 9, 8), 4608),
]
OUT_FLOATS = {"stage1": 165888, "stage2": 20160, "conv31": 48000, "conv32t": 23040, "conv41": 20736, "conv42": 4608, "fc5": 128}


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def gpu_fe(eng):
    model = copy.deepcopy(R.trained_model()).to(eng.device).eval()
    return model.fused_inference()


def _room(eng, need):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(eng.device)
    if free < need * 1.15:
        pytest.skip("needs %.1f GB free, %.1f of %.1f GB are" % (need / 1e9, free / 1e9, total / 1e9))


def _windows(n, per_cube):
    """64-aligned window starts: the first, the one holding element 2^31 and the one holding byte 2^32 of the crossing tensor,
    the last (partial)."""
    starts = [0, (2 ** 31 // per_cube) // 64 * 64, (2 ** 30 // per_cube) // 64 * 64, (n - 1) // 64 * 64]
    assert n % 64 and 2 ** 31 // per_cube < n
    return sorted(set(starts))


@pytest.mark.parametrize("kernel,crossing,n,shape,per_cube", CASES, ids=["%s-%s" % (c[0], c[1].replace(" ", "-")) for c in CASES])
def test_launch_past_2_31_elements(eng, gpu_fe, kernel, crossing, n, shape, per_cube):
    assert n * per_cube > 2 ** 31
    scratch = n * 225792 if kernel == "stage2" else (n * 4608 if kernel == "fc5" else 0)
    _room(eng, 4 * (n * (int(torch.tensor(shape).prod()) + OUT_FLOATS[kernel]) + scratch))
    state = R.state_of(R.trained_model())
    g = torch.Generator(device=eng.device)
    g.manual_seed(2 ** 31 % 97)
    x = torch.randn((n,) + shape, device=eng.device, generator=g)
    if kernel == "stage1":
        crops = torch.randint(0, shape[0] - 80, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
        big = eng.c3d2_stage1(x, crops, gpu_fe.stage1_tables())
    else:
        big = R.run_kernel(eng, gpu_fe, kernel, x)
    torch.cuda.synchronize()
    for s in _windows(n, per_cube):
        e = min(n, s + 64)
        if kernel == "stage1":
            alone = eng.c3d2_stage1(x[s:e], crops[s:e], gpu_fe.stage1_tables())
        else:
            alone = R.run_kernel(eng, gpu_fe, kernel, x[s:e].contiguous())
        assert torch.equal(big[s:e], alone), "%s, %d cubes: rows %d - %d differ from the same window launched alone" % (kernel, n, s, e)
        rows = [s, e - 1]
        got = R.from_kernel(kernel, big[rows].cpu())
        if kernel == "stage1":     # the cubes the crop starts select, NCDHW
            fx = x[rows].cpu()
            cr = crops[rows].cpu().long()
            xin = torch.stack([fx[i][cr[i][:, None] + torch.arange(80)[None]] for i in range(2)])[:, None]
        else:
            xin = R.from_input(kernel, x[rows].cpu())
        yb = R.ref_b(kernel, state, xin)
        eb = R.errors_b(got, yb)
        print("%s, %d cubes (%s past 2^31), rows %d / %d: (B) max %.2e rms %.2e of the scale"
              % (kernel, n, crossing, s, e - 1, eb[0], eb[1]))
        assert eb[0] <= 4e-6, (kernel, s, eb)
    del big, x


def test_embed_features_13000_cubes_in_one_sequence(eng, gpu_fe):
    """One embed_features of 13 000 cubes (stage-1 output 8.6 GB, conv2_1 scratch 11.7 GB behind one pointer) against the same
    cubes in 4 096-cube batches: bit for bit."""
    n, T = 13000, 200
    _room(eng, 4 * n * (T * 40 + 165888 + 225792 + 20160 + 48000 * 2))
    g = torch.Generator(device=eng.device)
    g.manual_seed(5)
    feat = torch.randn((n, T, 40), device=eng.device, generator=g)
    crops = torch.randint(0, T - 80, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
    one = gpu_fe.embed_features(feat, crops)
    torch.cuda.synchronize()
    for lo in range(0, n, 4096):
        hi = min(n, lo + 4096)
        assert torch.equal(one[lo:hi], gpu_fe.embed_features(feat[lo:hi], crops[lo:hi])), (lo, hi)
