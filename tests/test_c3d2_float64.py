"""The seven C3D2 network kernels against float64 (tests/c3d2_f64_ref.py: references (A) and (B), the CPU emulation and its
mutants).

CPU (default pass):
  * the kernels' operand tables hold the BatchNorm-folded weights to f16 rounding of the low piece, tap by tap, channel by
    channel (what makes reference (A), which reads those tables, trustworthy);
  * the CPU emulation of the two-piece arithmetic passes (A) and (B) on the trained checkpoint's activations in every
    accumulation order, and each mutant of it fails: the bars have teeth.
GPU (-m gpu):
  * every kernel on the trained activations against (A) element by element and (B) against torch-CPU f32's error;
  * half-pair domain edges (zeros, -0.0, 2^-3 +- 1 ulp, subnormal h, ties of x - h, |x| near 65 504, 1e4 next to 1e-4);
  * isolation between cubes (NaN / +inf neighbours) and from memory the call did not write (NaN-filled free blocks).
"""
import copy
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_host_logic)


@pytest.fixture(scope="module")
def cpu_fe():
    from speaker_verification_amd.model import FusedEmbedder
    return FusedEmbedder(R.trained_model())


@pytest.fixture(scope="module")
def acts():
    return R.trained_activations()


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_trained_activations_cover_eight_speakers(acts):
    x, y = acts["stage1"]
    assert x.shape == (8, 1, 20, 80, 40) and x.dtype == torch.float32
    assert len({tuple(np.round(c.numpy().ravel()[:64], 4)) for c in x}) == 8
    for k in R.KERNELS:
        assert acts[k][1].dtype == torch.float64 and bool(torch.isfinite(acts[k][1]).all())
    # the embeddings of distinct speakers differ
    e = acts["fc5"][1]
    assert float(torch.cdist(e, e).add(torch.eye(8, dtype=e.dtype) * 1e9).min()) > 1e-3 * float(e.abs().max())


@pytest.mark.parametrize("kernel", R.HALF_PAIR)
def test_tables_hold_the_folded_weights(cpu_fe, kernel):
    """In float64, H + L read back from the kernel's tables equals the BatchNorm-folded f32 weight within f16 rounding of the
    low piece (2^-22 relative, 2^-25 absolute), for every tap and channel of every layer; H is f16(w) exactly; every weight
    appears in the tables, and every pad slot is zero."""
    for j, p in enumerate(R.weight_pieces(kernel, cpu_fe)):
        H, L, w = p["H"], p["L"], p["w"]
        assert p["consistent"] and p["covered"] and p["pads_zero"], (kernel, j)
        assert torch.equal(H, w.float().half().double()), (kernel, j)
        err = (H + L - w).abs() / (2.0 ** -22 * w.abs() + 2.0 ** -25)
        worst = np.unravel_index(int(torch.argmax(err)), tuple(w.shape))
        assert float(err.max()) <= 1.0, "%s layer %d: H + L misses the folded weight at (co, ci, kd, kh, kw) = %s" % (kernel, j, worst)


def test_f32_tail_tables_hold_the_folded_weights(cpu_fe):
    """conv4_2's Winograd table gives back the folded weight (g0 = G0, g2 = G3, g1 = G1 - G2) to f32 rounding, and FC5's
    table is FC5's weight in the chunked K order, bit for bit."""
    w = cpu_fe.stages[7][0].double()
    frag = cpu_fe.conv42_tables()[0].double()                     # [nt][chunk][tap][k][lane][e]
    lane = torch.arange(64)
    g = torch.zeros((4, 128, 128, 7), dtype=torch.float64)         # [k][co][ci][tap]
    for nt in range(8):
        for ch in range(16):
            for e in range(2):
                g[:, 16 * nt + (lane & 15), 8 * ch + 2 * (lane >> 4) + e, :] = frag[nt, ch, :, :, :, e].permute(1, 2, 0)
    g0, g1, g2 = w[:, :, 0, :, 0], w[:, :, 1, :, 0], w[:, :, 2, :, 0]
    scale = g0.abs() + g1.abs() + g2.abs()
    assert torch.equal(g[0], g0) and torch.equal(g[3], g2)
    assert float(((g[1] - g[2] - g1).abs() / scale.clamp(min=1e-30)).max()) <= 2.0 ** -22
    assert float(((g[1] + g[2] - g0 - g2).abs() / scale.clamp(min=1e-30)).max()) <= 2.0 ** -22
    fw, fb = cpu_fe.fc5_tables()
    d, ch, px, c8 = torch.meshgrid(*(torch.arange(n) for n in (4, 16, 9, 8)), indexing="ij")
    col = ((8 * ch + c8) * 36 + d * 9 + px).reshape(-1)
    want = cpu_fe.fc_w[:, col].view(8, 16, 4, 72, 4, 4)               # [nt][n][d][step][kq][e]
    assert torch.equal(fw, want[:, lane & 15, :, :, lane >> 4].permute(2, 1, 3, 0, 4))
    assert torch.equal(fb, cpu_fe.fc_b)


def _refs(kernel, fe, state, x):
    ya, bound = R.ref_a(kernel, fe, x)
    yb = R.ref_b(kernel, state, x)
    return ya, bound, yb, R.bar_b(kernel, R.errors_b(R.ref_b_f32(kernel, state, x), yb))


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_emulation_passes_both_references(cpu_fe, acts, kernel):
    """The two-piece arithmetic with f32 accumulation (pairwise; sequential and reversed over MFMA-sized blocks) passes (A)
    element by element and (B) on the trained activations (a two-output-depth window of every layer).  Calibrates lam:
    the (A) ratio printed is max |emul - ref_A| / bound at lam = R.LAMBDA.  One running sum over single products
    ("sequential1") still passes (A); its (B) number is printed for the record."""
    state = R.state_of(R.trained_model())
    x = R.crop_depth(kernel, acts[kernel][0])
    ya, bound, yb, bar = _refs(kernel, cpu_fe, state, x)
    for order in ("pairwise", "sequential", "reversed", "sequential1"):
        got = R.emulate(kernel, cpu_fe, x, order)
        ra, _ = R.check_a(got, ya, bound)
        eb = R.errors_b(got, yb)
        print("%s %-11s (A) %.3f of the bound  (B) max %.2e rms %.2e of the scale, bars %.2e %.2e"
              % (kernel, order, ra, eb[0], eb[1], bar[0], bar[1]))
        assert ra <= 0.5, (kernel, order, ra)        # lam could be halved and this order would still pass
        if order != "sequential1":
            assert eb[0] <= bar[0] and eb[1] <= bar[1], (kernel, order, eb, bar)


@pytest.mark.parametrize("kernel", R.HALF_PAIR)
def test_mutants_fail_the_bars(cpu_fe, acts, kernel, request):
    """Each mutant of the emulation, on this layer: printed with its ratio to the (B) bars and to the (A) bound.  That every
    mutant fails somewhere is asserted in test_every_mutant_fails_somewhere, over all layers."""
    state = R.state_of(R.trained_model())
    x = R.crop_depth(kernel, acts[kernel][0])
    ya, bound, yb, bar = _refs(kernel, cpu_fe, state, x)
    res = {}
    for mu in R.MUTANTS:
        got = R.emulate(kernel, cpu_fe, x, "sequential", mu)
        ra, _ = R.check_a(got, ya, bound)
        eb = R.errors_b(got, yb)
        res[mu] = (ra, max(eb[0] / bar[0], eb[1] / bar[1]))
        print("%s mutant %-22s (A) %7.2f x the bound   (B) %7.1f x the bar" % (kernel, mu, res[mu][0], res[mu][1]))
    _MUTANT_RESULTS[kernel] = res


_MUTANT_RESULTS = {}


def test_every_mutant_fails_somewhere(cpu_fe, acts):
    """Each mutant fails the (B) bar by >= 4 x on at least one layer, and the first two and the last fail (A) too.  The
    rounding-direction mutant (l toward zero instead of to nearest) changes a product by at most one ulp of l, 2^-22 of it:
    the size of f32 rounding, so no tolerance on O(1) activations can see it (it stays under the (B) bar).  It is caught where
    l is a subnormal half: on the trained input scaled by 2^-14 (values in [2^-24, 2^-12): the domain edge of
    test_half_pair_domain_edges) it fails (A) on conv4_1 (2.8 x the bound; the folded biases swamp it on the others)."""
    for k in R.HALF_PAIR:
        if k not in _MUTANT_RESULTS:
            test_mutants_fail_the_bars(cpu_fe, acts, k, None)
    for mu in R.MUTANTS:
        worst_b = max(_MUTANT_RESULTS[k][mu][1] for k in R.HALF_PAIR)
        worst_a = max(_MUTANT_RESULTS[k][mu][0] for k in R.HALF_PAIR)
        print("mutant %-22s worst (B) %.1f x the bar, worst (A) %.2f x the bound" % (mu, worst_b, worst_a))
        if mu != "l_toward_zero":
            assert worst_b >= 4.0, mu
        if mu in ("drop_lx_H", "drop_hx_L", "no_low_at_border_tap"):
            assert worst_a > 1.0, mu
    caught = {}
    for k in ("stage1", "conv31", "conv41"):
        x = R.crop_depth(k, acts[k][0]) * 2.0 ** -14
        ya, bound = R.ref_a(k, cpu_fe, x)
        assert R.check_a(R.emulate(k, cpu_fe, x, "sequential"), ya, bound)[0] <= 1.0
        caught[k] = R.check_a(R.emulate(k, cpu_fe, x, "sequential", "l_toward_zero"), ya, bound)[0]
        print("%s: l toward zero on the input x 2^-14: (A) %.2f x the bound" % (k, caught[k]))
    assert max(caught.values()) > 1.0, caught


def test_domain_edge_inputs_are_what_they_say():
    x = _edge_values(torch.Generator().manual_seed(1), (4096,), stage1=False)
    h = x.half()
    lo = x - h.float()
    assert bool((x == 0).any()) and bool((torch.signbit(x) & (x == 0)).any())
    assert bool(((x.abs() >= 2.0 ** -24) & (x.abs() < 2.0 ** -14)).any())
    assert bool(((x.abs() > 0) & (x.abs() < 2.0 ** -25)).any())
    assert bool((x.abs() >= 6.0e4).any()) and float(x.abs().max()) < 65504.0
    # x - h on an f16 tie: half-way between two adjacent halves
    lo16 = lo.half().float()
    other = torch.where(lo16 > lo, torch.from_numpy(np.nextafter(lo16.numpy().astype(np.float16), np.float16(-1)).astype(np.float32)),
                        torch.from_numpy(np.nextafter(lo16.numpy().astype(np.float16), np.float16(1)).astype(np.float32)))
    assert bool((((lo16 - lo).abs() == (other - lo).abs()) & (lo != lo16)).any())


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def gpu_fe(eng):
    model = copy.deepcopy(R.trained_model()).to(eng.device).eval()
    return model.fused_inference()


def _gpu(eng, fe, kernel, x):
    """`kernel` on NCDHW x (the units it reads) -> its output as NCDHW on the CPU."""
    return R.from_kernel(kernel, R.run_kernel(eng, fe, kernel, R.to_kernel(kernel, x).to(eng.device))).cpu()


@pytest.mark.gpu
def test_kernels_against_float64_on_trained_activations(eng, gpu_fe, acts):
    """Every kernel on the trained checkpoint's activations (8 speakers): (A) element by element within its bound, and (B):
    max and RMS error / scale within FACTOR x torch-CPU f32's + 2^-24 (c3d2_f64_ref.FACTOR).  All layers are measured and
    printed before any assertion."""
    state = R.state_of(R.trained_model())
    rows, fails = [], []
    for k in R.KERNELS:
        x, _ = acts[k]
        xk = R.to_carried(gpu_fe, k, x)
        got = _gpu(eng, gpu_fe, k, xk)
        ya, bound = R.ref_a(k, gpu_fe, xk)
        ra, worst = R.check_a(got, ya, bound)
        yb = R.ref_b(k, state, x)
        yard = R.errors_b(R.ref_b_f32(k, state, x), yb)
        eb = R.errors_b(R.to_true(gpu_fe, k, got), yb)
        bar = R.bar_b(k, yard)
        rows.append((k, ra, eb, yard))
        print("GPU %-7s (A) %.3f of the bound   (B) max %.2e rms %.2e of the scale; torch-CPU f32 %.2e %.2e; ratios %.2f %.2f"
              % (k, ra, eb[0], eb[1], yard[0], yard[1], eb[0] / yard[0], eb[1] / yard[1]))
        if not ra <= 1.0:
            fails.append("%s (A): %.3f x the bound at flat index %d" % (k, ra, worst))
        if not (eb[0] <= bar[0] and eb[1] <= bar[1]):
            fails.append("%s (B): %s over %s" % (k, eb, bar))
    assert not fails, fails


def _edge_values(gen, shape, stage1):
    """Values that probe the half pairs, mixed at random within every dot product (see the module docstring)."""
    n = int(np.prod(shape))
    ulp = lambda v: np.float32(np.spacing(np.float32(v)))       # noqa: E731
    pool = [0.0, -0.0, 0.125, 0.125 + ulp(0.125), 0.125 - ulp(0.125) / 2, -0.125 - ulp(0.125),
            3.0e-6, -1.1e-5, 6.2e-8, 4.0e-7, -2.0e-8, 1.0e-8, 1.0e-4, -1.0e-4,
            # x - h half-way between two halves: 2^-12 + 2^-23 (ulp 2^-22), 2^-11 + 2^-22, 2^-13 + 2^-24
            1.0 + 2.0 ** -12 + 2.0 ** -23, -(2.0 + 2.0 ** -11 + 2.0 ** -22), 0.75 + 2.0 ** -13 + 2.0 ** -24]
    pool += [1.0e3, -1.0e3, 7.5] if stage1 else [6.0e4, -6.2e4, 65000.0, 1.0e4, -1.0e4]
    pool = torch.tensor(pool, dtype=torch.float32)
    pick = torch.randint(0, len(pool), (n,), generator=gen)
    x = pool[pick] * torch.where(torch.rand((n,), generator=gen) < 0.5, 1.0, -1.0)
    x = torch.where(torch.rand((n,), generator=gen) < 0.3, torch.randn((n,), generator=gen), x)   # ordinary values among them
    return x.view(shape).float()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["stage1", "conv31", "conv32t", "conv41"])
def test_half_pair_domain_edges(eng, gpu_fe, acts, kernel):
    """Crafted inputs (zeros, -0.0, a whole zero channel, 2^-3 +- 1 ulp, subnormal h, values below 2^-25, ties of x - h,
    |x| up to 65 000, 1e4 next to 1e-4) against (A): its element bound is the only tolerance (lam = 8, the largest allowed:
    crafted sums are not random walks).  stage1's values stay small enough that conv1_1's output, split again inside the
    kernel, stays below 65 504."""
    gen = torch.Generator().manual_seed(7)
    shape = tuple(acts[kernel][0].shape)
    x = _edge_values(gen, (6,) + shape[1:], stage1=(kernel == "stage1"))
    if kernel != "stage1":
        x[:, 3] = 0.0                                   # a whole channel of zeros
        x[:, 5] = -0.0
    else:
        x[:, :, :, :, 7] = 0.0                          # a whole coefficient column
    got = _gpu(eng, gpu_fe, kernel, x)
    ya, bound = R.ref_a(kernel, gpu_fe, x, lam=8.0)
    if kernel == "stage1":
        assert float(R.ref_a_layer1_max(gpu_fe, x)) < 65504.0
    ra, worst = R.check_a(got, ya, bound)
    print("domain edges, %s: (A) %.3f of the bound; |y| up to %.3g" % (kernel, ra, float(ya.abs().max())))
    assert bool(torch.isfinite(got).all()) and ra <= 1.0, (kernel, ra, worst)


def _poison(x, step, value):
    y = x.clone()
    y[::step] = value
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_cubes_stay_confined(eng, gpu_fe, value):
    """300 cubes (workgroups take several items; partial last groups of 16 and of FC5's 64): every 7th cube's input NaN, then
    +inf.  Each kernel and embed_features: every other cube's output bit-identical to the run with those cubes zero."""
    g = torch.Generator(device=eng.device)
    g.manual_seed(11)
    n = 300
    keep = torch.ones(n, dtype=torch.bool)
    keep[::7] = False
    shapes = {"stage1": (n, 1600, 40), "stage2": (n, 16, 36, 18, 16), "conv31": (n, 12, 15, 7, 32), "conv32t": (n, 10, 8, 5, 15, 8),
              "conv41": (n, 8, 8, 45, 8), "conv42": (n, 6, 16, 27, 8), "fc5": (n, 4, 16, 9, 8)}
    for k, shp in shapes.items():
        x = torch.randn(shp, device=eng.device, generator=g)
        a = R.run_kernel(eng, gpu_fe, k, _poison(x, 7, value))
        b = R.run_kernel(eng, gpu_fe, k, _poison(x, 7, 0.0))
        assert torch.equal(a[keep.to(a.device)], b[keep.to(b.device)]), k
        assert not bool(torch.isfinite(a[~keep.to(a.device)]).all()), k      # the poison did reach its own cubes
    feat = torch.randn((n, 300, 40), device=eng.device, generator=g)
    crops = torch.randint(0, 220, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
    a = gpu_fe.embed_features(_poison(feat, 7, value), crops)
    b = gpu_fe.embed_features(_poison(feat, 7, 0.0), crops)
    assert torch.equal(a[keep.to(a.device)], b[keep.to(b.device)])


def _nan_filled_free_blocks(eng, floats):
    """Allocate one block of each size in `floats` through torch, fill them with NaN, free them: the caching allocator hands
    these bytes to the next allocations of those sizes (best fit).  -> their (lo, hi) address ranges."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    blks = [torch.full((int(f),), float("nan"), dtype=torch.float32, device=eng.device) for f in floats]
    ranges = [(b.data_ptr(), b.data_ptr() + b.numel() * 4) for b in blks]
    torch.cuda.synchronize()
    del blks
    return ranges


def _inside(t, ranges):
    return any(lo <= t.data_ptr() < hi for lo, hi in ranges)


@pytest.mark.gpu
def test_outputs_ignore_nan_filled_free_memory(eng, gpu_fe):
    """Each kernel's output, scratch (stage2's conv2_1 columns, FC5's workspace) and partial-group rows taken from NaN-filled
    memory: the output lies inside the poisoned blocks (else the test would test nothing), is finite, and is bit-identical
    to an ordinary run."""
    g = torch.Generator(device=eng.device)
    g.manual_seed(12)
    n = 300
    shapes = {"stage1": (n, 1600, 40), "stage2": (n, 16, 36, 18, 16), "conv31": (n, 12, 15, 7, 32), "conv32t": (n, 10, 8, 5, 15, 8),
              "conv41": (n, 8, 8, 45, 8), "conv42": (n, 6, 16, 27, 8), "fc5": (n, 4, 16, 9, 8)}
    for k, shp in shapes.items():
        x = torch.randn(shp, device=eng.device, generator=g)
        want = R.run_kernel(eng, gpu_fe, k, x)
        sizes = [want.numel()] + ([n * 14 * 36 * 14 * 32] if k == "stage2" else []) + ([4 * n * 128] if k == "fc5" else [])
        ranges = _nan_filled_free_blocks(eng, sizes)
        got = R.run_kernel(eng, gpu_fe, k, x)
        assert _inside(got, ranges), "%s: the output did not land in the NaN-filled blocks: nothing was tested" % k
        assert bool(torch.isfinite(got).all()), k
        assert torch.equal(got, want), k
        del got, want, x
    feat = torch.randn((n, 300, 40), device=eng.device, generator=g)
    crops = torch.randint(0, 220, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
    want = gpu_fe.embed_features(feat, crops)
    ranges = _nan_filled_free_blocks(eng, [n * f for f in (165888, 14 * 36 * 14 * 32, 20160, 48000, 23040, 20736, 4608, 4 * 128, 128)])
    got = gpu_fe.embed_features(feat, crops)
    assert _inside(got, ranges), "embed_features: the output did not land in the NaN-filled blocks"
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
