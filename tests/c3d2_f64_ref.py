"""Float64 references of the seven C3D2 network kernels (tests/test_c3d2_float64.py, tests/test_c3d2_large_launch.py).

Two references per kernel, both started from the f32 tensor the kernel is given (input rounding is never counted as kernel
error):

(A) `ref_a(kernel, fe, x)`: the kernel's OWN arithmetic, exactly, in float64.  A half-pair layer splits its f32 input as the
    kernel does, h = f16(x), l = f16(x - h), and multiplies the pieces by the H | L weight pieces read back from the kernel's
    own operand tables (`FusedEmbedder.*_tables`, so BatchNorm folding and `act_scale` are in): (h + l)(H + L) - l L.  Then
    the folded bias, PReLU and the pool in float64.  conv4_2 (f32 Winograd) and FC5 (f32) take the float64 product of the
    f32 operands they read.  The returned element bound is

        bound = lam * sqrt(K) * 2^-24 * S  +  2^-23 * max(1, |slope|) * |y|

    S = sum|terms|: the float64 convolution of the absolute pieces (|h||H| + |h||L| + |l||H|) plus |bias|, K = the layer's
    dot-product length (input channels x taps).  The first term is the f32 accumulation, taken as a random walk (the worst
    case K * 2^-24 is ~2^-15 at K = 432, too loose to see a lost low piece); lam is calibrated on the CPU emulation below
    (tests/test_c3d2_float64.py::test_emulation_passes_both_references).  The second term covers the epilogue: the bias add and
    the PReLU multiply, one f32 rounding each.
    Propagation: PReLU is max(1, |slope|)-Lipschitz, so an input error e leaves at most max(1, |slope|) e; the (1, 1, 2)
    max-pool is 1-Lipschitz, so the bound of a pooled element is the max of its window's bounds.  In a fused block
    (stage1, stage2) the kernel splits its OWN f32 first-layer output y1' = y1 + e1 (|e1| <= bound1) again; the second
    layer of (A) therefore takes the float64 y1 unsplit and its bound adds

        conv(bound1 + 2^-21 |y1| + 2^-25,  |H2| + |L2|)

    2^-22 |y1| + 2^-25 for what the split of y1' drops (l's rounding, the floor of a subnormal l), 2^-22 |y1| |W| for the
    l L product the kernel leaves out.  The check is elementwise: a wrong tap, channel or piece fails it even where the
    output is small.
    For conv4_2 S is the convolution of |x| with 2 sum_kd |g| (the Winograd F(2, 3) transforms add up to two input and
    three weight values per product) and for FC5 |x| |W|^T + |b|.

(B) `ref_b(kernel, state, x)`: the true layers, float64, unfolded BatchNorm (tests/test_gpu_parity.py::_cpu_layers in
    double), in the true units (the kernel's input times act_scale of the layer before, its output divided by its own).
    `ref_b_f32` is the same on torch-CPU f32: the yardstick the bar is measured against.

`trained_activations()`: eight cubes of eight synthetic speakers through the oracle front end and the trained checkpoint
in float64, each kernel's input (rounded to f32) and float64 output.

`emulate(kernel, fe, x, order, mutant)`: the two-piece arithmetic on the CPU with f32 accumulation in a chosen order
(sequential, pairwise, reversed) -- and with one of five deliberate mistakes (`MUTANTS`), to show that the bars catch them.
"""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKPOINT = os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt")

KERNELS = ("stage1", "stage2", "conv31", "conv32t", "conv41", "conv42", "fc5")
# kernel -> indices into model._LAYERS (FusedEmbedder.stages); FC5 has none
LAYERS_OF = {"stage1": (0, 1), "stage2": (2, 3), "conv31": (4,), "conv32t": (5,), "conv41": (6,), "conv42": (7,), "fc5": ()}
HALF_PAIR = ("stage1", "stage2", "conv31", "conv32t", "conv41")
LAMBDA = 2.0          # calibrated on the CPU emulation: (A) ratio <= 0.2 in every order at this lam (test_emulation_passes_both_references)
EPS = 2.0 ** -24
MUTANTS = ("drop_lx_H", "drop_hx_L", "l_zero_1_in_16", "l_toward_zero", "no_low_at_border_tap")


def _layers():
    from speaker_verification_amd.model import _LAYERS
    return _LAYERS


# ---- the trained checkpoint and its activations --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trained_model():
    """C3D2 with the committed trained checkpoint, eval mode, on the CPU."""
    from speaker_verification_amd.model import C3D2
    ck = torch.load(CHECKPOINT, map_location="cpu", weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    return model.eval()


def state_of(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


@functools.lru_cache(maxsize=None)
def trained_cubes(n_speakers=8):
    """(n, 1, 20, 80, 40) f32: utterance 0 of synthetic speakers 0 .. n - 1 through the oracle front end the checkpoint was
    trained on (preemphasis 0.98 -> lmfe(16 000, 0.025, 0.01, 40, 1 024) -> cmvn with variance), 20 crops each drawn as
    tests/golden/round4.npz drew them (np.random seed 4242)."""
    from oracle import model_ref, speechpy_ref as sp
    from speaker_verification_amd import synth
    rng = np.random.RandomState(4242)
    cubes = []
    for s in range(n_speakers):
        sig = synth.speaker_clip(s, 0) / 32768.0
        feat = sp.lmfe(sp.preemphasis(sig, cof=0.98), 16000, 0.025, 0.01, 40, 1024)
        feat = sp.cmvn(feat, variance_normalization=True)
        cubes.append(model_ref.feature_cube(feat, model_ref.draw_crops(rng, feat.shape[0])))
    return torch.from_numpy(np.stack(cubes))


def _layer_f(state, x, i, dtype):
    tag, _, _, _, stride, pool = _layers()[i]
    g = lambda k: state[k].to(dtype)       # noqa: E731
    x = F.conv3d(x, g(f"conv{tag}.weight"), g(f"conv{tag}.bias"), stride=stride)
    x = F.batch_norm(x, g(f"batch_norm{tag}.running_mean"), g(f"batch_norm{tag}.running_var"), g(f"batch_norm{tag}.weight"),
                     g(f"batch_norm{tag}.bias"), training=False, eps=1e-5)
    x = F.prelu(x, g(f"PReLu{tag}.weight"))
    if pool:
        x = F.max_pool3d(x, kernel_size=(1, 1, 2), stride=(1, 1, 2))
    return x


def _true(kernel, state, x, dtype):
    """The true layers of `kernel` on NCDHW x (FC5: x [n, 4 608] or NCDHW), unfolded BatchNorm, in `dtype`."""
    with torch.no_grad():
        x = x.to(dtype)
        if kernel == "fc5":
            return F.linear(x.reshape(x.shape[0], -1), state["FC5.weight"].to(dtype), state["FC5.bias"].to(dtype))
        for i in LAYERS_OF[kernel]:
            x = _layer_f(state, x, i, dtype)
        return x


def ref_b(kernel, state, x):
    """(B): the true math in float64 on the f32 input x (true units, NCDHW)."""
    return _true(kernel, state, x.float(), torch.float64)


def ref_b_f32(kernel, state, x):
    """torch-CPU f32 of the same layers: the yardstick of (B)."""
    return _true(kernel, state, x.float(), torch.float32)


@functools.lru_cache(maxsize=None)
def trained_activations(n_speakers=8):
    """{kernel: (input f32 NCDHW in true units, float64 output)} of the trained checkpoint on `trained_cubes`: the network in
    float64, each kernel's input rounded to f32."""
    state = state_of(trained_model())
    x = trained_cubes(n_speakers).double()
    out = {}
    for k in KERNELS:
        xin = x.float()
        x = ref_b(k, state, xin)
        out[k] = (xin, x)
    return out


# ---- layouts: NCDHW (true units) <-> what each kernel reads and writes --------------------------------------------------
def _to_chunked(x):
    """(n, C, D, H, W) -> [n][D][C / 8][H * W][8] (csrc/c3d2_tail.hip)."""
    n, C, D, H, W = x.shape
    return x.reshape(n, C // 8, 8, D, H * W).permute(0, 3, 1, 4, 2).contiguous()


def _from_chunked(y, H, W):
    n, D, Cg, P, _ = y.shape
    return y.permute(0, 2, 4, 1, 3).reshape(n, Cg * 8, D, H, W)


def to_kernel(kernel, x):
    """NCDHW -> the kernel's input tensor (stage1: feature rows [n, 1 600, 40] with crop starts 0, 80, ...)."""
    n = x.shape[0]
    if kernel == "stage1":
        return x.reshape(n, 1600, 40).contiguous()
    if kernel in ("stage2", "conv31"):
        return x.permute(0, 2, 3, 4, 1).contiguous()
    if kernel == "conv32t":      # (n, 64, 10, 15, 5) -> [n][10 d][8 chunks][5 w][15 h][8]
        return x.reshape(n, 8, 8, 10, 15, 5).permute(0, 3, 1, 5, 4, 2).contiguous()
    if kernel in ("conv41", "conv42", "fc5"):
        return _to_chunked(x)
    raise KeyError(kernel)


def from_kernel(kernel, y):
    """The kernel's output -> NCDHW ([n, 128] for FC5)."""
    n = y.shape[0]
    if kernel in ("stage1", "stage2"):
        return y.permute(0, 4, 1, 2, 3)
    if kernel == "conv31":       # [n][10 d][8 chunks][5 w][15 h][8] -> (n, 64, 10, 15, 5)
        return y.permute(0, 2, 5, 1, 4, 3).reshape(n, 64, 10, 15, 5)
    if kernel == "conv32t":
        return _from_chunked(y, 9, 5)
    if kernel == "conv41":
        return _from_chunked(y, 9, 3)
    if kernel == "conv42":
        return _from_chunked(y, 3, 3)
    if kernel == "fc5":
        return y
    raise KeyError(kernel)


def from_input(kernel, xk):
    """The kernel's input tensor -> NCDHW (the inverse of to_kernel; stage1's feature rows excepted)."""
    if kernel in ("stage2", "conv31"):
        return xk.permute(0, 4, 1, 2, 3)
    prev = {"conv32t": "conv31", "conv41": "conv32t", "conv42": "conv41", "fc5": "conv42"}[kernel]
    return from_kernel(prev, xk)


def run_kernel(eng, fe, kernel, xk):
    """One launch of `kernel` on its own input layout xk (on the device)."""
    if kernel == "stage1":
        return eng.c3d2_stage1(xk, fe.crop_starts(xk.shape[0], xk.device), fe.stage1_tables())
    return getattr(eng, "c3d2_" + kernel)(xk, getattr(fe, kernel + "_tables")())


def in_scale(fe, kernel):
    """The per-channel power of two the kernel's input is carried in (act_scale of the layer before; ones for the cube)."""
    if kernel == "stage1":
        return None
    prev = LAYERS_OF[kernel][0] - 1 if kernel != "fc5" else 7
    return fe.act_scale[prev].cpu()


def out_scale(fe, kernel):
    return None if kernel == "fc5" else fe.act_scale[LAYERS_OF[kernel][-1]].cpu()


def _chan(s, x):
    return s.to(x.dtype).view((1, -1) + (1,) * (x.dim() - 2))


def to_carried(fe, kernel, x):
    """True units -> the units the kernel reads (exact: powers of two)."""
    s = in_scale(fe, kernel)
    return x if s is None else x * _chan(s, x)


def to_true(fe, kernel, y):
    s = out_scale(fe, kernel)
    return y if s is None else y / _chan(s, y)


# ---- the kernel's own weight pieces, read back from its operand tables --------------------------------------------------
def _builder_tables(kernel, stages):
    from speaker_verification_amd import model as M
    st = [stages[i] for i in LAYERS_OF[kernel]]
    return {"stage1": lambda: M._stage1_tables(*st), "stage2": lambda: M._stage2_tables(*st),
            "conv31": lambda: M._conv31_tables(*st), "conv32t": lambda: M._conv32t_tables(*st),
            "conv41": lambda: M._conv41_tables(*st)}[kernel]()


def _blocks(kernel, tables):
    """The H | L weight-block tensors of each layer of a half-pair kernel's tables (axis -3: 0 = H, 1 = L)."""
    return [tables[0], tables[3]] if kernel in ("stage1", "stage2") else [tables[0]]


def weight_pieces(kernel, fe):
    """[(H, L) float64 in the conv weight's shape (co, ci, kd, kh, kw)] per layer of `kernel`, read from fe's tables: every
    position of the tables is traced back to its weight by building the same tables from weights that hold their own index
    (two f16-exact integer digits), H taken where the weight first appears (all its appearances must agree: `consistent`),
    L summed over its appearances (a weight whose L the layout places twice, or nowhere, shows up as a wrong H + L)."""
    tables = [t.cpu() if torch.is_tensor(t) else t for t in getattr(fe, kernel + "_tables")()]
    out = []
    stages = [tuple(t.cpu() if torch.is_tensor(t) else t for t in s) for s in fe.stages]
    digits = []
    for d in (0, 1):
        enc = list(stages)
        for i in LAYERS_OF[kernel]:
            w = stages[i][0]
            idx = torch.arange(1, w.numel() + 1, dtype=torch.int64).view(w.shape)
            enc[i] = ((idx % 2048 if d == 0 else idx // 2048).to(torch.float32),) + tuple(stages[i][1:])
        digits.append(_builder_tables(kernel, enc))
    for j, i in enumerate(LAYERS_OF[kernel]):
        w = stages[i][0]
        blk = _blocks(kernel, tables)[j].double()
        lo, hi = (_blocks(kernel, dg)[j].select(-3, 0).double() for dg in digits)
        idx = (hi * 2048 + lo).long().reshape(-1) - 1           # -1: a zero pad slot
        hv, lv = blk.select(-3, 0).reshape(-1), blk.select(-3, 1).reshape(-1)
        keep = idx >= 0
        H = torch.zeros(w.numel(), dtype=torch.float64)
        H[idx[keep]] = hv[keep]
        Hmin = torch.full((w.numel(),), math.inf, dtype=torch.float64).scatter_reduce(0, idx[keep], hv[keep], "amin")
        Hmax = torch.full((w.numel(),), -math.inf, dtype=torch.float64).scatter_reduce(0, idx[keep], hv[keep], "amax")
        L = torch.zeros(w.numel(), dtype=torch.float64).index_add_(0, idx[keep], lv[keep])
        seen = torch.zeros(w.numel(), dtype=torch.bool)
        seen[idx[keep]] = True
        pads_zero = bool((blk.select(-3, 0).reshape(-1)[~keep] == 0).all() and (lv[~keep] == 0).all())
        out.append(dict(H=H.view(w.shape), L=L.view(w.shape), consistent=bool((Hmin == Hmax)[seen].all()),
                        covered=bool(seen.all()), pads_zero=pads_zero, w=w.double()))
    return out


# ---- reference (A) -------------------------------------------------------------------------------------------------------
def split(x):
    """The kernel's split of f32 x: h = f16(x), l = f16(x - h), as float64."""
    x = x.float()
    h = x.half()
    return h.double(), (x - h.float()).half().double()


def _epilogue(acc, S, bound_in, b, slope, pool, K, lam=None):
    """bias, PReLU, pool in float64 on the accumulated float64 sum; -> (y, bound) (the module docstring)."""
    v = acc + _chan(b, acc)
    S = S + _chan(b.abs(), acc)
    s = _chan(slope, acc)
    lip = torch.clamp(s.abs(), min=1.0)
    y = torch.where(v >= 0, v, v * s)
    bound = lip * ((lam or LAMBDA) * math.sqrt(K) * EPS * S + bound_in) + 2.0 ** -23 * lip * v.abs()
    if pool:
        y = F.max_pool3d(y, kernel_size=(1, 1, 2), stride=(1, 1, 2))
        bound = F.max_pool3d(bound, kernel_size=(1, 1, 2), stride=(1, 1, 2))
    return y, bound


def ref_a(kernel, fe, x, lam=None):
    """(A) on the kernel's input x (NCDHW f32, in the units the kernel reads; FC5: [n, 4 608] or NCDHW) -> (float64 output
    in the kernel's units, element bound), NCDHW."""
    x = x.float()
    if kernel == "fc5":
        w = fe.fc_w.cpu().double()
        b = fe.fc_b.cpu().double()
        xd = x.reshape(x.shape[0], -1).double()
        y = xd @ w.T + b
        S = xd.abs() @ w.abs().T + b.abs()
        return y, (lam or LAMBDA) * math.sqrt(w.shape[1]) * EPS * S + 2.0 ** -23 * y.abs()
    if kernel == "conv42":
        w, b, sl, stride, pool = (t.cpu() if torch.is_tensor(t) else t for t in fe.stages[7])
        w = w.double()
        xd = x.double()
        acc = F.conv3d(xd, w, stride=stride)
        wabs = 2.0 * w.abs().sum(dim=2, keepdim=True).expand_as(w)
        S = F.conv3d(xd.abs(), wabs, stride=stride)
        return _epilogue(acc, S, 0.0, b.double(), _slopes(sl, w.shape[0]), pool, w[0].numel(), lam)
    pieces = weight_pieces(kernel, fe)
    y, bound = None, 0.0
    for j, i in enumerate(LAYERS_OF[kernel]):
        _, b, sl, stride, pool = (t.cpu() if torch.is_tensor(t) else t for t in fe.stages[i])
        H, L = pieces[j]["H"], pieces[j]["L"]
        K = H[0].numel()
        if j == 0:
            h, l = split(x)
            acc = F.conv3d(h, H + L, stride=stride) + F.conv3d(l, H, stride=stride)
            S = F.conv3d(h.abs(), H.abs() + L.abs(), stride=stride) + F.conv3d(l.abs(), H.abs(), stride=stride)
            carried = 0.0
        else:       # the fused second layer: y unsplit, the first layer's bound and the split of its f32 output carried
            wa = H.abs() + L.abs()
            acc = F.conv3d(y, H + L, stride=stride)
            S = F.conv3d(y.abs(), wa, stride=stride)
            carried = F.conv3d(bound + 2.0 ** -21 * y.abs() + 2.0 ** -25, wa, stride=stride)
        y, bound = _epilogue(acc, S, carried, b.double(), _slopes(sl, H.shape[0]), pool, K, lam)
    return y, bound


def ref_a_layer1_max(fe, x):
    """max |conv1_1 output| of stage1 on x, float64: what the kernel splits again inside (must stay below 65 504)."""
    w, b, *_ = (t.cpu() if torch.is_tensor(t) else t for t in fe.stages[0])
    return (F.conv3d(x.double(), w.double()) + _chan(b.double(), x)).abs().max()


def _slopes(sl, co):
    sl = sl.double().reshape(-1)
    return sl.expand(co) if sl.numel() == 1 else sl


# ---- CPU emulation of the two-piece arithmetic, f32 accumulation -------------------------------------------------------
def _f16_toward_zero(v):
    """f16(v) rounded toward zero (v f32)."""
    r = v.numpy().astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v.numpy())
    r[over] = np.nextafter(r[over], np.float16(0))
    return torch.from_numpy(r)


def _patches(x, ksize, stride):
    """(n, ci, D, H, W) -> [n * Do * Ho * Wo, ci * kd * kh * kw] in the conv weight's K order."""
    kd, kh, kw = ksize
    sd, sh, sw = stride
    p = x.unfold(2, kd, sd).unfold(3, kh, sh).unfold(4, kw, sw)              # n, ci, Do, Ho, Wo, kd, kh, kw
    n, ci, Do, Ho, Wo = p.shape[:5]
    return p.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(n * Do * Ho * Wo, ci * kd * kh * kw), (n, Do, Ho, Wo)


def _accumulate(P, order, block=32):
    """Sum f32 products P [M, co, K] over K in f32 in the given order: "pairwise" (a binary tree over K), "sequential" /
    "reversed" (one running sum over blocks of `block` products in K order / the reverse, each block summed pairwise first:
    what one MFMA per block does to an f32 accumulator: K = 32 for v_mfma_f32_16x16x32_f16, 4 for v_mfma_f32_16x16x4_f32), "sequential1" (one running sum over every
    single product: no kernel here accumulates so; (A) holds for it, (B)'s bar does not -- test_emulation_orders)."""
    if order in ("sequential", "reversed") and P.shape[-1] > block:
        pad = (-P.shape[-1]) % block
        if pad:
            P = torch.cat([P, torch.zeros(P.shape[:-1] + (pad,), dtype=P.dtype)], -1)
        B = _accumulate(P.reshape(P.shape[:-1] + (-1, block)), "pairwise")
        return _accumulate(B, order + "1")
    if order == "pairwise":
        while P.shape[-1] > 1:
            if P.shape[-1] % 2:
                P = torch.cat([P, torch.zeros_like(P[..., :1])], -1)
            P = P[..., 0::2] + P[..., 1::2]
        return P[..., 0]
    seq = range(P.shape[-1]) if order.startswith("sequential") else range(P.shape[-1] - 1, -1, -1)
    acc = torch.zeros(P.shape[:-1], dtype=torch.float32)
    for k in seq:
        acc = acc + P[..., k]
    return acc


def _emulate_conv(x, H, L, b, sl, stride, pool, order, mutant, two_piece=True):
    """One conv layer (+ bias, PReLU, pool) in f32 the way the kernels compute it: x f32 NCDHW, H / L float64 weight pieces
    (f16 values; two_piece False: H = the f32 weight, L unused)."""
    co = H.shape[0]
    K = H[0].numel()
    ksize = tuple(H.shape[2:])
    xp, (n, Do, Ho, Wo) = _patches(x.float(), ksize, stride)
    Hm = H.float().reshape(co, K)
    outs = []
    for m0 in range(0, xp.shape[0], 4096):
        xs = xp[m0:m0 + 4096]
        if not two_piece:
            P = xs[:, None, :] * Hm[None]
        else:
            h = xs.half()
            d = xs - h.float()
            l = (_f16_toward_zero(d) if mutant == "l_toward_zero" else d.half()).float()
            h = h.float()
            Lm = L.float().reshape(co, K)
            if mutant == "l_zero_1_in_16":
                ci = torch.arange(K) // (K // H.shape[1])
                l = torch.where((ci % 16 == 0)[None], torch.zeros_like(l), l)
            lH = l[:, None, :] * Hm[None]
            hL = h[:, None, :] * Lm[None]
            if mutant == "drop_lx_H":
                lH = torch.zeros_like(lH)
            if mutant == "drop_hx_L":
                hL = torch.zeros_like(hL)
            if mutant == "no_low_at_border_tap":
                taps = int(np.prod(ksize))
                last = (torch.arange(K) % taps) == taps - 1
                lH[..., last] = 0
                hL[..., last] = 0
            P = torch.stack((h[:, None, :] * Hm[None], lH, hL), -1).reshape(xs.shape[0], co, 3 * K)
        outs.append(_accumulate(P, order, 32 if two_piece else 4))
    acc = torch.cat(outs).view(n, Do, Ho, Wo, co).permute(0, 4, 1, 2, 3)
    v = acc + b.float().view(1, -1, 1, 1, 1)
    s = _slopes(sl, co).float().view(1, -1, 1, 1, 1)
    y = torch.where(v >= 0, v, v * s)
    if pool:
        y = F.max_pool3d(y, kernel_size=(1, 1, 2), stride=(1, 1, 2))
    return y


def emulate(kernel, fe, x, order="sequential", mutant=None):
    """`kernel` on the CPU in f32 the way the GPU computes it (x: NCDHW f32 in the kernel's units) -> f32 NCDHW (FC5 [n, 128])."""
    x = x.float()
    if kernel == "fc5":
        w, b = fe.fc_w.cpu().float(), fe.fc_b.cpu().float()
        P = x.reshape(x.shape[0], 1, -1) * w[None]
        return _accumulate(P, order, 4) + b
    if kernel == "conv42":
        w, b, sl, stride, pool = (t.cpu() if torch.is_tensor(t) else t for t in fe.stages[7])
        return _emulate_conv(x, w.double(), None, b, sl, stride, pool, order, None, two_piece=False)
    pieces = weight_pieces(kernel, fe)
    for j, i in enumerate(LAYERS_OF[kernel]):
        _, b, sl, stride, pool = (t.cpu() if torch.is_tensor(t) else t for t in fe.stages[i])
        x = _emulate_conv(x, pieces[j]["H"], pieces[j]["L"], b, sl, stride, pool, order, mutant)
    return x


# ---- the two checks ------------------------------------------------------------------------------------------------------
def check_a(got, ref, bound):
    """-> (max of |got - ref| / bound, index of the worst element); <= 1 passes."""
    err = (got.double() - ref).abs() / bound
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    k = int(torch.argmax(err))
    return float(err.reshape(-1)[k]), k


def errors_b(got, ref):
    """(max |err| / scale, RMS err / scale) of `got` against the float64 `ref`; scale = max |ref|."""
    scale = float(ref.abs().max())
    d = got.double() - ref
    return float(d.abs().max()) / scale, float(torch.sqrt((d * d).mean())) / scale


# (B): the kernel's (max, RMS) error / scale may be at most FACTOR x torch-CPU f32's + 2^-24.  The proposal was 2 x for both;
# measured on the CPU emulation (blocked MFMA-like orders) the pieces' 22 bits put the RMS of the half-pair layers at up to
# 2.5 x torch's, and a long f32 MFMA chain (conv4_2 K = 2 688, FC5 K = 4 608, blocks of 4) against torch-CPU's blocked
# GEMM at 3.2 x and 12 x.  Every mutant of MUTANTS but the rounding-direction one still fails these bars by >= 9 x.
FACTOR = {"stage1": (2, 4), "stage2": (2, 4), "conv31": (2, 4), "conv32t": (2, 4), "conv41": (2, 4), "conv42": (4, 4),
          "fc5": (16, 8)}


def bar_b(kernel, yard):
    """The (B) bars from torch-CPU f32's (max, RMS) errors."""
    return tuple(f * e + EPS for f, e in zip(FACTOR[kernel], yard))


def crop_depth(kernel, x, out_depth=2):
    """The input slice along depth that gives `out_depth` output depths of `kernel` (the emulation's window)."""
    if kernel == "fc5":
        return x
    need = out_depth + 2 * len(LAYERS_OF[kernel])      # every conv has 3 depth taps
    return x[:, :, :need]
