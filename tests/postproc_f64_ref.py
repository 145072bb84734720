"""Float64 references, error bars, CPU emulations and mutants for the feature post-processing kernels of csrc/stages.hip
(svk_cmvn, svk_cmvn_stats, svk_cmvnw, svk_derivative, svk_log_power, svk_cube_gather[_cmvn], svk_cube_draw_crops).  Used by
tests/test_postprocessing_float64.py and tests/test_cmvn_route_invariance.py (the two summation orders of the CMVN kernels).

THE BARS.  ulp32(v) is the float32 spacing at |v|.  The CMVN kernels compute in float64 and round to float32 once (cmvnw with
variance: twice, the centred rows are stored as float32 between the passes).  A kernel's float64 sums differ from the
reference's only in the order of the additions, by at most n 2^-52 max|x| per sum of n rows; two float64 values that close round
to float32 values at most one ulp apart.  Hence

    |got - want32| <= k ulp32(want32) + floor,    floor = n 2^-50 max|x| inv

per column, with k = 1 (cmvn, cmvn_stats + gather, cmvnw mean only) or k = 2 (cmvnw with variance: one ulp from the stored
centred row, one from the final rounding), inv = the largest 1 / (std + 2^-30) of the column (1 without variance) and n = the
number of rows that enter the LONGEST float64 sum the path forms:
    cmvn                  n = T                      (a column sum over the clip)
    cmvnw, sliding kernel n = win + 2 (seg - 1)      (a direct window sum, then one row in and one out per step of the segment)
    cmvnw, tile kernel    n = T + (win - 1) / 2 + 1  (the longest prefix sum it looks up, F(r + half + 1))
    the reference itself  n = win                    (what the reference's own direct sums may be off by)
`worst_ulps` returns max (|got - want| - floor) / ulp32(want): the bar is worst_ulps <= k.

Where a window or a column has std = 0 exactly (a constant column, a one-row clip) inv = 2^30 multiplies whatever rounding the
mean carries: there the ulp term means nothing and the floor alone decides.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

EPS = 2.0 ** -30
M64 = (1 << 64) - 1
SEG = 128                      # rows per thread of cmvnw_kernel (svk_cmvnw)
CW_CAP = 3900                  # svk_cmvnw: clips of up to this many frames take cmvnw_tile_kernel


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def worst_ulps(got, want, floor):
    """max over elements of (|got - want| - floor) / ulp32(want), never below 0.  `floor` broadcasts against the arrays."""
    got, want = np.asarray(got), np.asarray(want)
    if want.size == 0:
        return 0.0
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)) - floor
    return float(np.max(np.maximum(d, 0.0) / ulp32(want)))


def mismatches(got, want, floor):
    """(elements of got that differ from want by more than floor, the budget for that count).  got != want32 needs a float32
    rounding boundary between two float64 values at most `floor` apart: a chance of at most floor / ulp32 per element.  The
    budget is the sum of min(1, 2 floor / ulp32) over the elements, s, plus 5 sqrt(s) + 1."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    s = float(np.minimum(1.0, 2.0 * floor / ulp32(want) * np.ones(np.shape(want))).sum())
    return int((d > floor).sum()), s + 5.0 * np.sqrt(s) + 1.0


# ---- cmvn -------------------------------------------------------------------------------------------------------------
def cmvn_ref(x32, variance):
    """-> (want32 [T, C], mean [C], inv [C], floor [C]) of one clip: the header's own expression in float64."""
    x = np.asarray(x32, dtype=np.float64)
    T = x.shape[0]
    m = x.mean(0)
    inv = 1.0 / (x.std(0) + EPS) if variance else np.ones_like(m)
    want = ((x - m) * inv).astype(np.float32)
    return want, m, inv, T * 2.0 ** -50 * np.abs(x).max(0) * inv


def cmvn_stats_one_pass(x32):
    """The kernels' formula in float64 with exactly rounded-once sums (math.fsum is out of reach for arrays: long double
    accumulators): mean and 1 / (sqrt(max(E[x^2] - mean^2, 0)) + 2^-30).  What the one-pass formula costs by itself."""
    x = np.asarray(x32, dtype=np.float64)
    T = x.shape[0]
    xl = x.astype(np.longdouble)
    mean = (xl.sum(0) / T).astype(np.float64)
    ex2 = ((xl * xl).sum(0) / T).astype(np.float64)
    var = np.maximum(ex2 - mean * mean, 0.0)
    return mean, 1.0 / (np.sqrt(var) + EPS)


def emul_cmvn(x32, variance, mut=None):
    """cmvn_kernel<true> on one clip, operation for operation: 256 threads as [R][cb] over blocks of 256 columns, every thread
    sums its rows t = tr, tr + R, ... in order, the R partial sums are added in order, var = E[x^2] - mean^2."""
    x32 = np.asarray(x32, dtype=np.float32)
    T, C = x32.shape
    out = np.empty_like(x32)
    for c0 in range(0, C, 256):
        cb = min(256, C - c0)
        R = 256 // cb
        x = x32[:, c0:c0 + cb].astype(np.float64)
        s1 = np.zeros((R, cb))
        s2 = np.zeros((R, cb))
        for tr in range(min(R, T)):
            rows = x[tr::R]
            s1[tr] = np.cumsum(rows, axis=0)[-1]                     # cumsum adds in order
            s2[tr] = np.cumsum(rows * rows, axis=0)[-1]
        mean = np.cumsum(s1, axis=0)[-1] / T
        inv = np.ones(cb)
        if variance:
            var = np.cumsum(s2, axis=0)[-1] / T - mean * mean
            if mut == "ddof1":
                var = var * T / max(T - 1, 1)
            var = np.maximum(var, 0.0)
            inv = 1.0 / (np.sqrt(var) + (2.0 ** -20 if mut == "eps20" else EPS))
        out[:, c0:c0 + cb] = ((x - mean) * inv).astype(np.float32)
    return out


CMVN_CHUNK = 256               # frames per workgroup of cmvn_partial_kernel
CMVN_WHOLE = 1024              # clips of up to this many frames are summed whole, in cmvn_kernel's order, on every route


def _ordered_sums(x, R):
    """Column sums and sums of squares of x [T, cb] float64 as one workgroup forms them: row group tr adds the rows tr, tr + R, ..
    in order, then the R partial sums are added in order.  -> (s [cb], q [cb])"""
    T, cb = x.shape
    s1 = np.zeros((R, cb))
    s2 = np.zeros((R, cb))
    for tr in range(min(R, T)):
        rows = x[tr::R]
        s1[tr] = np.cumsum(rows, axis=0)[-1]                         # cumsum adds in order
        s2[tr] = np.cumsum(rows * rows, axis=0)[-1]                  # the square of a float32 is exact in float64: fused or not
    return np.cumsum(s1, axis=0)[-1], np.cumsum(s2, axis=0)[-1]


def emul_cmvn_sums(x32, order):
    """The float64 column sums behind a clip's CMVN statistics, in one of the two orders the kernels know.  order = "whole":
    cmvn_kernel's (and, for clips of up to CMVN_WHOLE frames, the chunk-0 workgroup's of the split launch); order = "chunked":
    cmvn_partial_kernel's inside each chunk of CMVN_CHUNK frames, the chunks then added in order (cmvn_stats_kernel).
    -> (s [C], q [C]); mean = s / T."""
    x32 = np.asarray(x32, dtype=np.float32)
    T, C = x32.shape
    s, q = np.zeros(C), np.zeros(C)
    for c0 in range(0, C, 256):
        cb = min(256, C - c0)
        x = x32[:, c0:c0 + cb].astype(np.float64)
        if order == "whole":
            s[c0:c0 + cb], q[c0:c0 + cb] = _ordered_sums(x, 256 // cb)
        else:
            assert order == "chunked"
            parts = [_ordered_sums(x[t0:t0 + CMVN_CHUNK], 256 // cb) for t0 in range(0, T, CMVN_CHUNK)]
            s[c0:c0 + cb] = np.cumsum(np.stack([p[0] for p in parts]), axis=0)[-1]
            q[c0:c0 + cb] = np.cumsum(np.stack([p[1] for p in parts]), axis=0)[-1]
    return s, q


def cmvn_order(T):
    """The order a clip's own frame count selects (csrc/stages.hip, CMVN_WHOLE)."""
    return "whole" if T <= CMVN_WHOLE else "chunked"


def ulp64_distance(a, b):
    """Element-wise distance of two float64 arrays in units of the last place (same-sign finite values)."""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)


# ---- cmvnw ------------------------------------------------------------------------------------------------------------
def _window_stats(a, win, want_std, pad="symmetric"):
    """Direct sums over every row's window of the padded array: (mean [T, C], std [T, C] or None).  No running sums."""
    half = (win - 1) // 2
    T, C = a.shape
    p = np.pad(a, ((half, half), (0, 0)), pad)
    v = sliding_window_view(p, win, axis=0)                           # [T, C, win], a view
    mean = np.empty((T, C))
    std = np.empty((T, C)) if want_std else None
    step = max(1, 2_000_000 // (win * C))
    for i in range(0, T, step):
        blk = v[i:i + step]
        mean[i:i + step] = blk.mean(axis=-1)
        if want_std:
            std[i:i + step] = blk.std(axis=-1)
    return mean, std


def cmvnw_ref(x32, win, pad="symmetric"):
    """One clip [T, C] -> dict(centred, out, inv): out = x - window mean rounded to float32 (`centred`, the mean-only result),
    then / (population std of the window over those float32 rows + 2^-30), rounded to float32 (`out`); inv [T, C] = the float64
    1 / (std + 2^-30).  This is oracle.speechpy_ref.cmvnw with its row loop replaced by a strided view and its second pass
    (float32 in the oracle, whatever the input type) in float64."""
    x = np.asarray(x32, dtype=np.float64)
    mean, _ = _window_stats(x, win, False, pad)
    centred = (x - mean).astype(np.float32)
    _, std = _window_stats(centred.astype(np.float64), win, True, pad)
    inv = 1.0 / (std + EPS)
    return {"centred": centred, "out": (centred.astype(np.float64) / (std + EPS)).astype(np.float32), "inv": inv}


def cmvnw_n(path, T, win):
    """n of the floor for a cmvnw path (module docstring)."""
    return {"sliding": win + 2 * (SEG - 1), "tile": T + (win - 1) // 2 + 1, "reference": win}[path]


def cmvnw_floor(x32, ref, variance, n):
    """[C]: n 2^-50 max|x| inv, inv = the column's largest 1 / (std + 2^-30) with variance and 1 without."""
    inv = ref["inv"].max(0) if variance else 1.0
    return n * 2.0 ** -50 * np.abs(np.asarray(x32, np.float64)).max(0) * inv


def _sym(k, T):
    m = np.mod(k, 2 * T)
    return np.where(m < T, m, 2 * T - 1 - m)


def _reflect(k, T):                                                    # np.pad's 'reflect': the edge sample is not repeated
    if T == 1:
        return np.zeros_like(k)
    m = np.mod(k, 2 * T - 2)
    return np.where(m < T, m, 2 * T - 2 - m)


def _slide_pass(src, raw, win, passno, seg, mut):
    """One launch of cmvnw_kernel on one clip: thread = (segment, column); `raw` feeds the variance window of the
    'rawvar' mutant."""
    T, C = src.shape
    half = (win - 1) // 2
    idx = _reflect if mut == "reflect" else _sym
    sh = 1 if mut == "shift" else 0
    b = np.asarray(src, dtype=np.float64)
    rawvar = mut == "rawvar" and passno == 1
    w = np.asarray(raw, dtype=np.float64) if rawvar else b
    wmean = _window_stats(w, win, False)[0] if rawvar else None         # the raw rows' window mean goes with their squares
    inv_win = 1.0 / win
    r0 = np.arange(0, T, seg)
    s = np.zeros((r0.size, C))
    q = np.zeros((r0.size, C))
    for k in range(-half, half + 1):
        s += b[idx(r0 + k + sh, T)]
        v = w[idx(r0 + k + sh, T)]
        q += v * v
    out = np.empty((T, C), dtype=np.float64 if (mut == "y64" and passno == 0) else np.float32)
    for j in range(seg):
        r = r0 + j
        live = r < T
        if j > 0:
            vin, vout = b[idx(r + half + sh, T)], b[idx(r - half - 1 + sh, T)]
            s += (vin * (1.0 + 2.0 ** -30) if mut == "leak" else vin) - vout
            vin, vout = w[idx(r + half + sh, T)], w[idx(r - half - 1 + sh, T)]
            q += vin * vin - vout * vout
        mean = s * inv_win
        x = b[np.minimum(r, T - 1)]
        if passno == 0:
            o = x - mean
        else:
            m2 = wmean[np.minimum(r, T - 1)] if rawvar else mean
            var = q * inv_win - m2 * m2
            if mut == "ddof1":
                var = var * win / max(win - 1, 1)
            var = np.maximum(var, 0.0)
            o = x / (np.sqrt(var) + (2.0 ** -20 if mut == "eps20" else EPS))
        out[r[live]] = o[live]
    return out


def emul_cmvnw_sliding(x32, win, variance, mut=None, seg=SEG):
    x32 = np.asarray(x32, dtype=np.float32)
    y = _slide_pass(x32, x32, win, 0, seg, mut)
    if not variance:
        return y.astype(np.float32)
    return _slide_pass(y, x32, win, 1, seg, mut).astype(np.float32)


def _scan64(a, drop_carry_at=None):
    """Prefix sums along time as cmvnw_tile_kernel forms them: a wave-wide inclusive scan (shuffle-up by 1, 2, .. 32) over 64
    rows at a time plus a carry.  a [T, C] float64 -> P [T + 1, C]."""
    T, C = a.shape
    nb = -(-T // 64)
    v = np.zeros((nb * 64, C))
    v[:T] = a
    v = v.reshape(nb, 64, C)
    d = 1
    while d < 64:
        u = v.copy()
        v[:, d:] += u[:, :-d]
        d <<= 1
    tot = v[:, 63].copy()
    if drop_carry_at is not None and drop_carry_at < nb:
        tot[drop_carry_at] = 0.0
    carry = np.concatenate([np.zeros((1, C)), np.cumsum(tot, axis=0)[:-1]])
    P = np.zeros((T + 1, C))
    P[1:] = (carry[:, None, :] + v).reshape(nb * 64, C)[:T]
    return P


def _prefix_at(P, T, n):
    q, r = np.divmod(n, 2 * T)
    p2 = np.where((r <= T)[:, None], P[np.minimum(r, T)], 2.0 * P[T] - P[np.where(r <= T, 0, 2 * T - r)])
    return q[:, None].astype(np.float64) * (2.0 * P[T]) + p2


def emul_cmvnw_tile(x32, win, variance, mut=None):
    x32 = np.asarray(x32, dtype=np.float32)
    T, C = x32.shape
    half = (win - 1) // 2
    inv_win = 1.0 / win
    r = np.arange(T) + (1 if mut == "shift" else 0)
    drop = 1 if mut == "carry" else None
    A = x32.astype(np.float64)
    P = _scan64(A, drop)
    mean = (_prefix_at(P, T, r + half + 1) - _prefix_at(P, T, r - half)) * inv_win
    y = A - mean
    if mut != "y64":
        y = y.astype(np.float32)
    if not variance:
        return y.astype(np.float32)
    y = y.astype(np.float64)
    w = A if mut == "rawvar" else y
    P, Q = _scan64(w, drop), _scan64(w * w, drop)
    mean = (_prefix_at(P, T, r + half + 1) - _prefix_at(P, T, r - half)) * inv_win
    var = (_prefix_at(Q, T, r + half + 1) - _prefix_at(Q, T, r - half)) * inv_win - mean * mean
    if mut == "ddof1":
        var = var * win / max(win - 1, 1)
    var = np.maximum(var, 0.0)
    return (y / (np.sqrt(var) + (2.0 ** -20 if mut == "eps20" else EPS))).astype(np.float32)


SLIDING_MUTANTS = ("shift", "reflect", "ddof1", "eps20", "y64", "rawvar", "leak")
TILE_MUTANTS = ("shift", "ddof1", "eps20", "y64", "rawvar", "carry")
CMVN_MUTANTS = ("ddof1", "eps20")


# ---- derivative ---------------------------------------------------------------------------------------------------------
def derivative_bar(x32, delta):
    """(delta + 2) 2^-24 sum_k k |x_k| / scale per element: delta float32 multiply-adds and one float32 scale, whose factor is
    itself rounded once."""
    x = np.abs(np.asarray(x32, dtype=np.float64))
    C = x.shape[-1]
    acc = np.zeros_like(x)
    scale = 0.0
    for k in range(1, delta + 1):
        acc += k * x[..., np.minimum(np.arange(C) + k, C - 1)]
        scale += 2.0 * k * k
    return (delta + 2) * 2.0 ** -24 * acc / scale


# ---- crop starts -------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw_ref(n_frames, gids, n_crops, crop_frames, seed, mut=None):
    """svk.h's arithmetic in Python integers -> (starts [n, n_crops] int32, number of clips too short to crop)."""
    out = np.empty((len(n_frames), n_crops), dtype=np.int32)
    bad = 0
    seed &= M64
    for u, (nf, g) in enumerate(zip(n_frames, gids)):
        rng = int(nf) - crop_frames
        if rng <= 0:
            out[u] = -1
            bad += 1 if n_crops > 0 else 0
            continue
        g = int(g) & M64
        key = splitmix64(((seed + g) & M64) if mut == "plus" else (seed ^ g))
        for c in range(n_crops):
            r = splitmix64((key + c) & M64)
            out[u, c] = ((r * rng) & M64) % rng if mut == "low" else (r * rng) >> 64
    return out, bad


# ---- feature cube -------------------------------------------------------------------------------------------------------
def cube_ref(feat, crops, crop_frames):
    """feat [n, T, C], crops [n, k] -> [n, 1, k, crop_frames, C]: rows at or past T are zeros; starts < 0 or > T give zero
    cubes."""
    n, T, C = feat.shape
    k = crops.shape[1]
    out = np.zeros((n, 1, k, crop_frames, C), dtype=feat.dtype)
    for u in range(n):
        for j in range(k):
            s = int(crops[u, j])
            if 0 <= s <= T:
                rows = feat[u, s:min(T, s + crop_frames)]
                out[u, 0, j, :rows.shape[0]] = rows
    return out
