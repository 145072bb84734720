"""TEST INFRASTRUCTURE for tests/test_ingest_float64.py: svk_ingest_resample's float64 reference, the derived bars, NumPy
emulations of resample_kernel and decimate_kernel with their mutants, and the case list.

Reference.  y64[m] = sum_j x[j] * h32[m down + half - j up] in float64, x = (sum_c pcm[j, c]) / (32768 n_ch), h32 the float32
taps AS UPLOADED, zero outside the clip, ceil(n up / down) outputs.  It differs from oracle.ingest_ref.resample_poly only by the
float32 rounding of the taps (held to 1e-7 on the CPU).

Float bar.  The kernels hold x in float32: float(acc) is exact (|acc| <= 8 * 32768), `scale` = 1 / (32768 n_ch) is one
rounding and acc * scale a second one.  The sum is a chain y = fma(x, h, y) over the n_m frames of the clip that the output
touches (frames outside add an exact zero): one rounding each.  To first order the error is therefore at most
(n_m + 2) u sum_j |x[j]| |h32[k]|, u = 2^-24; 1.01 covers the higher-order terms ((n_m + 2) u < 1e-5):

    |got - y64[m]| <= bar[m] = 1.01 (n_m + 2) 2^-24 sum_j |x[j]| |h32[k]|

Int16 bar.  The int16 output is sat(rintf(y * 32768)) of the same y (the product with 2^15 is exact), rint and sat are
monotone, so with v = 32768 y64[m] and d = 32768 bar[m] it lies in [sat(rint(v - d)), sat(rint(v + d))], with no exclusions.
That interval holds ONE value except where v is within d of a tie; the share of such samples is held to <= 10 % on every
random-input case (asserted from the reference alone), so a kernel that truncates, or rounds ties the wrong way on more than
that share, fails.
"""
import numpy as np

from speaker_verification_amd.ingest import resample_taps

U = 2.0 ** -24
GARBAGE = (32767, -32768)          # what lies behind in_len


def taps32(up, down, taps=None):
    """The float32 taps as Engine.resample uploads them."""
    return np.asarray(resample_taps(up, down) if taps is None else taps, dtype=np.float32)


def custom_taps(down=3, half=15):
    """A non-default design for 1/3 (31 taps): Hamming-windowed sinc, unit DC gain.  Its tap count is not 20 down + 1, so the
    library takes the generic kernel for an integer decimation."""
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(n / down) * np.hamming(2 * half + 1)
    return h / h.sum()


def mono64(pcm):
    pcm = np.asarray(pcm)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    return pcm.astype(np.int64).sum(axis=1).astype(np.float64) / (32768.0 * pcm.shape[1])


def n_out_of(n_in, up, down):
    return -(-int(n_in) * up // down)


def reference(pcm, up, down, h32):
    """(y64, bar, n_m) of one clip, pcm int16 [n] or [n, n_ch] cut to its length."""
    x = mono64(pcm)
    h = np.asarray(h32, dtype=np.float64)
    half = (len(h) - 1) // 2
    n_out = n_out_of(len(x), up, down)
    y, s = np.zeros(n_out), np.zeros(n_out)
    cnt = np.zeros(n_out, dtype=np.int64)
    t = np.arange(n_out, dtype=np.int64) * down
    j_lo = -((half - t) // up)              # ceil((t - half) / up)
    j_hi = (t + half) // up
    for step in range(int((j_hi - j_lo).max()) + 1 if n_out else 0):
        j = j_lo + step
        ok = (j <= j_hi) & (j >= 0) & (j < len(x))
        k = t + half - j * up
        y[ok] += x[j[ok]] * h[k[ok]]
        s[ok] += np.abs(x[j[ok]] * h[k[ok]])
        cnt[ok] += 1
    return y, 1.01 * (cnt + 2) * U * s, cnt


def sat_rint(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int64)


def int16_interval(y64, bar):
    return sat_rint(32768.0 * (y64 - bar)), sat_rint(32768.0 * (y64 + bar))


def float_ratio(got, y64, bar):
    """Worst |error| / bar; inf where the bar is 0 and the error is not."""
    err = np.abs(np.asarray(got, dtype=np.float64) - y64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def int16_from_float(y32):
    """sat(rintf(y * 32768)) of a float32 output: what the int16 output of the same call must equal bit for bit."""
    r = np.rint(np.asarray(y32, dtype=np.float32) * np.float32(32768.0))
    return np.clip(r, -32768, 32767).astype(np.int16)


# ---- emulations ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("first tap dropped", "last tap dropped", "tap index off by one", "1/32767 scale", "floor for ceil in the output count",
           "truncation for rintf", "no clamp", "down-mix by sum without / n_ch", "samples past in_len read")


def _scale(n_ch, mutant):
    if mutant == "1/32767 scale":
        return np.float32(1.0) / (np.float32(32767.0) * np.float32(n_ch))
    if mutant == "down-mix by sum without / n_ch":
        return np.float32(1.0) / np.float32(32768.0)
    return np.float32(1.0) / (np.float32(32768.0) * np.float32(n_ch))


def _fma(x, h, y):
    """fmaf: the float32 x float32 product is exact in float64, the sum is rounded there and once more to float32."""
    return (x.astype(np.float64) * h.astype(np.float64) + y.astype(np.float64)).astype(np.float32)


def _n_out(n_in, up, down, clip_out, mutant):
    n = int(n_in) * up // down if mutant == "floor for ceil in the output count" else n_out_of(n_in, up, down)
    return n if clip_out is None else min(n, clip_out)


def _store(y, out, mutant):
    if out == "f32":
        return y
    r = y * np.float32(32768.0)
    r = np.trunc(r) if mutant == "truncation for rintf" else np.rint(r)
    if mutant != "no clamp":
        r = np.clip(r, -32768, 32767)
    return r.astype(np.int64).astype(np.int16)          # (without the clamp: wraps, as a 16-bit store of the integer would)


def _xs(row, n_in, n_ch, j, readable, mutant):
    """float32 mono sample of frames j (any integers): 0 outside [0, n_in); `readable` marks frames the kernel would load
    without looking at n_in (the mutant's over-read)."""
    ok = (j >= 0) & ((j < n_in) | readable)
    acc = np.zeros(j.shape, dtype=np.int64)
    acc[ok] = row[j[ok]].astype(np.int64).sum(axis=1)
    return acc.astype(np.float32) * _scale(n_ch, mutant)


def emul_resample(row, n_in, up, down, h32, out="f32", clip_out=None, mutant=None):
    """resample_kernel for one clip: row int16 [frames, n_ch] (frames >= n_in: what lies behind in_len is there to be
    over-read by a mutant).  Same chain: j from ja up to jb, k stepping down by `up`, y = fmaf(xs, h, y)."""
    n_ch = row.shape[1]
    half = (len(h32) - 1) // 2
    n_out = _n_out(n_in, up, down, clip_out, mutant)
    t = np.arange(n_out, dtype=np.int64) * down
    a, b = t - half, t + half
    ja = -((-a) // up)
    jb = b // up
    k0 = t + half - ja * up
    y = np.zeros(n_out, dtype=np.float32)
    for s in range(int((jb - ja).max()) + 1 if n_out else 0):
        j = ja + s
        act = j <= jb
        if mutant == "first tap dropped" and s == 0:
            continue
        if mutant == "last tap dropped":
            act = j < jb
        k = k0 - s * up
        if mutant == "tap index off by one":
            k = np.maximum(k - 1, 0)
        k = np.where(act, k, 0)
        readable = (j < row.shape[0]) if mutant == "samples past in_len read" else np.zeros(j.shape, dtype=bool)
        x = _xs(row, n_in, n_ch, np.where(act, j, -1), readable & act, mutant)
        y = np.where(act, _fma(x, h32[k], y), y)
    return _store(y, out, mutant)


def emul_decimate(row, n_in, down, h32, out="f32", clip_out=None, mutant=None, row_aligned=True):
    """decimate_kernel<down> for one clip: workgroups of 768 outputs stage their input span in groups of 8 frames from a
    multiple of 8 (one 16-byte load where the clip is mono, the row aligned and the group inside [0, n_in); frame by frame with
    a range check otherwise), then every output runs n = 0 .. NT - 1 over x[m down - half + n] with taps[NT - 1 - n]."""
    n_ch = row.shape[1]
    half, nt = 10 * down, 20 * down + 1
    assert len(h32) == nt
    n_out = _n_out(n_in, 1, down, clip_out, mutant)
    m = np.arange(n_out, dtype=np.int64)
    j_al = ((m // 768) * 768 * down - half) & ~np.int64(7)
    vec = n_ch == 1 and row_aligned
    y = np.zeros(n_out, dtype=np.float32)
    for n in range(nt):
        if (mutant == "first tap dropped" and n == 0) or (mutant == "last tap dropped" and n == nt - 1):
            continue
        j = m * down - half + n
        g = j_al + 8 * ((j - j_al) // 8)                 # first frame of the group of 8 that holds j
        if mutant == "samples past in_len read":         # the vector load taken for a group that only STARTS inside the clip
            readable = vec & (g >= 0) & (g < n_in) & (j < row.shape[0])
        else:
            readable = np.zeros(j.shape, dtype=bool)     # (g + 8 <= n_in: every frame of the group is inside anyway)
        k = nt - 1 - n - (mutant == "tap index off by one")
        y = _fma(_xs(row, n_in, n_ch, j, readable, mutant), np.full(n_out, h32[max(k, 0)], dtype=np.float32), y)
    return _store(y, out, mutant)


def emulate(case, row, n_in, out, mutant=None, u=0):
    """The kernel the library picks for `case` (svk_ingest_resample's own rule)."""
    h = case["h32"]
    if case["up"] == 1 and case["down"] in (2, 3) and len(h) == 20 * case["down"] + 1:
        aligned = (u * case["frames"] * row.shape[1]) % 8 == 0
        return emul_decimate(row, n_in, case["down"], h, out, mutant=mutant, row_aligned=aligned)
    return emul_resample(row, n_in, case["up"], case["down"], h, out, mutant=mutant)


# ---- cases --------------------------------------------------------------------------------------------------------------------
N_OUTS = (1, 2, 255, 256, 257, 767, 768, 769, 1537)
N_INS = (1, 2, 3, 7, 8, 9)


def lengths_for(up, down, extra=()):
    """Input lengths that give each n_out of N_OUTS (the shortest such clip; the nearest count where the ratio skips it), the
    short inputs of N_INS, and `extra`.  Several end inside a group of 8 frames."""
    lens = {(n - 1) * down // up + 1 for n in N_OUTS} | set(N_INS) | set(extra)
    return sorted(lens, reverse=True)


def _case(name, up, down, n_ch, residue=0, kind="random", taps=None, seed=0):
    lens = lengths_for(up, down)
    frames = max(lens) + 5
    frames += (residue - frames) % 8                  # the row width decides which rows start on a 16-byte boundary
    if kind != "random":
        lens = [frames - 3] * 3
    return {"name": name, "up": up, "down": down, "n_ch": n_ch, "frames": frames, "lengths": [frames] + lens if kind == "random" else lens,
            "kind": kind, "h32": taps32(up, down, taps), "seed": seed, "custom": taps is not None}


def cases():
    out = []
    for down in (3, 2):                               # decimate_kernel<3>, <2>
        for residue in (0, 1, 4):
            out.append(_case("1/%d mono, rows of 8 k + %d frames" % (down, residue), 1, down, 1, residue, seed=len(out)))
        for n_ch in (2, 3, 8):
            out.append(_case("1/%d, %d channels" % (down, n_ch), 1, down, n_ch, seed=len(out)))
    out.append(_case("1/6 mono (generic, up == 1)", 1, 6, 1, 1, seed=len(out)))
    out.append(_case("1/6, 2 channels", 1, 6, 2, seed=len(out)))
    for up, down, n_ch in ((160, 441, 1), (160, 441, 2), (320, 441, 1), (640, 441, 1), (2, 1, 1), (2, 1, 3), (1, 1, 1), (1, 1, 2)):
        out.append(_case("%d/%d, %d channel%s" % (up, down, n_ch, "s" * (n_ch > 1)), up, down, n_ch, 1, seed=len(out)))
    out.append(_case("1/3 mono, 31-tap design (generic kernel)", 1, 3, 1, 4, taps=custom_taps(), seed=len(out)))
    for up, down in ((1, 3), (1, 2), (160, 441), (2, 1)):
        out.append(_case("%d/%d mono, full scale: +32767, -32768, step" % (up, down), up, down, 1, 1, kind="full scale", seed=len(out)))
    return out


def make_input(case):
    """int16 [n_utt, frames, n_ch] (the mono cases are passed to the library as [n_utt, frames]) with full-scale garbage behind
    every clip's length."""
    rng = np.random.default_rng(100 + case["seed"])
    n_utt, frames, n_ch = len(case["lengths"]), case["frames"], case["n_ch"]
    if case["kind"] == "random":
        pcm = (rng.standard_normal((n_utt, frames, n_ch)) * 3000).clip(-32768, 32767).astype(np.int16)
        if (case["up"], case["down"]) == (1, 1):
            pcm[:, 5::97] = 0                          # zero samples: they come back as 0 only if the off-centre taps are exactly 0
    else:
        pcm = np.empty((n_utt, frames, n_ch), dtype=np.int16)
        pcm[0], pcm[1] = 32767, -32768
        pcm[2, :frames // 2], pcm[2, frames // 2:] = -32768, 32767
    for u, n in enumerate(case["lengths"]):
        pcm[u, n:] = np.array(GARBAGE, dtype=np.int16)[(np.arange(frames - n) % 2)][:, None]
    return pcm


_REFS = {}


def case_reference(case):
    """(pcm, [(y64, bar, n_m) per clip]) of a case, computed once and shared read-only."""
    if case["name"] not in _REFS:
        pcm = make_input(case)
        refs = [reference(pcm[u, :n], case["up"], case["down"], case["h32"]) for u, n in enumerate(case["lengths"])]
        pcm.setflags(write=False)
        for r in refs:
            for a in r:
                a.setflags(write=False)
        _REFS[case["name"]] = (pcm, refs)
    return _REFS[case["name"]]
