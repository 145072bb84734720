"""TEST INFRASTRUCTURE for tests/test_vad_adaptive*.py: the level-adaptive VAD rule of include/svk.h ("level-adaptive energy VAD") restated in Python
integers, its mutants, and the case list the GPU tests run (the CPU tests hold the list to having teeth).

The rule (all integers): nf whole frames, E_f = sum(x^2) of frame f; rank(q) = (q (nf - 1)) >> 16; E_lo, E_hi = the
rank(floor_q16)-th and rank(peak_q16)-th smallest E_f; A = (E_lo above_floor_q16) >> 16, B = (E_hi below_peak_q16) >> 16;
T = max(min(A, B), min_threshold frame_samples); frame f is speech iff E_f > T.  nf == 0: the levels are
(0, 0, min_threshold frame_samples).  Energies come from int64 NumPy, the order statistics from `sorted`, the products are
Python ints (unbounded), and oracle.vad_ref.collect does the hysteresis.
"""
import collections

import numpy as np

import vad_cases as V
from oracle import vad_ref

Params = collections.namedtuple("Params", "floor_q16 peak_q16 above_floor_q16 below_peak_q16 min_threshold")

MUTANTS = ("rank + 1", "rank - 1", ">= for >", "max for min", "shift before multiply", "threshold without frame_samples",
           "32-bit products", "64-bit products")


def db_to_q16(db):
    """round(10^(dB / 10) 65536): the conversion AdaptiveEnergyVad uses, restated."""
    return int(round(10.0 ** (db / 10.0) * 65536.0))


def params(floor_quantile=0.10, peak_quantile=0.95, above_floor_db=10.0, below_peak_db=25.0, min_threshold=0):
    return Params(int(round(floor_quantile * 65536)), int(round(peak_quantile * 65536)), db_to_q16(above_floor_db),
                  db_to_q16(-below_peak_db), int(min_threshold))


DEFAULT = params()


def num_frames(n_samples, fsamp):
    """Frames the strict framer yields (vad.py:54, in bytes: offset + 2 fsamp < 2 n_samples)."""
    return (2 * n_samples - 1) // (2 * fsamp) if n_samples > 0 else 0


def energies(pcm, fsamp):
    """[nf] Python ints: sum of squares of every whole frame."""
    pcm = np.asarray(pcm, dtype=np.int16)
    nf = num_frames(len(pcm), fsamp)
    x = pcm[:nf * fsamp].astype(np.int64).reshape(nf, fsamp)
    return [int(e) for e in (x * x).sum(axis=1)]


def rank(q16, nf, mutant=None):
    r = (q16 * (nf - 1)) >> 16
    if mutant == "rank + 1":
        r = min(r + 1, nf - 1)
    if mutant == "rank - 1":
        r = max(r - 1, 0)
    return r


def levels(e, fsamp, p, mutant=None):
    """(E_lo, E_hi, T) of a clip's frame energies `e`."""
    floor = p.min_threshold * (1 if mutant == "threshold without frame_samples" else fsamp)
    if not e:
        return 0, 0, floor
    s = sorted(e)
    e_lo, e_hi = s[rank(p.floor_q16, len(e), mutant)], s[rank(p.peak_q16, len(e), mutant)]
    if mutant == "shift before multiply":
        a, b = (e_lo >> 16) * p.above_floor_q16, (e_hi >> 16) * p.below_peak_q16
    else:
        a, b = e_lo * p.above_floor_q16, e_hi * p.below_peak_q16
        if mutant == "32-bit products":
            a, b = a & 0xFFFFFFFF, b & 0xFFFFFFFF
        if mutant == "64-bit products":
            a, b = a & 0xFFFFFFFFFFFFFFFF, b & 0xFFFFFFFFFFFFFFFF
        a, b = a >> 16, b >> 16
    m = max(a, b) if mutant == "max for min" else min(a, b)
    return e_lo, e_hi, max(m, floor)


def vad(pcm, fsamp, ring_len, p, mutant=None):
    """One clip -> dict(levels (3 ints), energy [nf] ints, flags, keep, seg, voiced int16, src_frame)."""
    pcm = np.asarray(pcm, dtype=np.int16)
    e = energies(pcm, fsamp)
    lv = levels(e, fsamp, p, mutant)
    if mutant == ">= for >":
        flags = np.array([x >= lv[2] for x in e], dtype=bool)
    else:
        flags = np.array([x > lv[2] for x in e], dtype=bool)
    keep, seg = vad_ref.collect(flags, 1, ring_len)
    kept = np.nonzero(keep)[0]
    voiced = np.concatenate([pcm[f * fsamp:(f + 1) * fsamp] for f in kept]) if len(kept) else np.zeros(0, dtype=np.int16)
    return {"levels": lv, "energy": e, "flags": flags, "keep": keep, "seg": seg, "voiced": voiced, "src_frame": kept}


def same(a, b):
    return (a["levels"] == b["levels"] and np.array_equal(a["keep"], b["keep"]) and np.array_equal(a["seg"], b["seg"]))


# ---- clips -------------------------------------------------------------------------------------------------------------------
FAMILIES = ("speechlike", "equal", "silence", "full scale", "low byte", "above bit 32", "equality")
EQ_V = 37                       # the equality construction's quiet sample: E_lo = v^2, T = (2 v)^2 under EQUALITY


def _tail(rng, fsamp, tail):
    n = int(rng.integers(1, fsamp + 1)) if tail is None else tail
    return rng.integers(20000, 30000, n)            # loud: a rule that read the partial frame would count it


def family_clip(family, nf, fsamp, ring_len, rng, tail=None):
    """nf whole frames of `family` and a loud partial frame of `tail` samples (1 .. fsamp, drawn if None)."""
    x = np.zeros((nf, fsamp), dtype=np.int64)
    if family == "speechlike":            # loud and quiet runs around the ring's length, every frame at its own level
        flags = V.family_flags("ring-sized runs" if nf % 2 else "long runs, 3 % flipped", nf, ring_len, rng)
        for f in range(nf):
            amp = int(rng.integers(500, 20000)) if flags[f] else int(rng.integers(1, 50))
            x[f] = rng.integers(-amp, amp + 1, fsamp)
    elif family == "equal":               # ties at both ranks
        x[:] = rng.integers(-3000, 3001, fsamp)[None, :]
    elif family == "full scale":          # the largest energy there is: 2^30 fsamp
        x[:] = -32768
    elif family == "low byte":            # single-sample frames 1 .. 15: the energies differ in the lowest byte only
        for f in range(nf):
            x[f, rng.integers(fsamp)] = (1 + (f * 7) % 15) * int(rng.choice((-1, 1)))
    elif family == "above bit 32":        # 4 m samples of -32768: E = m 2^32
        for f in range(nf):
            m = 1 + (f * 5) % max(1, fsamp // 4)
            x[f, rng.permutation(fsamp)[:min(fsamp, 4 * m)]] = -32768
    elif family == "equality":            # under EQUALITY: a frame exactly at T = (2 v)^2, one at T + 1, loud ones above
        assert nf >= 8 and fsamp >= 2
        kinds = ["quiet"] * (nf // 2) + ["at"] + ["above"] + ["loud"] * (nf - nf // 2 - 2)
        for f, k in enumerate(rng.permutation(kinds)):
            if k == "loud":
                x[f] = rng.integers(5000, 20000, fsamp) * rng.choice((-1, 1), fsamp)
            else:
                i, j = rng.permutation(fsamp)[:2]
                x[f, i] = {"quiet": EQ_V, "at": 2 * EQ_V, "above": -2 * EQ_V}[k]
                if k == "above":
                    x[f, j] = 1
    elif family != "silence":
        raise ValueError(family)
    return np.concatenate([x.reshape(-1), _tail(rng, fsamp, tail)]).astype(np.int16)


# the parameter sets of the case list
EQUALITY = Params(6554, 62259, 4 * 65536, 65536, 0)             # T = 4 E_lo while the peak is loud
ONE_RANK = Params(32768, 32768, 2 * 65536, 65536, 0)            # floor_q16 == peak_q16: T = the median energy
TOP_RANK = Params(0, 65536, 1 << 40, db_to_q16(-10.0), 0)       # peak_q16 = 65536 (the maximum) and the largest ratio: A >= 2^64 on loud clips
WITH_FLOOR = Params(6554, 62259, db_to_q16(10.0), db_to_q16(-25.0), 1500)   # the absolute floor binds on the quiet clips
ABSOLUTE = Params(6554, 62259, db_to_q16(10.0), 0, 40000)       # below_peak_q16 = 0: the absolute rule

COUNTS = (1, 2, 64, 65, 130, 8, 33)
Case = collections.namedtuple("Case", "name route fsamp ring params clips")


def _clips(fsamp, ring, counts, seed, families=FAMILIES):
    """The lengths 0, fsamp (no frame) and fsamp + 1 (one frame), every family at two of the frame counts (the equality
    construction where it fits), and the speechlike family at all of them."""
    rng = np.random.default_rng(seed)
    out = [np.zeros(0, dtype=np.int16), family_clip("silence", 0, fsamp, ring, rng, tail=fsamp),
           family_clip("speechlike", 1, fsamp, ring, rng, tail=1)]
    for i, fam in enumerate(families):
        for nf in (counts[i % len(counts)], counts[(i + 3) % len(counts)]):
            if fam == "equality":
                nf = max(nf, 8 + i)
                if fsamp < 2:
                    continue
            out.append(family_clip(fam, nf, fsamp, ring, rng))
    for nf in counts:
        out.append(family_clip("speechlike", nf, fsamp, ring, rng))
    return out


_CASES = []


def gpu_cases():
    """What tests/test_vad_adaptive.py runs: (name, SVK_VAD_SPLIT or None, frame_samples, ring, params, clips).  Built once."""
    if _CASES:
        return _CASES

    def add(route, fsamp, ring, p, pname, counts=COUNTS, families=FAMILIES):
        name = "split=%s-fs%d-ring%d-%s-max%d" % (route, fsamp, ring, pname, max(counts))
        clips = _clips(fsamp, ring, counts, seed=len(_CASES) + 1, families=families)
        for c in clips:
            c.setflags(write=False)
        _CASES.append(Case(name, route, fsamp, ring, p, clips))

    # the short-clip kernel (the library's own choice up to 512 frames)
    add(None, 160, 10, DEFAULT, "default")
    add(None, 480, 1, EQUALITY, "equality")
    add(None, 8, 100, ONE_RANK, "one-rank", counts=COUNTS + (512,))
    add(None, 160, 10, TOP_RANK, "top-rank")
    add(None, 160, 100, WITH_FLOOR, "floor")
    add(None, 160, 10, ABSOLUTE, "absolute")
    # the long-clip kernels: forced onto short clips, and chosen by the library beyond 512 frames
    add("1", 160, 10, DEFAULT, "default", counts=COUNTS + (513, 700))
    add("1", 8, 100, EQUALITY, "equality", counts=COUNTS + (600,))
    add("1", 480, 1, TOP_RANK, "top-rank", counts=(1, 2, 64, 65, 130, 513))
    add("1", 8, 10, ONE_RANK, "one-rank", counts=COUNTS + (650,))
    add("1", 160, 10, ABSOLUTE, "absolute")
    add(None, 8, 10, WITH_FLOOR, "floor", counts=COUNTS + (700,))
    add("1", 8, 100, DEFAULT, "default", counts=(8192,), families=("equal", "low byte"))
    # the general route
    add("2", 160, 10, DEFAULT, "default")
    add("2", 100, 100, EQUALITY, "equality")
    add("2", 7, 1, ONE_RANK, "one-rank")
    add("2", 1323, 10, TOP_RANK, "top-rank", counts=(1, 2, 64, 65, 130))
    add("2", 65536, 1, DEFAULT, "default", counts=(5,), families=("full scale",))
    add("2", 65536, 1, TOP_RANK, "top-rank", counts=(5,), families=("full scale",))
    add(None, 100, 10, ABSOLUTE, "absolute")
    add("2", 7, 10, WITH_FLOOR, "floor", counts=COUNTS + (513,))
    return _CASES


_REF = {}


def reference(case, mutant=None):
    """[vad(clip)] of a case's clips; the unmutated one is computed once and shared."""
    if mutant is not None:
        return [vad(c, case.fsamp, case.ring, case.params, mutant) for c in case.clips]
    if case.name not in _REF:
        _REF[case.name] = [vad(c, case.fsamp, case.ring, case.params) for c in case.clips]
    return _REF[case.name]
