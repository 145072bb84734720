"""The reference for the ROC convex hull (include/svk.h, "the ROC convex hull") in Python integers and Fractions, and the case list the GPU tests
run.  Nothing here imports the package: the chain, the pool-adjacent-violators pass and the derived values are restated from the
header's definitions, so that tests/test_rocch*.py compare two independent statements of one object."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

OPS = ((0.01, 1, 1), (0.05, 1, 1), (0.5, 1, 1), (0.001, 10, 1))


# ---- the definitions ---------------------------------------------------------------------------------------------------------
def roc_points(labels, scores, pool_ties=True, origin=True):
    """-> (points [(f, t)], scores [float32 | None]): the origin, then one point per distinct score, descending (a stable sort:
    the order among equal scores changes no pooled point); -0.0 equals +0.0.  The score of a point is the tie group's value
    with -0.0 read as +0.0.  pool_ties / origin = False are the mutants of tests/test_rocch_host.py."""
    labels, scores = np.asarray(labels).reshape(-1), np.asarray(scores, dtype=np.float32).reshape(-1)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    lab, sc = (labels[order] != 0), scores[order] + np.float32(0.0)      # (-0.0 + 0.0 = +0.0)
    pts, vals = ([(0, 0)], [None]) if origin else ([], [])
    f = t = 0
    for i in range(lab.size):
        t += int(lab[i])
        f += int(not lab[i])
        if not pool_ties or i + 1 == lab.size or sc[i + 1] != sc[i]:
            pts.append((f, t))
            vals.append(sc[i])
    return pts, vals


def cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def hull_chain(points, pop_collinear=True):
    """Andrew's monotone chain, popping while cross >= 0 (pop_collinear=False: > 0, a mutant) -> indices of the vertices."""
    keep = []
    for i, p in enumerate(points):
        while len(keep) >= 2 and (cross(points[keep[-2]], points[keep[-1]], p) >= 0 if pop_collinear
                                  else cross(points[keep[-2]], points[keep[-1]], p) > 0):
            keep.pop()
        keep.append(i)
    return keep


def bridge(points, A, B, right_strict=False, bisect=True):
    """The merge predicate of include/svk.h ("the ROC convex hull", merge levels) on two adjacent hulls given as index lists: every candidate u is tried, and
    exactly one must qualify.  v(u) is found as the kernel's hull_bridge_at finds it, by bisection -- which is right only if the
    predicate is monotone along B -- or (bisect=False) as the definition states it, by the first i from the left; the host test
    holds the two to each other.  right_strict=True is the mutant '> 0 in the bridge's right test'."""
    found = []
    for u in range(len(A)):
        a = points[A[u]]
        if bisect:
            lo, hi = 0, len(B) - 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if cross(a, points[B[mid]], points[B[mid + 1]]) < 0:
                    hi = mid
                else:
                    lo = mid + 1
            v = lo
        else:
            v = next((i for i in range(len(B) - 1) if cross(a, points[B[i]], points[B[i + 1]]) < 0), len(B) - 1)
        b = points[B[v]]
        left = u == 0 or cross(points[A[u - 1]], a, b) < 0
        c = 0 if u == len(A) - 1 else cross(a, points[A[u + 1]], b)
        right = u == len(A) - 1 or (c > 0 if right_strict else c >= 0)
        if left and right:
            found.append((u, v))
    assert len(found) == 1 or right_strict, "the bridge is not unique: %s" % found
    return found[0] if found else (len(A) - 1, 0)


def hull_merge(points, leaf, right_strict=False, bisect=True):
    """The device's divide and conquer: the chain over leaves of `leaf` consecutive points, then pairwise merges of adjacent
    hulls by `bridge` until one is left (an odd last hull is carried up unchanged)."""
    hulls = []
    for lo in range(0, len(points), leaf):
        idx = list(range(lo, min(lo + leaf, len(points))))
        hulls.append([idx[k] for k in hull_chain([points[i] for i in idx])])
    while len(hulls) > 1:
        nxt = []
        for p in range(0, len(hulls), 2):
            if p + 1 == len(hulls):
                nxt.append(hulls[p])
                continue
            A, B = hulls[p], hulls[p + 1]
            u, v = bridge(points, A, B, right_strict, bisect)
            nxt.append(A[:u + 1] + B[v:])
        hulls = nxt
    return hulls[0]


def pav_pool(points):
    """Pool adjacent violators over the tie groups, an independent statement of the same object: isotonic regression of the
    labels on the scores.  Walking down the scores the target fraction of a block may only fall; a block whose exact mean
    (a Fraction) is >= the one above it is merged into it.  -> the blocks' end indices into `points` (the origin leads)."""
    blocks = []                                                         # [dt, df, end index]
    for j in range(1, len(points)):
        blocks.append([points[j][1] - points[j - 1][1], points[j][0] - points[j - 1][0], j])
        while len(blocks) >= 2:
            (t0, f0, _), (t1, f1, e1) = blocks[-2], blocks[-1]
            if Fraction(t1, t1 + f1) >= Fraction(t0, t0 + f0):
                blocks[-2:] = [[t0 + t1, f0 + f1, e1]]
            else:
                break
    return [0] + [b[2] for b in blocks]


def min_cllr(vertices):
    """float64 via math.fsum; the arguments of log1p are exact rationals rounded once."""
    N, P = vertices[-1]
    tar, non = [], []
    for (f0, t0), (f1, t1) in zip(vertices[:-1], vertices[1:]):
        df, dt = f1 - f0, t1 - t0
        if df and dt:
            tar.append(dt * math.log1p(float(Fraction(df * P, dt * N))))
            non.append(df * math.log1p(float(Fraction(dt * N, df * P))))
    return (math.fsum(tar) / P + math.fsum(non) / N) / (2.0 * math.log(2.0))


def rocch_eer(vertices):
    """The rational value of roc_points_kernel's rule on the hull's vertices."""
    N, P = vertices[-1]
    for (f0, t0), (f1, t1) in zip(vertices[:-1], vertices[1:]):
        g0, g1 = 1 - Fraction(f0, N) - Fraction(t0, P), 1 - Fraction(f1, N) - Fraction(t1, P)
        if g0 > 0 >= g1:
            return Fraction(f0, N) + (Fraction(f1, N) - Fraction(f0, N)) * g0 / (g0 - g1)
    raise AssertionError("no edge crosses the diagonal")


def edge_llr(dt, df, P, N):
    return math.inf if df == 0 else -math.inf if dt == 0 else math.log(dt) - math.log(df) - (math.log(P) - math.log(N))


def pav_table(labels, scores, laplace=False):
    """-> (edges, llr) float32 by `pav_pool`.  laplace: the pool runs on the AUGMENTED sequence -- a non-target, then a target
    above the best score, a non-target, then a target below the worst --; bins without a real trial are dropped, and a bin
    that ends among the dummies has the lowest real score as its edge."""
    pts, vals = roc_points(labels, scores)
    N, P = pts[-1]
    if not laplace:
        ends = pav_pool(pts)
        return (np.array([vals[e] for e in ends[1:]], np.float32),
                np.array([edge_llr(pts[b][1] - pts[a][1], pts[b][0] - pts[a][0], P, N) for a, b in zip(ends[:-1], ends[1:])],
                         np.float32))
    aug = [(0, 0), (1, 0), (1, 1)] + [(f + 1, t + 1) for f, t in pts[1:]] + [(N + 2, P + 1), (N + 2, P + 2)]
    ends = pav_pool(aug)
    edges, llr = [], []
    for a, b in zip(ends[:-1], ends[1:]):
        first_real, last_real = max(a + 1, 3), min(b, len(pts) + 1)     # aug[3 .. len(pts) + 1] are the real tie groups
        if first_real > last_real:
            continue
        edges.append(vals[last_real - 2])
        llr.append(edge_llr(aug[b][1] - aug[a][1], aug[b][0] - aug[a][0], P, N))
    return np.array(edges, np.float32), np.array(llr, np.float32)


def pav_map(s, edges):
    """The bin of score s: the smallest k with s >= edges[k], the last bin below every edge; None for a NaN."""
    if s != s:
        return None
    for k, e in enumerate(edges):
        if s >= e:
            return k
    return len(edges) - 1


def pav_apply(scores, edges, llr):
    """The bits svk_pav_apply must give: uint32 [n].  `pav_map` for every score by counting, not searching: with descending
    edges the smallest k with s >= edges[k] is the number of edges above s."""
    scores, edges, llr = np.asarray(scores, np.float32), np.asarray(edges, np.float32), np.asarray(llr, np.float32)
    k = np.minimum((edges[None, :] > scores[:, None]).sum(axis=1), edges.size - 1)
    return np.where(np.isnan(scores), scores.view(np.uint32), llr[k].view(np.uint32))


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _descending(n):
    """n strictly descending float32 scores, exact: (n - i) / 8 - 300."""
    return ((n - np.arange(n)) / 8.0 - 300.0).astype(np.float32)


def _shuffled(lab, sc, seed):
    order = np.random.default_rng(seed).permutation(lab.size)
    return np.ascontiguousarray(lab[order]), np.ascontiguousarray(sc[order])


def farey_case(R):
    """One tie group per coprime (df, dt), 0 <= df, dt <= R, steepest first: every point of the ROC is a hull vertex."""
    vecs = [(df, dt) for df in range(R + 1) for dt in range(R + 1) if math.gcd(df, dt) == 1]
    vecs.sort(key=lambda v: (Fraction(v[0], v[0] + v[1])))            # the non-target share rises: the slope falls
    sc = _descending(len(vecs))
    lab = np.concatenate([np.r_[np.zeros(df, np.uint8), np.ones(dt, np.uint8)] for df, dt in vecs])
    return lab, np.concatenate([np.full(df + dt, sc[g], np.float32) for g, (df, dt) in enumerate(vecs)])


def distinct_case(m, seed):
    """m distinct scores, one trial each (the ROC has m + 1 points with the origin), overlapping classes."""
    rng = np.random.default_rng(seed)
    lab = (rng.random(m) < 0.4 + 0.4 * np.linspace(1, -1, m) ** 3).astype(np.uint8)
    lab[5], lab[m - 6] = 0, 1
    return lab, _descending(m)


@lru_cache(maxsize=None)
def gpu_cases():
    """name -> (labels uint8, scores float32), read-only, stored shuffled unless the construction says otherwise."""
    import test_roc_dcf as T                                            # (tests/ is on sys.path)
    cases = {k: T.CASES[k] for k in ("n2", "n3", "all_equal", "n5000_16_levels", "signed_zeros", "dyadic")}
    lab = np.r_[np.ones(40, np.uint8), np.zeros(60, np.uint8)]
    cases["separated"] = _shuffled(lab, _descending(100), 1)
    cases["inverted"] = _shuffled(1 - lab, _descending(100), 2)
    for m in (2046, 2047, 2048, 4096):
        cases["points_%d" % (m + 1)] = _shuffled(*distinct_case(m, m), seed=m)
    cases["n300000"] = T.CASES["n300000"]
    lab = np.r_[np.ones(200, np.uint8), np.zeros(3000, np.uint8), (np.arange(4000) % 3 == 0).astype(np.uint8)]
    cases["flat_then_arc"] = _shuffled(lab, _descending(7200), 3)
    cases["farey_72"] = _shuffled(*farey_case(72), seed=4)
    cases["farey_8"] = _shuffled(*farey_case(8), seed=5)
    for lab, sc in cases.values():
        lab.setflags(write=False)
        sc.setflags(write=False)
    return cases


@lru_cache(maxsize=None)
def reference(name):
    """-> (points, point scores, vertex indices) of a case, computed once."""
    lab, sc = gpu_cases()[name]
    pts, vals = roc_points(lab, sc)
    return pts, vals, hull_chain(pts)
