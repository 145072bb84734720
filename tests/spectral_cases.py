"""The inputs of tests/test_spectral_embed.py, built here so that tests/test_spectral_host.py can hold every one of them to the
margin conditions on the CPU before a GPU ever sees it.  One padded batch per kind; the node counts are the sizes at which
svk_spectral_embed can go wrong: empty, one node, the smallest graphs, around a wave, odd counts (the round-robin pads them)
and the limit."""
import numpy as np

import ahc_f64_ref
import spectral_f64_ref as ref

NODE_COUNTS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128]
STRIDE = 128
SWEEP = (2, 32, 2)
MARGIN = 1e-9
# speakers of the "blocks" recording with that many nodes: 1 - 6, every count at least once
BLOCK_SPEAKERS = {0: 0, 1: 1, 2: 1, 3: 1, 15: 2, 16: 3, 17: 2, 63: 4, 64: 5, 65: 3, 127: 6, 128: 4}
BLOCKS_SEED = 11
# a target per recording of the block batch (0: not set), and the bounds the decision tests run under.  A count that is forced on
# a recording must not cut through equal eigenvalues (K3 has 0, 3, 3: two vectors of it span no space of their own; a graph
# of three components has three zeros) -- margin_cut, asserted in tests/test_spectral_host.py
TARGET = np.array([0, 0, 1, 1, 2, 0, 3, 4, 0, 5, 6, 5], np.int32)
BOUNDS = {"free": dict(), "min3": dict(min_speakers=3), "max2": dict(max_speakers=2), "target": dict(target=TARGET),
          "target_min3": dict(target=TARGET, min_speakers=3)}
GROUPED_STRIDE, GROUPED_NODES = 300, 128
GROUPED_WINDOWS = [0, 1, 2, 3, 40, 127, 128, 129, 200, 250, 299, 300]


def ties_matrix(rng, n):
    """Multiples of 1/8: most rows choose their neighbours among equals."""
    a = np.triu(rng.integers(-8, 9, (n, n)) / 8.0, 1)
    return (a + a.T).astype(np.float32)


def block_matrix(rng, n, speakers, sigma=0.12):
    """Within a speaker 0.6, across 0.1, Gaussian noise; speaker s owns the windows with i % speakers == s."""
    who = np.arange(n) % max(speakers, 1)
    a = np.where(who[:, None] == who[None, :], 0.6, 0.1) + rng.normal(0.0, sigma, (n, n))
    a = np.triu(a, 1)
    return (a + a.T).astype(np.float32), who.astype(np.int32)


def pad(mats, stride, below=0.0):
    """Square matrices -> one padded batch; the part below the diagonal and the dead rows hold `below` when it is not 0."""
    aff = np.full((len(mats), stride, stride), below, np.float32)
    for r, m in enumerate(mats):
        n = m.shape[0]
        if below == 0.0:
            aff[r, :n, :n] = m
        else:
            iu = np.triu_indices(n, 1)
            aff[r][iu] = m[iu]
    return aff, np.array([m.shape[0] for m in mats], np.int32)


def ties_batch(below=0.0):
    rng = np.random.default_rng(3)
    return pad([ties_matrix(rng, n) for n in NODE_COUNTS], STRIDE, below)


def blocks_batch(below=0.0):
    """-> (aff, n_seg, the speaker of every window as a list of int32 arrays)."""
    rng = np.random.default_rng(BLOCKS_SEED)
    pairs = [block_matrix(rng, n, BLOCK_SPEAKERS[n]) for n in NODE_COUNTS]
    aff, n_seg = pad([p[0] for p in pairs], STRIDE, below)
    return aff, n_seg, [p[1] for p in pairs]


def tight_batch():
    """Two speakers whose windows all but coincide (cosines near 1 inside a speaker), 24 - 35 windows: the larger candidates
    of the sweep give nearly complete graphs, whose spectra are heaps of equal eigenvalues -- where a Jacobi iteration that
    converges at all converges slowest.  -> (aff, n_seg)."""
    rng = np.random.default_rng(0)
    mats = []
    for r, n in enumerate(range(24, 36)):
        who = np.sort(rng.integers(0, 2, n)) if r % 2 else (np.arange(n) // 4) % 2
        rows = rng.normal(size=(2, 16))[who] + 0.08 * rng.normal(size=(n, 16))
        mats.append(ref.cosine_affinity(rows))
    return pad(mats, 36)


def grouped_ties_batch():
    """Ties at a window stride of 300, reduced to at most 128 nodes by the AHC definition -> (aff, n_seg, group)."""
    rng = np.random.default_rng(4)
    aff, n_seg = pad([ties_matrix(rng, n) for n in GROUPED_WINDOWS], GROUPED_STRIDE)
    group = np.stack([ahc_f64_ref.ahc(aff[r], n_seg[r], max_clusters=GROUPED_NODES)[0] for r in range(len(n_seg))])
    return aff, n_seg, group


def known_spectra():
    """[(name, affinity [m, m], fixed p, the exact spectrum ascending)]: unions of equal complete graphs and cycles."""
    out = []
    for s, count in ((2, 1), (3, 1), (5, 3), (4, 4), (17, 1), (9, 7), (8, 8), (13, 5), (127, 1), (16, 8)):
        out.append(("%d x K%d" % (count, s), ref.complete_union_affinity(s, count), s - 1, ref.complete_union_spectrum(s, count)))
    for m in (127, 128):
        out.append(("%d-cycle" % m, ref.cycle_affinity(m), 2, ref.cycle_spectrum(m)))
    return out


def reference_batch(aff, n_seg, group=None, node_stride=None, target=None, **kw):
    return [ref.spectral(aff[r], n_seg[r], None if group is None else group[r], node_stride,
                         target=None if target is None else target[r], **kw) for r in range(len(n_seg))]
