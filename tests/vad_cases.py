"""TEST INFRASTRUCTURE for tests/test_vad_paths.py: clips built from chosen per-frame flags, the flag families, Python
restatements of the two hysteresis walks of csrc/vad.hip with their mutants, and the case lists.

The VAD is integer arithmetic, so every comparison is exact.  The reference is oracle.vad_ref (framer, decision rule, the
deque walk of the collector); what is restated here is not a reference but the two ALGORITHMS the kernels use in its place:

  walk_sequential   vad_kernel's phase 2: 64 flags at a time as one ballot mask, the ring as (since, voiced_in_ring), the frame
                    that drops out of the ring read from this chunk's mask, the previous chunk's (`prev`) or the flag array;
  walk_scan         vad_walk_wave (vad_small_kernel, vad_walk_kernel): prefix sums of the flags, 64 frames tested for "does the
                    collector fire here" at once, the first lane that fires is the next event and the scan resumes behind it.

Both return what the edges of their own bookkeeping saw (events by lane, ring emissions that reach into earlier chunks, reads
past `prev`), so that the case list can be held to reaching them.
"""
import numpy as np

RINGS = (1, 2, 10, 33, 64, 65, 100, 129, 200)
FRAME_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1100)
FAMILIES = ("bernoulli 0.5", "bernoulli 0.93", "bernoulli 0.07", "ring-sized runs", "long runs, 3 % flipped", "lane edges",
            "slack before the event")
SENTINEL = -21846          # 0xAAAA: what the untouched parts of an output buffer hold


def ring_thresh(ring_len):
    """count > 0.9 * maxlen (vad.py:99,117) for an integer count: what Engine.vad_energy passes down."""
    return int(np.floor(0.9 * ring_len))


# ---- flags ------------------------------------------------------------------------------------------------------------------
def _runs(rng, nf, lo, hi, first):
    out = np.zeros(nf, dtype=bool)
    f, v = 0, first
    while f < nf:
        n = int(rng.integers(max(1, lo), max(1, hi) + 1))
        out[f:f + n] = v
        f, v = f + n, not v
    return out


def lane_edge_flags(nf, ring_len):
    """Triggers and releases placed on lanes 0 and 63 of vad_walk_wave's scan window.  After an event on frame e the scan
    resumes at s = e + 1 and moves on by 64 frames while nothing fires, so the frame s + 64 k + lane is on `lane`.  Idle, the
    collector fires on the frame that completes thresh + 1 voiced frames after silence; triggered, on the one that completes
    thresh + 1 unvoiced frames after speech.  One target in five is lane 20 of the same window, which puts the next event
    into the window that follows at once."""
    need = ring_thresh(ring_len) + 1
    flags = np.zeros(nf, dtype=bool)
    targets = ((0, 1), (63, 0), (63, 1), (0, 2), (20, 0))
    s, trig, i = 0, False, 0
    while True:
        lane, k = targets[i % len(targets)]
        i += 1
        e = s + 64 * k + lane
        while e - s + 1 < need:
            e += 64
        if e >= nf:
            break
        flags[s:e + 1 - need] = trig
        flags[e + 1 - need:e + 1] = not trig
        s, trig = e + 1, not trig
    flags[s:] = trig
    return flags


def slack_flags(nf, ring_len):
    """Events whose ring holds as many frames of the OTHER kind as the rule allows, right before the event, and the opposite run
    right behind it: need - 1 voiced, ring_len - need unvoiced, one voiced (the trigger, on a full ring), then the mirror image
    (the release).  A ring that is not cleared at an event still holds those frames, and fires the next event early."""
    need = ring_thresh(ring_len) + 1
    slack = ring_len - need
    period = np.array([1] * (need - 1) + [0] * slack + [1] + [0] * (need - 1) + [1] * slack + [0], dtype=bool)
    return np.tile(period, nf // len(period) + 1)[:nf]


def family_flags(family, nf, ring_len, rng):
    if family.startswith("bernoulli"):
        return rng.random(nf) < float(family.split()[1])
    if family == "ring-sized runs":
        return _runs(rng, nf, ring_thresh(ring_len) - 2, ring_len + 3, bool(rng.integers(2)))
    if family == "long runs, 3 % flipped":
        return _runs(rng, nf, 1, 3 * ring_len + 1, bool(rng.integers(2))) ^ (rng.random(nf) < 0.03)
    if family == "lane edges":
        return lane_edge_flags(nf, ring_len)
    if family == "slack before the event":
        return slack_flags(nf, ring_len)
    raise ValueError(family)


def hysteresis_cases():
    """(name, flags, ring_len): a covering set of ring x frame count x family (every pair of two of them occurs), the lane-edge
    family at a length that holds several of its events for every ring, and rings longer than the clip."""
    cases = []
    for i, ring in enumerate(RINGS + (300,)):
        for j, nf in enumerate(FRAME_COUNTS):
            for k in ((i + j) % len(FAMILIES), (2 * i + j + 3) % len(FAMILIES)):
                rng = np.random.default_rng(1000 * i + 10 * j + k)
                cases.append(("%s, ring %d, %d frames" % (FAMILIES[k], ring, nf), family_flags(FAMILIES[k], nf, ring, rng), ring))
        cases.append(("lane edges, ring %d, 2500 frames" % ring, lane_edge_flags(2500, ring), ring))
    for ring, nf in ((2500, 129), (70, 65), (1101, 1100)):          # the ring never fills
        rng = np.random.default_rng(ring)
        cases.append(("bernoulli 0.93, ring %d longer than %d frames" % (ring, nf), rng.random(nf) < 0.93, ring))
        cases.append(("all voiced, ring %d longer than %d frames" % (ring, nf), np.ones(nf, dtype=bool), ring))
    return cases


# ---- the two walks -----------------------------------------------------------------------------------------------------------
SEQ_MUTANTS = (">= for > when idle", ">= for > when triggered", "ring not cleared on trigger", "ring not cleared on release",
               "emitted ring short by one", "seg not advanced on release", "prev used beyond 64 frames back")
SCAN_MUTANTS = ("window f - ring_len", ">= for > when idle", ">= for > when triggered", "seg not advanced on release")


def walk_sequential(flags, ring_len, thresh, mutant=None):
    """vad_kernel, phase 2.  -> (keep, seg, stats)."""
    nf = len(flags)
    pos = np.full(nf, -1, dtype=np.int64)
    sego = np.full(nf, -1, dtype=np.int32)
    st = {"events_per_chunk": {}, "back_one_chunk": 0, "back_more_chunks": 0, "prev_reads": 0, "lds_reads": 0, "full_ring": 0}
    triggered = False
    since = voiced = kept = seg = 0
    prev = 0
    for f0 in range(0, nf, 64):
        cnt = min(64, nf - f0)
        m = 0
        for b in range(cnt):
            m |= int(bool(flags[f0 + b])) << b
        for b in range(cnt):
            f = f0 + b
            if since == ring_len:
                st["full_ring"] += 1
                o = b - ring_len
                if o >= 0:
                    voiced -= (m >> o) & 1
                elif o >= -64 or mutant == "prev used beyond 64 frames back":
                    voiced -= (prev >> ((64 + o) & 63)) & 1
                    st["prev_reads"] += 1
                else:
                    voiced -= int(bool(flags[f - ring_len]))
                    st["lds_reads"] += 1
            else:
                since += 1
            voiced += (m >> b) & 1
            if not triggered:
                if voiced > thresh or (mutant == ">= for > when idle" and voiced >= thresh):
                    triggered = True
                    first = f - since + 1 + (mutant == "emitted ring short by one")
                    for g in range(first, f + 1):
                        pos[g], sego[g] = kept, seg
                        kept += 1
                    st["back_one_chunk"] += first < f0
                    st["back_more_chunks"] += first < f0 - 64
                    if mutant != "ring not cleared on trigger":
                        since = voiced = 0
                    st["events_per_chunk"][f0] = st["events_per_chunk"].get(f0, 0) + 1
                    continue
            else:
                pos[f], sego[f] = kept, seg
                kept += 1
                if since - voiced > thresh or (mutant == ">= for > when triggered" and since - voiced >= thresh):
                    triggered = False
                    if mutant != "seg not advanced on release":
                        seg += 1
                    if mutant != "ring not cleared on release":
                        since = voiced = 0
                    st["events_per_chunk"][f0] = st["events_per_chunk"].get(f0, 0) + 1
        prev = m
    return pos >= 0, sego, st


def walk_scan(flags, ring_len, thresh, mutant=None):
    """vad_walk_wave.  -> (keep, seg, events): events = [(frame, lane of the scan window, "T" or "R")]."""
    nf = len(flags)
    P = np.concatenate([[0], np.cumsum(np.asarray(flags, dtype=np.int64))])
    segm = np.full(nf, -1, dtype=np.int32)
    back = 1 if mutant != "window f - ring_len" else 0
    events = []
    triggered = False
    s = seg = f0 = 0
    while f0 < nf:
        last = min(nf, f0 + 64) - 1
        f = np.arange(f0, last + 1)
        lo = np.maximum(s, f - ring_len + back)
        v = P[f + 1] - P[lo]
        if triggered:
            u = f - lo + 1 - v
            fire = (u >= thresh) if mutant == ">= for > when triggered" else (u > thresh)
        else:
            fire = (v >= thresh) if mutant == ">= for > when idle" else (v > thresh)
        if not fire.any():
            if triggered:
                segm[f0:last + 1] = seg
            f0 = last + 1
            continue
        e = f0 + int(np.argmax(fire))
        events.append((e, e - f0, "R" if triggered else "T"))
        if not triggered:
            segm[max(s, e - ring_len + back):e + 1] = seg
            triggered = True
        else:
            segm[f0:e + 1] = seg
            triggered = False
            if mutant != "seg not advanced on release":
                seg += 1
        s = f0 = e + 1
    return segm >= 0, segm, events


# ---- clips -------------------------------------------------------------------------------------------------------------------
def clip_from_flags(flags, frame_samples, threshold, rng, tail=None):
    """int16 samples whose frame f is above the rule sum(x^2) > threshold * n exactly when flags[f], with random signs.
    threshold = a^2.  Unvoiced frames: all |x| = a (equality: not voiced), or |x| drawn from [0, a].  Voiced frames: all
    |x| = a but one sample a + 1 (the least excess there is), or |x| drawn from [a + 1, 4 a].  `tail` (1 .. frame_samples, drawn
    if None) loud samples follow, so the strict framer `offset + n < len` yields exactly len(flags) frames."""
    n = int(frame_samples)
    a = int(round(np.sqrt(threshold)))
    assert a * a == threshold and 1 <= a and 4 * a + 1 <= 32767
    nf = len(flags)
    mag = np.empty((nf, n), dtype=np.int64)
    for f in range(nf):
        edge = rng.random() < 0.5
        if flags[f]:
            mag[f] = a if edge else rng.integers(a + 1, 4 * a + 1, n)
            if edge:
                mag[f, rng.integers(n)] = a + 1
        else:
            mag[f] = a if edge else rng.integers(0, a + 1, n)
    if tail is None:
        tail = int(rng.integers(1, n + 1))
    assert 1 <= tail <= n or nf == 0
    mag = np.concatenate([mag.reshape(-1), rng.integers(a + 1, 4 * a + 1, tail)])
    return (mag * rng.choice((-1, 1), mag.shape[0])).astype(np.int16)


# the families in the order a batch draws them: the two that seldom fire on a long ring come up once in nine
BATCH_FAMILIES = ("ring-sized runs", "bernoulli 0.93", "slack before the event", "long runs, 3 % flipped", "lane edges",
                  "bernoulli 0.5", "ring-sized runs", "long runs, 3 % flipped", "bernoulli 0.07")


def clips_for(frame_samples, ring_len, threshold, frame_counts, seed):
    """One clip per frame count, the families in turn, plus the lengths 0, frame_samples (no frame: the framer is strict) and
    frame_samples + 1 (one frame).  -> [(int16 clip, flags)]."""
    rng = np.random.default_rng(seed)
    out = []
    for i, nf in enumerate(frame_counts):
        flags = family_flags(BATCH_FAMILIES[(i + seed) % len(BATCH_FAMILIES)], nf, ring_len, rng)
        if nf == 0:
            out.append((clip_from_flags(flags, frame_samples, threshold, rng, tail=frame_samples), flags))   # len = frame_samples
            out.append((np.zeros(0, dtype=np.int16), flags))
        elif nf == 1:
            out.append((clip_from_flags(flags, frame_samples, threshold, rng, tail=1), flags))             # len = frame_samples + 1
        else:
            out.append((clip_from_flags(flags, frame_samples, threshold, rng), flags))
    return out
