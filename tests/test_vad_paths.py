"""svk_vad_energy against oracle.vad_ref on every kernel route, frame geometry, placement and ring (tests/vad_cases.py: clips
built from chosen flags, the flag families, Python restatements of the kernels' two hysteresis walks and their mutants).

Everything here is integer arithmetic: all comparisons are exact.

CPU (default pass):
  * clip_from_flags yields the flags it was given under the oracle's rule, with frames exactly AT sum(x^2) == threshold * n
    (unvoiced) and one step above it (voiced), and the strict framer counts len(flags) frames;
  * the restatements of vad_kernel's sequential walk and of vad_walk_wave's event scan equal vad_ref.collect on the case list,
    and the list reaches the edges of their bookkeeping (the counts are asserted);
  * every mutant of the walks differs from the oracle on some case of the list: the list has teeth.
GPU (-m gpu): vad_small_kernel, the split trio and vad_kernel (both of its frame loops), each with keep, seg, n_vad_frames,
voiced_len, voiced[:voiced_len] and src_frame equal to the oracle's and nothing written outside a clip's own slot.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import vad_cases as V                  # noqa: E402  (tests/ is on sys.path, as for test_c3d2_float64)
from oracle import vad_ref             # noqa: E402

_ORACLE = {}


def oracle_walk(name, flags, ring):
    """vad_ref.collect of one hysteresis case, computed once."""
    if name not in _ORACLE:
        keep, seg = vad_ref.collect(flags, 1, ring)
        _ORACLE[name] = (keep, seg)
    return _ORACLE[name]


CASES = V.hysteresis_cases()


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fsamp,a", [(480, 500), (8, 3), (7, 3), (1, 2), (100, 500), (1323, 500)])
def test_clips_sit_where_the_flags_say(fsamp, a):
    """The oracle's rule on clip_from_flags' samples returns the flags; equality frames and least-excess frames occur; the
    framer yields len(flags) frames for every tail 1 .. frame_samples; the lengths 0, frame_samples and frame_samples + 1."""
    rng = np.random.default_rng(fsamp)
    flags = rng.random(200) < 0.5
    thr = a * a
    clip = V.clip_from_flags(flags, fsamp, thr, rng)
    np.testing.assert_array_equal(vad_ref.frame_flags(clip, 1000, fsamp, thr), flags)
    fr = clip[:200 * fsamp].reshape(200, fsamp).astype(np.int64)
    e = (fr * fr).sum(axis=1)
    assert np.any(e[~flags] == thr * fsamp) and np.any(e[flags] == thr * fsamp + 2 * a + 1)
    assert np.any(fr < 0) and np.any(fr > 0)
    for tail in {1, fsamp}:
        c = V.clip_from_flags(flags[:5], fsamp, thr, rng, tail=tail)
        assert len(c) == 5 * fsamp + tail and vad_ref.num_frames(2 * len(c), 1000, fsamp) == 5
    lens = sorted(len(c) for c, _ in V.clips_for(fsamp, 10, thr, (0, 1), 0))
    assert lens == [0, fsamp, fsamp + 1]
    assert [vad_ref.num_frames(2 * n, 1000, fsamp) for n in lens] == [0, 0, 1]


def test_both_walks_equal_the_oracle_and_the_cases_reach_the_edges():
    """Both restatements against vad_ref.collect on every case.  The counts at the end are what keeps the case list from
    silently losing an edge."""
    lanes = {(k, lane): 0 for k in "TR" for lane in (0, 63)}
    n_events = close_pairs = chunks_with_two = back_one = back_more = prev_reads = lds_reads = never_full = 0
    for name, flags, ring in CASES:
        th = V.ring_thresh(ring)
        keep, seg = oracle_walk(name, flags, ring)
        k1, s1, st = V.walk_sequential(flags, ring, th)
        k2, s2, events = V.walk_scan(flags, ring, th)
        np.testing.assert_array_equal(k1, keep, err_msg="sequential walk: " + name)
        np.testing.assert_array_equal(s1, seg, err_msg="sequential walk: " + name)
        np.testing.assert_array_equal(k2, keep, err_msg="event scan: " + name)
        np.testing.assert_array_equal(s2, seg, err_msg="event scan: " + name)
        n_events += len(events)
        for e, lane, kind in events:
            if (kind, lane) in lanes:
                lanes[(kind, lane)] += 1
        close_pairs += sum(1 for x, y in zip(events, events[1:]) if y[0] - x[0] <= 64)
        chunks_with_two += sum(1 for n in st["events_per_chunk"].values() if n >= 2)
        back_one += st["back_one_chunk"]
        back_more += st["back_more_chunks"]
        prev_reads += st["prev_reads"]
        lds_reads += st["lds_reads"]
        never_full += len(flags) > 0 and st["full_ring"] == 0 and ring > len(flags)
    print("VAD cases: %d, events %d, by lane %s, pairs within one window %d, chunks with >= 2 events %d, ring emissions reaching "
          "back one chunk %d / more %d, drops read from prev %d / from the flag array %d, rings longer than the clip %d"
          % (len(CASES), n_events, lanes, close_pairs, chunks_with_two, back_one, back_more, prev_reads, lds_reads, never_full))
    assert all(n >= 10 for n in lanes.values()), lanes
    assert close_pairs >= 100 and chunks_with_two >= 100
    assert back_one >= 10 and back_more >= 10
    assert prev_reads >= 1000 and lds_reads >= 1000
    assert never_full >= 4


def test_gpu_batches_keep_frames_and_hold_several_segments():
    """What the ring sweep feeds the GPU (its two batches per ring taken together): for every ring that a clip here can fill,
    several clips keep frames, one keeps only a part of its frames, and one holds more than one segment, so the compaction
    copies and the seg output have something to get wrong.  (A ring of 3000 frames never fills: nothing is kept, by the rule.)"""
    for ring in ALL_RINGS:
        items = batch(160, ring, UP_TO_512, seed=160 + ring) + batch(8, ring, V.FRAME_COUNTS, seed=8 + ring)
        kept = [int(k.sum()) for _, k, _, _ in items]
        if ring == 3000:
            assert not any(kept)
            continue
        assert sum(1 for n in kept if n) >= 4, (ring, kept)
        assert any(0 < n < len(k) for n, (_, k, _, _) in zip(kept, items)), (ring, kept)
        assert max(int(s.max()) for _, _, s, _ in items if len(s)) >= 1, ring


@pytest.mark.parametrize("walk,mutant", [("sequential", m) for m in V.SEQ_MUTANTS] + [("scan", m) for m in V.SCAN_MUTANTS])
def test_every_mutant_walk_differs_from_the_oracle(walk, mutant):
    """A wrong comparison, a ring that is not cleared, an emitted ring short by one, a window off by one, a
    segment counter that stands still and a `prev` mask read past its 64 frames are each seen by some case of the list."""
    fn = V.walk_sequential if walk == "sequential" else V.walk_scan
    caught = []
    for name, flags, ring in CASES:
        keep, seg = oracle_walk(name, flags, ring)
        k, s, _ = fn(flags, ring, V.ring_thresh(ring), mutant)
        if not (np.array_equal(k, keep) and np.array_equal(s, seg)):
            caught.append(name)
            if len(caught) == 3:
                break
    print("MUTANT %s walk, %s: caught by %s" % (walk, mutant, caught))
    assert caught, (walk, mutant)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu

USUAL = (480, 160, 8, 512)                         # a frame = one 16-byte vector per lane: small kernel, split trio, one_vec
UNUSUAL = (520, 1440, 1323, 661, 100, 7, 1)        # vad_kernel's per-frame loop whatever is forced
UP_TO_512 = tuple(n for n in V.FRAME_COUNTS if n <= 512)
UP_TO_513 = UP_TO_512 + (513,)
SHORT_LIST = (0, 1, 31, 33, 64, 65, 127, 129, 512, 513)
ALL_RINGS = V.RINGS + (3000,)                      # 3000: longer than every clip here
SKEWS = ((0, 0), (0, 1), (1, 0), (4, 4), (3, 5))   # samples by which the source / the `voiced` destination are off a 16-byte boundary
RESIDUES = (0, 1, 4, 7)                            # clip offsets mod 8 inside one batch


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def amplitude(fsamp):
    return 500 if fsamp >= 100 else 3


_CLIPS = {}


def batch(fsamp, ring, counts, seed, same_len=False):
    """[(clip, oracle keep, seg, voiced)], computed once per key and shared read-only between the routes."""
    key = (fsamp, ring, counts, seed, same_len)
    if key not in _CLIPS:
        thr = amplitude(fsamp) ** 2
        if same_len:
            rng = np.random.default_rng(seed)
            clips = [V.clip_from_flags(V.family_flags(V.FAMILIES[(i + seed) % len(V.FAMILIES)], counts[0], ring, rng), fsamp, thr, rng, tail=fsamp)
                     for i in range(3)]
        else:
            clips = [c for c, _ in V.clips_for(fsamp, ring, thr, counts, seed)]
        out = []
        for c in clips:
            keep, seg, voiced = vad_ref.vad_energy(c, sample_rate=fsamp, frame_duration_ms=1000, padding_duration_ms=1000 * ring,
                                                   threshold=thr)
            for a in (c, keep, seg, voiced):
                a.setflags(write=False)
            out.append((c, keep, seg, voiced))
        _CLIPS[key] = out
    return _CLIPS[key]


def run_and_check(eng, items, fsamp, ring, threshold, skew, compact, matrix_stride=None, pass_lengths=True):
    """One svk_vad_energy call on the clips of `items`, laid out ragged (offsets mod 8 cycling through RESIDUES) or as a padded
    matrix, source and destination each `skew` samples off a 16-byte boundary; everything it returns against the oracle."""
    rng = np.random.default_rng(len(items) + fsamp)
    lens = np.array([len(c) for c, _, _, _ in items], dtype=np.int32)
    if matrix_stride is None:
        offs, cur = [], 0
        for i, n in enumerate(lens):
            cur += (RESIDUES[i % 4] - cur) % 8
            offs.append(cur)
            cur += int(n) + 3
        total = cur + 8
    else:
        offs = [i * matrix_stride for i in range(len(items))]
        total = matrix_stride * len(items)
        assert lens.max() <= matrix_stride and (pass_lengths or (lens == matrix_stride).all())
    a, b = skew
    host = rng.choice(np.array([-30000, 30000], dtype=np.int16), a + total + 8)      # loud where no clip lies
    inside = np.zeros(b + total + 8, dtype=bool)
    for (c, _, _, _), o in zip(items, offs):
        host[a + o:a + o + len(c)] = c
        inside[b + o:b + o + len(c)] = True
    big = torch.from_numpy(host).to(eng.device)
    obig = torch.full((b + total + 8,), V.SENTINEL, dtype=torch.int16, device=eng.device)
    x, vo = big[a:a + total], obig[b:b + total]
    assert x.data_ptr() % 16 == (2 * a) % 16 and vo.data_ptr() % 16 == (2 * b) % 16
    kw = dict(frame_samples=fsamp, ring_len=ring, want_segments=True, compact=compact)
    if matrix_stride is None:
        kw.update(lengths=lens, offsets=np.array(offs, dtype=np.int64))
    else:
        x, vo = x.view(len(items), matrix_stride), vo.view(len(items), matrix_stride)
        if pass_lengths:
            kw.update(lengths=lens)
    if compact is True:
        kw.update(voiced_out=vo)
    r = eng.vad_energy(x, threshold, **kw)
    torch.cuda.synchronize()
    keep, seg, nvf = r["keep"].cpu().numpy(), r["seg"].cpu().numpy(), r["n_vad_frames"].cpu().numpy()
    vlen = r["voiced_len"].cpu().numpy()
    max_vf = keep.shape[1]
    longest = int(lens.max()) if matrix_stride is None else matrix_stride        # (a matrix is sized by its stride)
    assert max_vf == max(1, (2 * longest - 1) // (2 * fsamp)) >= max(len(k) for _, k, _, _ in items)
    if compact is True:
        assert r["voiced"].data_ptr() == vo.data_ptr()
        got_v = obig.cpu().numpy()
        assert (got_v[~inside] == V.SENTINEL).all(), "svk_vad_energy wrote outside a clip's own slot of `voiced`"
    else:
        assert r["voiced"] is None
        src = r["src_frame"].cpu().numpy()
    for u, ((c, wkeep, wseg, wvoiced), o) in enumerate(zip(items, offs)):
        nf = len(wkeep)
        assert nvf[u] == nf, (u, nvf[u], nf)
        np.testing.assert_array_equal(keep[u], np.concatenate([wkeep, np.zeros(max_vf - nf, dtype=bool)]).astype(np.uint8),
                                      err_msg="keep of clip %d (%d frames)" % (u, nf))
        np.testing.assert_array_equal(seg[u], np.concatenate([wseg, np.full(max_vf - nf, -1, dtype=np.int32)]),
                                      err_msg="seg of clip %d (%d frames)" % (u, nf))
        assert vlen[u] == len(wvoiced) == int(wkeep.sum()) * fsamp
        if compact is True:
            np.testing.assert_array_equal(got_v[b + o:b + o + vlen[u]], wvoiced, err_msg="voiced of clip %d" % u)
        else:
            np.testing.assert_array_equal(src[u, :int(wkeep.sum())], np.nonzero(wkeep)[0])


def _cells():
    out, n = [], [0]

    def add(route, fsamp, counts, compact=True, ring=None):
        i = n[0]
        n[0] += 1
        ring = ALL_RINGS[i % len(ALL_RINGS)] if ring is None else ring
        skew = SKEWS[i % len(SKEWS)]
        out.append(pytest.param(route, fsamp, ring, counts, skew, compact,
                                id="split=%s-fs%d-ring%d-max%d-skew%d.%d-%s" % (route, fsamp, ring, max(counts), *skew, compact)))

    for fsamp in USUAL:                      # the library's own choice: small kernel up to 512 frames, the split trio beyond
        add(None, fsamp, UP_TO_512)
        add(None, fsamp, UP_TO_513)
        add(None, fsamp, V.FRAME_COUNTS)
        add("1", fsamp, UP_TO_512)           # the trio forced onto short clips
        add("2", fsamp, V.FRAME_COUNTS)      # vad_kernel with one vector per lane
        add("2", fsamp, UP_TO_512)
    for fsamp in UNUSUAL:                    # vad_kernel's per-frame loop: asked for plainly, and through both forced routes
        counts = SHORT_LIST if fsamp > 520 else V.FRAME_COUNTS
        for route in (None, "1", "2"):
            add(route, fsamp, counts)
    for ring in ALL_RINGS:                   # every ring through every walk
        add(None, 160, UP_TO_512, ring=ring)         # vad_small_kernel: vad_walk_wave on LDS flags
        add(None, 8, V.FRAME_COUNTS, ring=ring)      # vad_walk_kernel: vad_walk_wave on the workspace's flags
        add("2", 8, V.FRAME_COUNTS, ring=ring)       # vad_kernel: the sequential walk
    for route, fsamp, counts in ((None, 480, UP_TO_512), (None, 480, UP_TO_513), ("2", 160, V.FRAME_COUNTS), (None, 1323, SHORT_LIST),
                                 ("1", 100, UP_TO_513)):
        add(route, fsamp, counts, compact="index")
    return out


@gpu
@pytest.mark.parametrize("route,fsamp,ring,counts,skew,compact", _cells())
def test_ragged_batch_equals_the_oracle(eng, monkeypatch, route, fsamp, ring, counts, skew, compact):
    """A ragged batch (zero-length clip, frame_samples, frame_samples + 1, ... the longest) whose clips start 0, 1, 4 and 7
    samples past a multiple of 8, with source and destination skewed independently."""
    if route is not None:
        monkeypatch.setenv("SVK_VAD_SPLIT", route)
    items = batch(fsamp, ring, counts, seed=fsamp + ring)
    run_and_check(eng, items, fsamp, ring, amplitude(fsamp) ** 2, skew, compact)


@gpu
@pytest.mark.parametrize("route", [None, "1", "2"])
@pytest.mark.parametrize("fsamp,nf,ring,skew", [(480, 130, 10, (0, 0)), (480, 600, 33, (0, 4)), (160, 513, 2, (1, 0)), (8, 512, 64, (0, 0)),
                                                (1323, 65, 10, (0, 0)), (100, 129, 65, (4, 0)), (520, 70, 100, (0, 0))])
def test_padded_matrix_with_an_odd_stride(eng, monkeypatch, route, fsamp, nf, ring, skew):
    """Three clips as rows of a matrix whose stride is no multiple of 8 samples (rows 1 and 2 are off the 16-byte boundary by
    different amounts), with per-row lengths and, all rows full, without."""
    if route is not None:
        monkeypatch.setenv("SVK_VAD_SPLIT", route)
    thr = amplitude(fsamp) ** 2
    items = batch(fsamp, ring, (nf, max(nf // 2, 1), 1), seed=7)
    items = [it for it in items if len(it[0]) > fsamp][:3]
    assert len(items) == 3
    stride = max(len(c) for c, _, _, _ in items) + 5
    stride += 1 - stride % 2              # odd
    run_and_check(eng, items, fsamp, ring, thr, skew, True, matrix_stride=stride)
    same = batch(fsamp, ring, (nf,), seed=8, same_len=True)
    stride = len(same[0][0])
    if stride % 8 == 0:                   # three samples off the tail: the same frames, a stride that is no multiple of 8
        same = [(c[:-3], k, s, v) for c, k, s, v in same]
        stride -= 3
    assert stride % 8 != 0
    run_and_check(eng, same, fsamp, ring, thr, skew, True, matrix_stride=stride, pass_lengths=False)


@gpu
@pytest.mark.parametrize("route", [None, "1", "2"])
@pytest.mark.parametrize("fsamp", [480, 8, 100])
def test_full_scale_negative_frames_at_equality(eng, monkeypatch, route, fsamp):
    """Frames of -32768 only: the paired 32-bit squares of the vector loads reach exactly 2^31, and sum(x^2) = 2^30 n.  With
    threshold 2^30 that is equality (no frame voiced, nothing kept); with 2^30 - 1 every frame is voiced."""
    if route is not None:
        monkeypatch.setenv("SVK_VAD_SPLIT", route)
    clips = [np.full(nf * fsamp + 1, -32768, dtype=np.int16) for nf in (40, 65, 1)]
    for thr, voiced in ((1 << 30, False), ((1 << 30) - 1, True)):
        items = []
        for c in clips:
            keep, seg, v = vad_ref.vad_energy(c, sample_rate=fsamp, frame_duration_ms=1000, padding_duration_ms=10000, threshold=thr)
            assert keep.any() == (voiced and len(keep) >= 10)
            items.append((c, keep, seg, v))
        run_and_check(eng, items, fsamp, 10, thr, (0, 0), True)
        run_and_check(eng, items, fsamp, 10, thr, (1, 0), True)
