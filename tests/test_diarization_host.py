"""The host side of speaker diarization (speaker_verification_amd/diarization.py) and the reference form of the clustering
(tests/ahc_f64_ref.py): no GPU."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ahc_f64_ref as ref  # noqa: E402

from speaker_verification_amd import diarization as dz  # noqa: E402
from speaker_verification_amd.diarization import Turn  # noqa: E402


# ---- the reference form against scipy -------------------------------------------------------------------------------
def gaussian_set(seed):
    """5 - 70 points in 1 - 4 well separated Gaussian clusters in 32 dimensions -> cosine affinities (float32)."""
    rng = np.random.default_rng(seed)
    n, k = int(rng.integers(5, 71)), int(rng.integers(1, 5))
    centres = rng.standard_normal((k, 32)) * 3.0
    x = centres[rng.integers(0, k, n)] + 0.3 * rng.standard_normal((n, 32))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x @ x.T).astype(np.float32)


def same_partition(a, b):
    return np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])


@pytest.mark.parametrize("seed", range(20))
def test_reference_form_agrees_with_scipy(seed):
    """Average linkage on distances 1 - S cut at 1 - thr is the threshold rule on similarities.  The two differ in rounding
    only (scipy updates distances, in another operation order), so the inputs are separated sets, where no decision hinges on
    the last bit."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    S = gaussian_set(seed)
    n, thr = S.shape[0], 0.3
    labels, count, pairs, sims = ref.ahc(S, n, threshold=thr)
    D = 1.0 - S.astype(np.float64)
    D = (D + D.T) / 2
    np.fill_diagonal(D, 0.0)
    want = fcluster(linkage(squareform(D, checks=False), "average"), 1.0 - thr, "distance")
    assert same_partition(labels[:n], want)
    assert count == len(set(want)) == labels[:n].max() + 1
    steps = n - count
    assert (pairs[:steps, 0] < pairs[:steps, 1]).all() and (pairs[steps:] == -1).all()
    assert (sims[:steps] >= thr).all() and np.isnan(sims[steps:]).all()
    first = [int(np.flatnonzero(labels[:n] == c)[0]) for c in range(count)]
    assert first == sorted(first)                                   # numbered in the order of their lowest member


def test_reference_form_ties_stop_rules_and_rejects():
    S = np.full((6, 6), 0.5, np.float32)                            # every pair ties: lowest i, then lowest j
    labels, count, pairs, sims = ref.ahc(S, 4, threshold=0.5)
    assert count == 1 and pairs[:3].tolist() == [[0, 1], [0, 2], [0, 3]] and labels.tolist() == [0, 0, 0, 0, -1, -1]
    assert ref.ahc(S, 4, threshold=0.6)[1] == 4
    assert ref.ahc(S, 4, threshold=0.6, max_clusters=3)[1] == 3
    assert ref.ahc(S, 4, threshold=0.5, min_clusters=2)[1] == 2
    assert ref.ahc(S, 4, threshold=0.6, target=2)[1] == 2 and ref.ahc(S, 4, threshold=0.5, target=9)[1] == 4
    assert ref.ahc(S, 0)[1] == 0 and ref.ahc(S, 1)[1] == 1 and ref.ahc(S, 7)[1] == -1 and ref.ahc(S, -1)[1] == -1
    bad = S.copy()
    bad[2, 1] = np.nan                                              # below the diagonal: ignored
    bad[1, 5] = np.inf                                              # a dead column: ignored
    assert ref.ahc(bad, 4, threshold=0.5)[1] == 1
    bad[1, 2] = np.inf
    got = ref.ahc(bad, 4, threshold=0.5)
    assert got[1] == -1 and (got[0] == -1).all() and (got[2] == -1).all()


def test_reference_form_update_is_the_weighted_mean():
    S = np.zeros((3, 3), np.float32)
    S[0, 1], S[0, 2], S[1, 2] = 0.9, 0.2, 0.5
    _, count, pairs, sims = ref.ahc(S, 3, threshold=-1.0)
    assert count == 1 and pairs[:2].tolist() == [[0, 1], [0, 2]]
    assert sims[1] == (np.float64(np.float32(0.2)) + np.float64(np.float32(0.5))) / 2.0


# ---- the window rule ------------------------------------------------------------------------------------------------
def test_host_window_rule():
    cases = {0: [], 79: [], 80: [(0, 80)], 81: [(0, 81)], 149: [(0, 149)], 150: [(0, 150)], 151: [(0, 150), (1, 150)],
             224: [(0, 150), (74, 150)], 225: [(0, 150), (75, 150)], 226: [(0, 150), (75, 150), (76, 150)]}
    for T, wins in cases.items():
        crops, n, spans, over = dz.window_table(T, 4)
        assert n == len(wins) == dz.num_windows(T, 150, 75, 80) and not over, T
        assert spans[:n].tolist() == [list(w) for w in wins] and (spans[n:] == [-1, 0]).all() and (crops[n:] == -1).all()
        for w, (w0, length) in enumerate(wins):
            assert crops[w, 0] == w0 and crops[w, -1] == w0 + length - 80
            assert crops[w].tolist() == [w0 + (k * (length - 80)) // 19 for k in range(20)]
    assert dz.num_windows(1000, 150, 75, 80) == 13                  # 12 hops (0 .. 825) and the flush window at 850
    crops, n, spans, over = dz.window_table(1000, 12)
    assert n == 12 and over and spans[-1].tolist() == [825, 150]
    crops, n, spans, _ = dz.window_table(1000, 13)
    assert spans[12].tolist() == [850, 150]
    crops, n, spans, _ = dz.window_table(200, 3, win_frames=80, hop_frames=40, crop_frames=80, n_crops=1)
    assert n == 3 and crops[:, 0].tolist() == [0, 40, 80] and dz.num_windows(200, 80, 40, 80) == 4


# ---- the timeline ---------------------------------------------------------------------------------------------------
def test_frame_labels_centre_rule_and_tie():
    spans = [(0, 150), (75, 150), (150, 150)]                       # centres at 75, 150, 225
    fl = dz.frame_labels(spans, [5, 6, 7], 300)
    # frame f has its centre at f + 1/2: nearer to 75 than to 150 up to f = 111; f = 112 (centre 112.5) is 37.5 from both and
    # goes to the earlier window, as f = 187 does between 150 and 225
    assert (fl[:113] == 5).all() and (fl[113:188] == 6).all() and (fl[188:] == 7).all()
    # a tie: windows (0, 3) and (2, 3) have centres 1.5 and 3.5; frame 2 (centre 2.5) is one away from both: the earlier wins
    assert dz.frame_labels([(0, 3), (2, 3)], [1, 2], 5).tolist() == [1, 1, 1, 2, 2]
    assert dz.frame_labels(np.zeros((0, 2)), [], 4).tolist() == [-1] * 4


def test_timeline_runs_gaps_and_src_frame():
    fs, stride, S = 16000, 160, 480                                 # 10 ms feature hop, 30 ms VAD frames
    fl = np.array([0] * 6 + [1] * 6, np.int32)                      # 12 frames: packed samples 0 .. 1920, tail to n_packed
    # no VAD map: one turn per run, the last run takes the tail
    assert dz.timeline(fl, stride, 2400, None, 1, fs) == [Turn(0.0, 0.06, 0), Turn(0.06, 0.15, 1)]
    # hand-made map: kept VAD frames 0, 1 | 10, 11, 12 -- a gap after 960 packed samples, which is INSIDE run 0 (0 .. 960)?
    # run 0 covers packed [0, 960) = kept frames 0, 1 exactly; run 1 covers [960, 2400) = kept frames 2, 3, 4 -> source 10, 11, 12
    src = np.array([0, 1, 10, 11, 12, -99], np.int32)
    assert dz.timeline(fl, stride, 2400, src, S, fs) == [Turn(0.0, 0.06, 0), Turn(4800 / fs, 6240 / fs, 1)]
    # a VAD gap INSIDE a run splits the turn: kept frames 0 | 5, 6, 7, 8
    src = np.array([0, 5, 6, 7, 8], np.int32)
    want = [Turn(0.0, 480 / fs, 0), Turn(2400 / fs, (2400 + 480) / fs, 0), Turn(2880 / fs, (2880 + 1440) / fs, 1)]
    assert dz.timeline(fl, stride, 2400, src, S, fs) == want
    # a run boundary in the middle of a VAD frame: packed 800 = kept frame 1 (source 5) + 320 samples
    fl2 = np.array([0] * 5 + [1] * 7, np.int32)
    got = dz.timeline(fl2, stride, 2400, src, S, fs)
    assert got == [Turn(0.0, 480 / fs, 0), Turn(2400 / fs, 2720 / fs, 0), Turn(2720 / fs, 4320 / fs, 1)]
    # unlabelled frames give no turn; nothing voiced gives nothing
    assert dz.timeline(np.full(12, -1, np.int32), stride, 2400, None, 1, fs) == []
    assert dz.timeline(fl, stride, 0, None, 1, fs) == []


# ---- RTTM -----------------------------------------------------------------------------------------------------------
def test_rttm_round_trip(tmp_path):
    turns = {"rec_a": [Turn(0.0, 1.25, 0), Turn(1.25, 3.5, 1), Turn(4.0, 4.75, 0)], "rec_b": [Turn(0.125, 2.0, "alice")]}
    path = str(tmp_path / "out.rttm")
    dz.write_rttm(path, turns)
    lines = open(path).read().splitlines()
    assert lines[0] == "SPEAKER rec_a 1 0.000000 1.250000 <NA> <NA> 0 <NA> <NA>" and len(lines) == 4
    assert dz.read_rttm(path) == turns


# ---- DER ------------------------------------------------------------------------------------------------------------
REF = [Turn(0.0, 10.0, "a"), Turn(10.0, 20.0, "b")]


def test_der_known_answers():
    assert dz.der(REF, REF) == 0.0
    assert dz.der(REF, [Turn(0.0, 10.0, 1), Turn(10.0, 20.0, 0)]) == 0.0                  # labels permuted
    # the second half of speaker a given to b's cluster: 5 s of confusion over 20 s of speech
    swapped = [Turn(0.0, 5.0, 0), Turn(5.0, 20.0, 1)]
    assert dz.der(REF, swapped) == pytest.approx(5.0 / 20.0, abs=1e-12)
    # one missed turn: 10 of 20 seconds
    assert dz.der(REF, [Turn(0.0, 10.0, 0)]) == pytest.approx(0.5, abs=1e-12)
    # a false alarm of 2 s after the end
    assert dz.der(REF, REF + [Turn(20.0, 22.0, "a")]) == pytest.approx(2.0 / 20.0, abs=1e-12)
    # a collar: the hypothesis changes speaker 0.2 s late; +-0.25 s around the reference boundary is not scored
    late = [Turn(0.0, 10.2, 0), Turn(10.2, 20.0, 1)]
    assert dz.der(REF, late) == pytest.approx(0.2 / 20.0, abs=1e-12)
    assert dz.der(REF, late, collar=0.25) == 0.0
    # with the collar the scored reference shrinks too: 0.25 s at both ends and 0.5 s in the middle
    assert dz.der(REF, swapped, collar=0.25) == pytest.approx(4.75 / 19.0, abs=1e-12)
    with pytest.raises(ValueError):
        dz.der([], REF)


# ---- argument rules that need no engine -------------------------------------------------------------------------------
def fake_pipeline(**kw):
    return types.SimpleNamespace(**dict(dict(plda=None, calibration=None, score_norm=None, backend=None), **kw))


def test_diarize_needs_a_stop_rule():
    d = dz.Diarizer(fake_pipeline())
    assert (d.win_frames, d.hop_frames) == (150, 75)
    with pytest.raises(ValueError, match="threshold"):
        d.diarize(np.zeros((1, 16000), np.int16))


@pytest.mark.parametrize("what", ["plda", "calibration", "score_norm"])
def test_diarizer_names_what_is_not_built(what):
    with pytest.raises(ValueError, match=what):
        dz.Diarizer(fake_pipeline(**{what: object()}))
    assert dz.Diarizer(fake_pipeline(backend=object())).pipeline.backend is not None
    with pytest.raises(ValueError):
        dz.Diarizer(fake_pipeline(), window_s=0.5)
