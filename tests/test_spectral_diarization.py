"""diarize(method="spectral") end to end on the synthetic conversations of tests/test_diarization_pipeline.py (rebuilt here) and on
one long enough to take the two-stage route: what the device counted, chose and labelled must be what the definitions
(tests/spectral_f64_ref.py, tests/ahc_f64_ref.py) give on the device's own affinities, and the turns must be the host timeline of
those labels.  The estimated speaker counts and the DER are PRINTED, not asserted: they are properties of the synthetic
checkpoint, not of the code under test."""
import os

import numpy as np
import pytest

import ahc_f64_ref
import spectral_f64_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURN_S = 3
SPEAKERS = [[11, 12], [21, 22, 23]]
LONG_SPEAKERS, LONG_TURNS = [31, 32, 33], 40          # 120 s: more 1.5 s windows than svk_spectral_embed takes nodes
MARGIN = 1e-9


def conversation(speakers, turns=8):
    """Turns of 3 s, the speakers in rotation -> (int16 PCM, ground-truth turns)."""
    from speaker_verification_amd import synth
    from speaker_verification_amd.diarization import Turn
    clips, truth = [], []
    for t in range(turns):
        who = speakers[t % len(speakers)]
        clips.append(synth.speaker_clip(who, t // len(speakers), TURN_S * synth.SAMPLE_RATE))
        truth.append(Turn(float(TURN_S * t), float(TURN_S * (t + 1)), who))
    return np.concatenate(clips), truth


def reference_chain(aff, n_win, limit, **kw):
    """The chain of Diarizer._spectral in NumPy on one batch of affinities -> per recording (window labels [K] with -1 in dead
    windows, the reference dict of the spectral step, the groups or None)."""
    out = []
    K = aff.shape[1]
    for r, n in enumerate(n_win):
        group = ahc_f64_ref.ahc(aff[r], n, max_clusters=limit)[0] if K > limit else None
        spec = ref.spectral(aff[r], n, group, limit if group is not None else None, **kw)
        node_labels = ref.embedding_labels(spec["embed"], spec["n_nodes"], spec["n_speakers"])
        labels = np.full(K, -1, np.int32)
        labels[:n] = node_labels if group is None else ref.gather_labels(node_labels, group, n)
        out.append((labels, spec, group))
    return out


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.diarization import Diarizer
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ck = torch.load(os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu",
                    weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    pipe = VerificationPipeline(model, use_vad=True)
    made = [conversation(s) for s in SPEAKERS]
    pcm = np.stack([m[0] for m in made])
    d = Diarizer(pipe)
    turns, dev = d.diarize(pcm, method="spectral", return_device=True)
    long_pcm, long_truth = conversation(LONG_SPEAKERS, LONG_TURNS)
    long_turns, long_dev = d.diarize(long_pcm[None], method="spectral", return_device=True)
    return {"pipe": pipe, "d": d, "pcm": pcm, "truth": [m[1] for m in made], "turns": turns, "dev": dev,
            "long": (long_pcm, long_truth, long_turns, long_dev), "limit": pipe.eng.spectral_limits()[0]}


def assert_chain(dev, limit, two_stage):
    aff, n_win = dev["affinity"].cpu().numpy(), dev["n_windows"].cpu().numpy()
    want = reference_chain(aff, n_win, limit, neighbours=(2, 32, 2), max_speakers=8)
    assert (dev["group"] is not None) == two_stage
    for r, (labels, spec, group) in enumerate(want):
        for what in ("margin_ratio", "margin_gap", "margin_keep"):       # the device's affinities decide nothing on a last bit
            assert spec[what] > MARGIN, "recording %d: %s = %g" % (r, what, spec[what])
        assert dev["n_nodes"][r].item() == spec["n_nodes"] and dev["neighbours"][r].item() == spec["neighbours"]
        assert dev["n_clusters"][r].item() == spec["n_speakers"]
        if two_stage:
            assert np.array_equal(dev["group"][r].cpu().numpy()[:n_win[r]], group[:n_win[r]])
        assert np.array_equal(dev["labels"][r].cpu().numpy(), labels), "recording %d" % r
    return want


def assert_timeline(pipe, dev, turns, seconds):
    from speaker_verification_amd import diarization as dz
    labels, spans = dev["labels"].cpu().numpy(), dev["spans"].cpu().numpy()
    n_win, n_frames, packed = (dev[k].cpu().numpy() for k in ("n_windows", "n_frames", "packed"))
    src = dev["src_frame"].cpu().numpy()
    for r, ts in enumerate(turns):
        fl = dz.frame_labels(spans[r, :n_win[r]], labels[r, :n_win[r]], n_frames[r])
        assert ts == dz.timeline(fl, pipe.spec.frame_stride, packed[r], src[r], dev["frame_samples"])
        ends, starts = np.array([t.end_s for t in ts]), np.array([t.start_s for t in ts])
        assert (ends > starts).all() and (starts[1:] >= ends[:-1]).all() and ends[-1] <= seconds
        assert abs(float((ends - starts).sum()) - packed[r] / 16000.0) < 1e-6          # every voiced sample lies in exactly one turn


def test_count_neighbours_and_labels_are_the_definition_on_the_device_affinities(world):
    dev = world["dev"]
    assert (dev["n_windows"].cpu().numpy() >= 10).all() and dev["affinity"].shape[1] <= world["limit"]
    assert_chain(dev, world["limit"], two_stage=False)
    assert_timeline(world["pipe"], dev, world["turns"], TURN_S * 8)


def test_num_speakers_is_the_target(world):
    turns, dev = world["d"].diarize(world["pcm"], method="spectral", num_speakers=[2, 3], return_device=True)
    assert dev["n_clusters"].cpu().numpy().tolist() == [2, 3]
    assert [len({t.speaker for t in ts}) for ts in turns] == [2, 3]
    labels, n_win = dev["labels"].cpu().numpy(), dev["n_windows"].cpu().numpy()
    assert [sorted(set(labels[r, :n_win[r]])) for r in range(2)] == [[0, 1], [0, 1, 2]]
    assert torch.equal(dev["neighbours"], world["dev"]["neighbours"])                # the target leaves the graph alone


def test_ahc_stays_what_it_was(world):
    d, pcm = world["d"], world["pcm"]
    plain, dev_plain = d.diarize(pcm, num_speakers=[2, 3], return_device=True)
    named, dev_named = d.diarize(pcm, num_speakers=[2, 3], method="ahc", return_device=True)
    assert plain == named and torch.equal(dev_plain["labels"], dev_named["labels"])
    assert torch.equal(dev_plain["affinity"], dev_named["affinity"]) and torch.equal(dev_plain["n_clusters"], dev_named["n_clusters"])
    assert world["pipe"].diarize(pcm, method="spectral") == world["turns"]            # the keyword passes through the pipeline
    with pytest.raises(ValueError, match="threshold"):
        d.diarize(pcm, method="spectral", threshold=0.2)
    with pytest.raises(ValueError, match="unknown method"):
        d.diarize(pcm, method="kmeans")


def test_a_long_recording_takes_the_two_stage_route(world):
    pcm, truth, turns, dev = world["long"]
    assert dev["n_windows"][0].item() > world["limit"] and dev["n_nodes"][0].item() == world["limit"] == 128
    assert_chain(dev, world["limit"], two_stage=True)
    assert_timeline(world["pipe"], dev, turns, TURN_S * LONG_TURNS)


def test_counts_and_der_are_reported(world, capsys):
    from speaker_verification_amd.diarization import der
    with capsys.disabled():
        rows = list(zip(SPEAKERS, world["truth"], world["turns"], world["dev"]["n_clusters"].cpu().tolist(),
                        world["dev"]["neighbours"].cpu().tolist()))
        pcm, truth, turns, dev = world["long"]
        rows.append((LONG_SPEAKERS, truth, turns[0], dev["n_clusters"][0].item(), dev["neighbours"][0].item()))
        for r, (spk, truth, ts, count, p) in enumerate(rows):
            print("\nconversation %d (%d speakers, %d s) under method='spectral', count unknown: %d speakers estimated, p = %d, "
                  "DER %.4f (collar 0), %.4f (collar 0.25 s), %d turns"
                  % (r, len(spk), int(truth[-1].end_s), count, p, der(truth, ts), der(truth, ts, collar=0.25), len(ts)))
