"""Diarization end to end (pipeline.diarize / diarization.Diarizer) on two synthetic conversations with the committed checkpoint:
what the device clustered must be what the definition (tests/ahc_f64_ref.py) gives on the device's own affinities, and the turns
must be the host timeline of those labels.  The DER against the construction's ground truth is PRINTED, not asserted: how well
1.5 s windows separate these synthetic voices is a property of the checkpoint, not of the code under test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ahc_f64_ref as ref  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURN_S, TURNS = 3, 8
SPEAKERS = [[11, 12], [21, 22, 23]]


def conversation(speakers):
    """Turns of 3 s, the speakers in rotation -> (int16 PCM, ground-truth turns)."""
    from speaker_verification_amd import synth
    from speaker_verification_amd.diarization import Turn
    clips, truth = [], []
    for t in range(TURNS):
        who = speakers[t % len(speakers)]
        clips.append(synth.speaker_clip(who, t // len(speakers), TURN_S * synth.SAMPLE_RATE))
        truth.append(Turn(float(TURN_S * t), float(TURN_S * (t + 1)), who))
    return np.concatenate(clips), truth


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
    turns, dev = Diarizer(pipe).diarize(pcm, num_speakers=[2, 3], return_device=True)
    return {"pipe": pipe, "model": model, "pcm": pcm, "truth": [m[1] for m in made], "turns": turns, "dev": dev,
            "Diarizer": Diarizer, "Pipeline": VerificationPipeline}


def test_labels_are_the_definition_on_the_device_affinities(world):
    dev = world["dev"]
    aff, n_win = world["Diarizer"](world["pipe"]).affinity(world["pcm"])
    assert torch.equal(aff, dev["affinity"]) and torch.equal(n_win, dev["n_windows"])
    n_win = n_win.cpu().numpy()
    assert (n_win >= 10).all()                         # 24 s with the VAD's pauses removed: well over ten 1.5 s windows
    labels, count, _, _ = ref.ahc_batch(aff.cpu().numpy(), n_win, target=[2, 3])
    assert np.array_equal(dev["labels"].cpu().numpy(), labels)
    assert dev["n_clusters"].cpu().numpy().tolist() == count.tolist() == [2, 3]


def test_turns_are_the_host_timeline_of_the_device_labels(world):
    from speaker_verification_amd import diarization as dz
    dev, pipe = world["dev"], world["pipe"]
    labels, spans = dev["labels"].cpu().numpy(), dev["spans"].cpu().numpy()
    n_win, n_frames, packed = (dev[k].cpu().numpy() for k in ("n_windows", "n_frames", "packed"))
    src = dev["src_frame"].cpu().numpy()
    for r, turns in enumerate(world["turns"]):
        fl = dz.frame_labels(spans[r, :n_win[r]], labels[r, :n_win[r]], n_frames[r])
        assert turns == dz.timeline(fl, pipe.spec.frame_stride, packed[r], src[r], dev["frame_samples"])
        assert len(turns) >= 2 and {t.speaker for t in turns} == set(range(len(SPEAKERS[r])))
        ends = np.array([t.end_s for t in turns])
        starts = np.array([t.start_s for t in turns])
        assert (ends > starts).all() and (starts[1:] >= ends[:-1]).all() and ends[-1] <= TURN_S * TURNS
        voiced = float((ends - starts).sum())
        assert abs(voiced - packed[r] / 16000.0) < 1e-6             # every voiced sample lies in exactly one turn


def test_pipeline_diarize_is_the_diarizer(world):
    again = world["pipe"].diarize(world["pcm"], num_speakers=[2, 3])
    assert again == world["turns"]
    assert world["pipe"].diarize(world["pcm"], num_speakers=[2, 3]) == again        # the cached Diarizer, the same bits
    with pytest.raises(ValueError, match="threshold"):
        world["pipe"].diarize(world["pcm"])


def test_der_against_the_construction_is_reported(world, capsys):
    from speaker_verification_amd.diarization import der
    with capsys.disabled():
        for r, (truth, turns) in enumerate(zip(world["truth"], world["turns"])):
            print("\nconversation %d (%d speakers, %d s): DER %.4f (collar 0), %.4f (collar 0.25 s), %d turns"
                  % (r, len(SPEAKERS[r]), TURN_S * TURNS, der(truth, turns), der(truth, turns, collar=0.25), len(turns)))


def test_backend_projected_windows_are_what_the_affinity_sees(world):
    from speaker_verification_amd.backend import EmbeddingBackend
    pipe = world["pipe"]
    eng = pipe.eng
    plain = world["Diarizer"](pipe)._windows(world["pcm"], None)
    n_rec, K = plain["emb"].shape[:2]
    # a back end fitted on the windows themselves, labelled by the plain clustering: any fitted projection serves the wiring check
    live = (torch.arange(K, device=eng.device)[None, :] < plain["n_windows"][:, None]).cpu().numpy()
    ids = (world["dev"]["labels"].cpu().numpy() + 10 * np.arange(n_rec)[:, None])[live]
    rows = plain["emb"].cpu().numpy()[live]
    b = EmbeddingBackend().fit(rows, ids, method="lda", out_dim=4, shrinkage=1e-2)
    with_backend = world["Pipeline"](world["model"], use_vad=True, backend=b)
    aff, n_win = world["Diarizer"](with_backend).affinity(world["pcm"])
    projected = b.transform(plain["emb"].reshape(n_rec * K, -1), engine=eng).view(n_rec, K, -1)
    assert projected.shape[-1] == 4
    assert torch.equal(aff, eng.segment_affinity(projected, plain["n_windows"])) and torch.equal(n_win, plain["n_windows"])
    assert not torch.equal(aff, world["dev"]["affinity"])
    turns = with_backend.diarize(world["pcm"], num_speakers=[2, 3])
    assert [len({t.speaker for t in ts}) for ts in turns] == [2, 3]
