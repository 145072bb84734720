"""Trial-list verification end to end: the synthetic corpus through VerificationPipeline.embed with the committed checkpoint,
make_trials, evaluate_trials on the device against its host path, pipeline.score_trials, and a list read back from a file."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ((0.01, 1, 1), (0.05, 1, 1), (0.5, 1, 1))


@pytest.fixture(scope="module")
def setup():
    from speaker_verification_amd import evaluation, synth
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ck = torch.load(os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu",
                    weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    pipe = VerificationPipeline(model, use_vad=True)
    pcm, spk = synth.corpus(4, 3)                              # 12 clips: 12 target pairs, 54 non-target pairs
    emb = pipe.embed(pcm)
    labels, ia, ib = evaluation.make_trials(spk, 10, 30, seed=5)
    return pipe, emb, spk, labels, ia, ib


def assert_same_metrics(dev, host):
    # EER / AUC: the tolerance tests/test_device_evaluation.py holds the device path to against the host path
    assert dev["eer"] == pytest.approx(host["eer"], abs=1e-9) and dev["auc"] == pytest.approx(host["auc"], abs=1e-9)
    assert dev["eer_threshold"] == host["eer_threshold"]
    assert dev["min_dcf"] == pytest.approx(host["min_dcf"], rel=1e-13)
    assert len(dev["min_dcf"]) == len(dev["threshold"]) == len(dev["p_miss"]) == len(dev["p_fa"]) == len(OPS)


def test_device_metrics_equal_the_host_path(setup):
    from speaker_verification_amd import evaluation
    pipe, emb, spk, labels, ia, ib = setup
    np.testing.assert_array_equal(labels, (spk[ia] == spk[ib]).astype(np.uint8))
    for metric in ("cosine", "l2"):
        dev = evaluation.evaluate_trials(emb, labels, ia, ib, metric=metric, operating_points=OPS, device=True)
        host = evaluation.evaluate_trials(emb, labels, ia, ib, metric=metric, operating_points=OPS, device=False)
        assert dev["scores"].is_cuda and dev["scores"].dtype == torch.float32 and torch.equal(dev["scores"], host["scores"])
        assert_same_metrics(dev, host)
        assert 0.0 <= dev["eer"] <= 1.0 and all(0.0 <= v <= 1.0 for v in dev["min_dcf"])
    default = evaluation.evaluate_trials(emb, labels, ia, ib)
    assert len(default["min_dcf"]) == len(evaluation.DEFAULT_OPERATING_POINTS) == 2
    with pytest.raises(ValueError, match="outside"):
        bad = ia.copy()
        bad[3] = emb.shape[0]
        evaluation.evaluate_trials(emb, labels, bad, ib)


def test_pipeline_score_trials(setup):
    pipe, emb, spk, labels, ia, ib = setup
    for metric in ("cosine", "l2"):
        assert torch.equal(pipe.score_trials(emb, ia, ib, metric=metric), pipe.eng.pair_scores(emb, emb, ia, ib, metric=metric))
    other = emb.flip(0).contiguous()
    assert torch.equal(pipe.score_trials(emb, ia, ib, emb_b=other), pipe.eng.pair_scores(emb, other, ia, ib))
    full = pipe.score(emb, emb)                                 # the matrix the list is a sample of (test_gpu_parity's bar)
    got = pipe.score_trials(emb, ia, ib)
    np.testing.assert_allclose(got.cpu().numpy(), full.cpu().numpy()[ia, ib], rtol=0, atol=1e-5)


def test_a_list_read_back_from_a_file(setup, tmp_path):
    from speaker_verification_amd import evaluation
    pipe, emb, spk, labels, ia, ib = setup
    path = tmp_path / "trials.txt"
    with open(path, "w") as fh:
        fh.write("# label utterance_a utterance_b\n\n")
        for y, i, j in zip(labels, ia, ib):
            fh.write("%d spk%02d/utt%03d.wav spk%02d/utt%03d.wav\n" % (y, spk[i], i, spk[j], j))
    r_labels, r_ia, r_ib, names = evaluation.read_trials(str(path))
    np.testing.assert_array_equal(r_labels, labels)
    rows = np.array([int(name[9:12]) for name in names])        # the corpus row behind each name, in first-appearance order
    np.testing.assert_array_equal(rows[r_ia], ia)
    np.testing.assert_array_equal(rows[r_ib], ib)
    want = evaluation.evaluate_trials(emb, labels, ia, ib, operating_points=OPS)
    got = evaluation.evaluate_trials(emb[torch.from_numpy(rows).to(emb.device)], r_labels, r_ia, r_ib, operating_points=OPS)
    assert torch.equal(got["scores"], want["scores"])
    for key in ("eer", "auc", "eer_threshold", "min_dcf", "threshold", "p_miss", "p_fa"):
        assert got[key] == want[key]
