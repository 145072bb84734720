"""VerificationPipeline(vad=AdaptiveEnergyVad()) end to end with the committed checkpoint: `embed` is the same bits as the
stages chained by hand through `voiced()`, a corpus recorded 24 dB down yields no bad clip (the default pipeline's absolute rule
drops every one of them), and `diarize` keeps a speaker who is 18 dB below the other (the absolute rule calls none of that
speaker's frames speech, so nothing of that speaker reaches a window: checked on the CPU reference first)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import vad_adaptive_ref as R           # noqa: E402  (tests/ is on sys.path)
from oracle import vad_ref             # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURN_S, TURNS, LOUD, QUIET = 3, 8, 11, 12


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd import synth
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    from speaker_verification_amd.vad import AdaptiveEnergyVad
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ck = torch.load(os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu",
                    weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    pcm, _ = synth.corpus(4, 2)
    return {"Pipeline": VerificationPipeline, "model": model, "vad": AdaptiveEnergyVad(), "pcm": pcm, "synth": synth}


def test_vad_argument_rules(world):
    with pytest.raises(ValueError, match="use_vad=False"):
        world["Pipeline"](world["model"], use_vad=False, vad=world["vad"])
    with pytest.raises(ValueError, match="AdaptiveEnergyVad"):
        world["Pipeline"](world["model"], vad=250000)


def test_embed_is_the_stages_chained_by_hand_and_a_quiet_corpus_has_no_bad_clip(world):
    pcm = world["pcm"] >> 4                                     # 24 dB down
    assert pcm.shape[0] == 8
    pipe = world["Pipeline"](world["model"], vad=world["vad"], crop_rng="device")
    crops = pipe.crops_and_cubes(pcm, want_cubes=False)
    emb = pipe.embed(pcm, crop_idx=crops)
    voiced, vlen = pipe.voiced(pipe.eng.to_device(pcm))
    feat, n_frames = pipe.features(voiced, vlen)
    by_hand = pipe.embed_features(feat, crops)
    assert torch.equal(emb, by_hand) and bool(torch.isfinite(emb).all()) and float(emb.abs().max()) > 0
    # what voiced() packed is what the rule keeps
    for u in range(pcm.shape[0]):
        want = R.vad(pcm[u], 480, 10, R.DEFAULT)["voiced"]
        assert int(vlen[u]) == len(want) > 0
        np.testing.assert_array_equal(voiced[u, :len(want)].cpu().numpy(), want)
    assert int(pipe.bad_clips.item()) == 0
    drawn = pipe.embed(pcm)                                     # the device-drawn crops: the same draw, the same bits
    assert torch.equal(drawn, emb) and int(pipe.bad_clips.item()) == 0
    # the default pipeline: the absolute rule keeps nothing of these clips, every one is a bad clip
    default = world["Pipeline"](world["model"], crop_rng="device")
    default.embed(pcm)
    assert int(default.bad_clips.item()) == pcm.shape[0]
    # and at full level the adaptive pipeline has no bad clip either
    full = world["Pipeline"](world["model"], vad=world["vad"], crop_rng="device")
    full.embed(world["pcm"])
    assert int(full.bad_clips.item()) == 0


def conversation(synth):
    """Turns of 3 s, the two speakers in rotation, the second one 18 dB down -> (int16 PCM, [(start sample, end sample, who)])."""
    clips, truth = [], []
    n = TURN_S * synth.SAMPLE_RATE
    for t in range(TURNS):
        who = (LOUD, QUIET)[t % 2]
        clip = synth.speaker_clip(who, t // 2, n)
        clips.append(clip >> 3 if who == QUIET else clip)
        truth.append((t * n, (t + 1) * n, who))
    return np.concatenate(clips), truth


def test_diarize_keeps_the_quiet_speaker(world):
    from speaker_verification_amd import constants as c
    pcm, truth = conversation(world["synth"])
    n = TURN_S * world["synth"].SAMPLE_RATE
    assert n % 480 == 0                                         # the turns lie on frame boundaries
    # on the CPU first: the absolute rule drops every frame of the quiet speaker, the adaptive rule keeps most of them
    # (what it still keeps inside that speaker's turns is the collector's release tail behind the loud turn: under a second per turn)
    flags_abs = vad_ref.frame_flags(pcm, c.VAD_FRAME_MS, 16000, c.VAD_ENERGY_THRESHOLD)
    keep_abs = vad_ref.collect(flags_abs, c.VAD_FRAME_MS, c.VAD_PADDING_MS)[0]
    keep_ada = R.vad(pcm, 480, 10, R.DEFAULT)["keep"]
    kept_s, tail_s = {}, 0.0
    for who in (LOUD, QUIET):
        frames = np.concatenate([np.arange(a // 480, min(b // 480, len(keep_ada))) for a, b, w in truth if w == who])
        kept_s[who] = keep_ada[frames].sum() * 0.03
        if who == QUIET:
            assert not flags_abs[frames].any() and keep_abs[frames].sum() <= 10 * (TURNS // 2)
            tail_s = keep_abs[frames].sum() * 0.03
        else:
            assert keep_abs[frames].sum() > 0.5 * len(frames)
        assert kept_s[who] > 0.9 * len(frames) * 0.03, (who, kept_s)
    pipe = world["Pipeline"](world["model"], vad=world["vad"])
    turns = pipe.diarize(pcm[None, :], num_speakers=2)[0]
    assert {t.speaker for t in turns} == {0, 1}
    # both speakers are in the timeline: the turns cover exactly the frames the rule keeps inside each speaker's spans
    for who in (LOUD, QUIET):
        covered = sum(max(0.0, min(t.end_s, b / 16000.0) - max(t.start_s, a / 16000.0)) for t in turns for a, b, w in truth if w == who)
        assert abs(covered - kept_s[who]) < 1e-6, (who, covered, kept_s[who])
    # under the default pipeline the quiet speaker's spans hold the release tails and nothing else
    turns_abs = world["Pipeline"](world["model"]).diarize(pcm[None, :], num_speakers=2)[0]
    covered = sum(max(0.0, min(t.end_s, b / 16000.0) - max(t.start_s, a / 16000.0)) for t in turns_abs for a, b, w in truth if w == QUIET)
    assert abs(covered - tail_s) < 1e-6 and tail_s < 0.1 * kept_s[QUIET]
