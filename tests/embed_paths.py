"""The cases of tests/test_embedding_invariance.py, stated once: two seeded worlds of clips, a covering set of pipeline
configurations, and one runner per embed path.  A helper module, not a test (as tests/vad_cases.py is for the VAD).

THE CLAIM ("One clip, one embedding"): a clip's embedding depends on the clip, its global index and the pipeline's
options -- not on the other clips of the launch, on the batch cuts (micro_batch, max_batch_samples, upload pieces) or on which
embed method carried it.  Every runner here returns [n, 128] for the same clips with the same global indices F .. F + n - 1.

overlap_front=True is deliberately absent: DESIGN §7 records that it is not bit-stable against the serial schedule.
"""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKPOINT = os.path.join(REPO, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt")

F = 700                                       # global index of clip 0 in every run
FS = 16000
# The ragged world, in list order (the length sort reorders it): 1 - 3 s clips, two of them equal; one whose frame count is
# just under 1 024 (the front end counts (n - 400) / 160 frames: 1 020 here); 14 s, above 1 024 frames after the VAD; 0.7 s,
# too short to crop (67 frames: it counts in bad_clips on every path).
RAGGED_SAMPLES = [19200, 32000, 163600, 32000, 43200, 24000, 224000, 48000, 11200, 28800, 38400, 20800]
NEAR_1024, LONG, SHORT = 2, 6, 8              # positions of the three special clips
UNIFORM_CLIPS, UNIFORM_SAMPLES = 10, 24000    # ten clips of 1.5 s for the [n, L] methods
SMALL_CAP = 100_000                           # max_batch_samples at which the sample cap ends every batch of the ragged world
PIECES_CAP = 200_000                          # ... at which a host arena of the ragged world goes up in >= 3 pieces
DEFAULT_CAP = 64 * 1024 * 1024

# id -> pipeline options (crop_rng="device" throughout: the ragged methods need it)
CONFIGS = {
    "a": dict(channels=1, normalize=False, vad="absolute", K=1),                          # the reference's default
    "b": dict(channels=1, normalize=True, vad="absolute", K=1, preemph_cof=0.98),
    "c": dict(channels=1, normalize=True, vad="adaptive", K=3, pool="mean_l2"),
    "d": dict(channels=3, normalize=True, vad="absolute", K=2, pool="mean"),
    "e": dict(channels=3, normalize=False, vad=None, K=1),
}

_WORLDS = {}


def _frozen(x):
    x.setflags(write=False)
    return x


def ragged_world():
    """The dozen clips of different lengths (host int16 arrays, read-only), made once."""
    if "ragged" not in _WORLDS:
        from speaker_verification_amd import synth
        _WORLDS["ragged"] = [_frozen(synth.speaker_clip(k % 4 + 1, 40 + k, n)) for k, n in enumerate(RAGGED_SAMPLES)]
    return _WORLDS["ragged"]


def uniform_world():
    """[10, 24 000] int16, read-only."""
    if "uniform" not in _WORLDS:
        from speaker_verification_amd import synth
        _WORLDS["uniform"] = _frozen(np.stack([synth.speaker_clip(k % 3 + 1, 60 + k, UNIFORM_SAMPLES) for k in range(UNIFORM_CLIPS)]))
    return _WORLDS["uniform"]


def windows_world(window=24000, hop=12000, seconds=8):
    """The diarizer's use: one recording and overlapping windows over it -> (recording, offsets, lengths); offsets are
    multiples of 8 samples."""
    if "windows" not in _WORLDS:
        from speaker_verification_amd import synth
        rec = np.concatenate([synth.speaker_clip(1 + k % 2, 80 + k, 2 * FS) for k in range(seconds // 2)])
        offsets = np.arange(0, rec.size - window + 1, hop, dtype=np.int64)
        assert not (offsets % 8).any() and len(offsets) >= 9
        _WORLDS["windows"] = (_frozen(rec), _frozen(offsets), _frozen(np.full(len(offsets), window, dtype=np.int32)))
    return _WORLDS["windows"]


def equal_world(n=9, samples=FS):
    """Nine different clips of exactly 1 s (the wrap-around case)."""
    if "equal" not in _WORLDS:
        from speaker_verification_amd import synth
        _WORLDS["equal"] = [_frozen(synth.speaker_clip(k % 3 + 1, 90 + k, samples)) for k in range(n)]
    return _WORLDS["equal"]


def arena(clips):
    """Clips packed back to back in 16-byte-aligned slots -> (buffer, offsets, lengths), host arrays."""
    slots = [(len(x) + 7) // 8 * 8 for x in clips]
    offsets = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64)
    buf = np.zeros(int(sum(slots)), dtype=np.int16)
    for off, x in zip(offsets, clips):
        buf[off:off + len(x)] = x
    return buf, offsets, np.array([len(x) for x in clips], dtype=np.int32)


# ---- models and pipelines ---------------------------------------------------------------------------------------------
def model_for(channels):
    """One channel: the committed trained checkpoint (as tests/c3d2_f64_ref.py loads it); three: the seeded, perturbed model of
    tests/test_block12_addressing.py."""
    import torch
    from speaker_verification_amd.model import C3D2, perturb_inference_state, seeded_model
    if channels == 1:
        ck = torch.load(CHECKPOINT, map_location="cpu", weights_only=True)
        model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
        model.load_state_dict(ck["state_dict"])
        return model.eval()
    model = seeded_model(31, 4, 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), 32))
    return model.eval()


def make_pipe(cfg, micro_batch=1024):
    """The VerificationPipeline of a CONFIGS entry."""
    from speaker_verification_amd.pipeline import VerificationPipeline
    from speaker_verification_amd.vad import AdaptiveEnergyVad
    kw = dict(use_vad=cfg["vad"] is not None, normalize=cfg["normalize"], crop_rng="device", micro_batch=micro_batch,
              cubes_per_clip=cfg["K"], pool=cfg.get("pool", "mean"), preemph_cof=cfg.get("preemph_cof"))
    if cfg["vad"] == "adaptive":
        kw["vad"] = AdaptiveEnergyVad()
    return VerificationPipeline(model_for(cfg["channels"]), **kw)


def bad_count(pipe):
    return int(pipe.bad_clips.item())


def alone(pipe, clips, first=F):
    """Every clip in a launch of its own: embed(clip[None], first_utt = first + i) -> [n, 128]."""
    import torch
    return torch.cat([pipe.embed(np.asarray(x)[None], first_utt=first + i) for i, x in enumerate(clips)])


# ---- the uniform methods: pcm [n, L] -> [n, 128] -------------------------------------------------------------------------
def run_embed(pipe, pcm, first=F):
    return pipe.embed(pcm, first_utt=first)


def run_embed_host(pipe, pcm, first=F):
    return pipe.embed_host(np.array(pcm), first_utt=first)


def run_intermediates(pipe, pcm, first=F):
    """The copying VAD followed by `cubes` and `embed_cubes`."""
    emb, inter = pipe.embed(pcm, return_intermediates=True, first_utt=first)
    assert [(p["lo"], p["hi"]) for p in inter] == pipe.chunks(len(pcm))
    return emb


def run_cubes(pipe, pcm, first=F):
    """crops_and_cubes, then embed_cubes over ALL cubes in one launch, then the pool when K > 1."""
    _, cubes = pipe.crops_and_cubes(pcm, first_utt=first)
    if cubes.dim() == 6:
        each = pipe.embed_cubes(cubes.reshape((-1,) + tuple(cubes.shape[2:])))
        return pipe.eng.embedding_pool(each, rows_per_seg=cubes.shape[1], l2_rows=pipe._pool_flag())
    return pipe.embed_cubes(cubes)


UNIFORM_RUNNERS = {"embed": run_embed, "embed_host": run_embed_host, "intermediates": run_intermediates,
                   "crops_and_cubes + embed_cubes": run_cubes}


# ---- the ragged methods: list of clips -> [n, 128] -----------------------------------------------------------------------
def run_ragged(pipe, clips, cap=DEFAULT_CAP, first=F, crop_idx=None):
    return pipe.embed_ragged(list(clips), max_batch_samples=cap, first_utt=first, crop_idx=crop_idx)


def run_resident_host(pipe, clips, cap=DEFAULT_CAP, first=F, crop_idx=None):
    buf, offsets, lengths = arena(clips)
    return pipe.embed_ragged_resident(buf, offsets, lengths, max_batch_samples=cap, first_utt=first, crop_idx=crop_idx)


def run_resident_device(pipe, clips, cap=DEFAULT_CAP, first=F, crop_idx=None):
    buf, offsets, lengths = arena(clips)
    return pipe.embed_ragged_resident(pipe.eng.to_device(buf), offsets, lengths, max_batch_samples=cap, first_utt=first,
                                      crop_idx=crop_idx)


def run_resident_pieces(pipe, clips, cap=DEFAULT_CAP, first=F, crop_idx=None):
    """A host arena that goes up in at least three pieces (its own cap, whatever the caller's): the count is asserted."""
    buf, offsets, lengths = arena(clips)
    cap = min(cap, PIECES_CAP)
    assert buf.size > 2 * cap
    groups, pieces = pipe._upload_groups(offsets, lengths.astype(np.int64), buf.size, cap)
    assert len(groups) >= 3 and len(pieces) == len(groups), len(groups)
    return pipe.embed_ragged_resident(buf, offsets, lengths, max_batch_samples=cap, first_utt=first, crop_idx=crop_idx)


RAGGED_RUNNERS = {"embed_ragged": run_ragged, "resident, host arena": run_resident_host,
                  "resident, device arena": run_resident_device, "resident, host arena in pieces": run_resident_pieces}


def run_windows(pipe, first=F, device=False):
    """embed_ragged_resident on overlapping windows over one recording."""
    rec, offsets, lengths = windows_world()
    buf = pipe.eng.to_device(np.array(rec)) if device else np.array(rec)
    return pipe.embed_ragged_resident(buf, np.array(offsets), np.array(lengths), first_utt=first)


def windows_clips():
    rec, offsets, lengths = windows_world()
    return [rec[o:o + n] for o, n in zip(offsets, lengths)]


def drawn_crops(pipe, clips, first=F):
    """The crop starts the device draws for every clip ALONE, on the host: [n, 20], or [n, K, 20] with K cubes per clip; -1
    for a clip that is too short."""
    return np.concatenate([pipe.crops_and_cubes(np.asarray(x)[None], first_utt=first + i, want_cubes=False)
                           for i, x in enumerate(clips)])
