"""One clip, one embedding: a clip's embedding is a function of the clip, its global index and the pipeline's
options.  It does not depend on the other clips of the launch, on the batch cuts (micro_batch, max_batch_samples, upload
pieces), on the ring's wrap-around or on which embed method carried it -- to the last bit.

The cases, the configurations and one runner per path are stated in tests/embed_paths.py.  Every comparison is torch.equal
against the clip embedded ALONE (a launch of one clip); one test anchors those rows to the CPU oracle chain, so that the
equalities cannot all be wrong together.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import embed_paths as P               # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

_PIPES, _ALONE = {}, {}


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def pipe_of(cid):
    """One pipeline per configuration, shared by the tests (they set its micro_batch)."""
    if cid not in _PIPES:
        _PIPES[cid] = P.make_pipe(P.CONFIGS[cid])
    return _PIPES[cid]


def alone_of(cid, world):
    """-> (the clips' embeddings alone [n, 128], how many of them counted in bad_clips), computed once per configuration."""
    if (cid, world) not in _ALONE:
        pipe = pipe_of(cid)
        clips = {"ragged": P.ragged_world, "uniform": lambda: list(P.uniform_world()), "windows": P.windows_clips}[world]()
        before = P.bad_count(pipe)
        rows = P.alone(pipe, clips)
        assert bool(torch.isfinite(rows).all())
        _ALONE[cid, world] = (rows, P.bad_count(pipe) - before)
    return _ALONE[cid, world]


def _mismatch(got, want):
    """Rows that differ, and by how much (for the assertion message)."""
    rows = (got != want).any(1).nonzero().flatten().tolist()
    return "rows %s differ, max |diff| %.3g" % (rows, float((got - want).abs().max()))


def test_the_ragged_world_meets_every_cut(eng):
    """The module's own premises: the near-1 024 clip has 1 000 .. 1 024 frames in the front end's count, the long clip more
    than 1 024 frames AFTER the VAD, the short one too few to crop; the small sample cap, not the clip cap, ends every batch."""
    pipe = pipe_of("b")
    clips = P.ragged_world()
    lengths = np.array([len(x) for x in clips], dtype=np.int64)
    assert 1000 < pipe.spec.num_frames(int(lengths[P.NEAR_1024])) <= 1024
    assert sorted(lengths.tolist()).count(32000) == 2
    dev = eng.to_device(np.array(clips[P.LONG])[None])
    _, n_frames = pipe.features(dev, *pipe.vad(dev))
    assert int(n_frames[0]) > 1024
    assert pipe.spec.num_frames(int(lengths[P.SHORT])) <= 80
    pipe.micro_batch = 64
    plan = pipe._ragged_batches(lengths, P.SMALL_CAP)
    assert len(plan) > 3 and all(total <= P.SMALL_CAP or len(ids) == 1 for ids, total in plan)
    assert [ids for ids, _ in plan] != [ids for ids, _ in pipe._ragged_batches(lengths, P.DEFAULT_CAP)]


def test_a_batch_of_clips_too_short_to_crop(eng):
    """With one clip per batch the 0.7 s clip is a batch of its own, whose 67 feature rows are fewer than a crop: the gathers
    refuse such a buffer and embed_ragged used to raise.  The ragged front end now sizes the feature buffer to at least one
    crop; a list of nothing but short clips gives the rows the clips give alone and counts every one of them."""
    from speaker_verification_amd import synth
    pipe = pipe_of("b")
    pipe.micro_batch = 4
    clips = [synth.speaker_clip(1 + k, 70 + k, n) for k, n in enumerate((11200, 9600, 12000))]
    assert max(pipe.spec.num_frames(len(x)) for x in clips) < 80
    before = P.bad_count(pipe)
    want = P.alone(pipe, clips)
    assert P.bad_count(pipe) - before == 3
    for name in ("embed_ragged", "resident, device arena"):
        before = P.bad_count(pipe)
        got = P.RAGGED_RUNNERS[name](pipe, clips)
        assert P.bad_count(pipe) - before == 3 and torch.equal(got, want), name


@pytest.mark.parametrize("cap", [P.DEFAULT_CAP, P.SMALL_CAP], ids=["default cap", "sample cap"])
@pytest.mark.parametrize("micro_batch", [1, 4, 64])
@pytest.mark.parametrize("cid", list(P.CONFIGS))
def test_alone_against_together(eng, cid, micro_batch, cap):
    """Row i of every ragged runner called with first_utt = F is clip i embedded alone with first_utt = F + i, bit for bit,
    and bad_clips advances by the same count on every path."""
    pipe = pipe_of(cid)
    want, bad = alone_of(cid, "ragged")
    assert bad >= 1                                                    # the 0.7 s clip, at least
    pipe.micro_batch = micro_batch
    clips = P.ragged_world()
    for name, run in P.RAGGED_RUNNERS.items():
        before = P.bad_count(pipe)
        got = run(pipe, clips, cap)
        assert P.bad_count(pipe) - before == bad, (name, P.bad_count(pipe) - before, bad)
        assert torch.equal(got, want), "%s, micro_batch %d: %s" % (name, micro_batch, _mismatch(got, want))


@pytest.mark.parametrize("cid", list(P.CONFIGS))
def test_windows_over_one_recording(eng, cid):
    """The diarizer's arena: overlapping windows over one recording, on the host and on the device."""
    pipe = pipe_of(cid)
    want, bad = alone_of(cid, "windows")
    pipe.micro_batch = 4
    for device in (False, True):
        before = P.bad_count(pipe)
        got = P.run_windows(pipe, device=device)
        assert P.bad_count(pipe) - before == bad
        assert torch.equal(got, want), "device arena %s: %s" % (device, _mismatch(got, want))


@pytest.mark.parametrize("micro_batch", [1, 3, 4, 16])
@pytest.mark.parametrize("cid", list(P.CONFIGS))
def test_the_uniform_methods(eng, cid, micro_batch):
    """embed, embed_host, the intermediates form and crops_and_cubes + embed_cubes on ten uniform clips: each row is the clip
    alone.  With micro_batch = 3 cubes' worth of clips the last chunk is shifted back and recomputes two clips next to another
    neighbour; the plan is asserted."""
    pipe = pipe_of(cid)
    want, bad = alone_of(cid, "uniform")
    assert bad == 0
    K = P.CONFIGS[cid]["K"]
    pipe.micro_batch = micro_batch * K                                 # micro_batch counts cubes: that many CLIPS per chunk
    if micro_batch == 3:
        assert pipe.chunks(P.UNIFORM_CLIPS) == [(0, 3), (3, 6), (6, 9), (7, 10)]
    pcm = P.uniform_world()
    before = P.bad_count(pipe)
    for name, run in P.UNIFORM_RUNNERS.items():
        got = run(pipe, pcm)
        assert torch.equal(got, want), "%s, %d clips per chunk: %s" % (name, micro_batch, _mismatch(got, want))
    assert P.bad_count(pipe) == before


@pytest.mark.parametrize("cid", list(P.CONFIGS))
def test_order(eng, cid):
    """Crop starts given on the host ([n, 20] or [n, K, 20]): a permuted list returns the permuted rows, for the list form and
    the resident form; with the starts the device draws for each clip alone, the rows are the clips alone as well."""
    pipe = pipe_of(cid)
    want, _ = alone_of(cid, "ragged")
    pipe.micro_batch = 4
    clips = P.ragged_world()
    crops = P.drawn_crops(pipe, clips)
    K = P.CONFIGS[cid]["K"]
    assert crops.shape == ((len(clips), 20) if K == 1 else (len(clips), K, 20)) and (crops[P.SHORT] == -1).all()
    perm = np.random.default_rng(5).permutation(len(clips))
    assert (perm != np.arange(len(clips))).any()
    for name in ("embed_ragged", "resident, device arena"):
        run = P.RAGGED_RUNNERS[name]
        base = run(pipe, clips, crop_idx=crops)
        assert torch.equal(base, want), "%s with given crops: %s" % (name, _mismatch(base, want))
        got = run(pipe, [clips[p] for p in perm], crop_idx=crops[perm])
        assert torch.equal(got, base[torch.from_numpy(perm).to(base.device)]), name


@pytest.mark.parametrize("channels,K", [(1, 1), (1, 3), (3, 2)])
def test_the_wrap_is_reached(eng, monkeypatch, channels, K):
    """Nine equal clips in batches of three through a ring of eight clips' cubes: the third push straddles the ring's end and
    gathers in two calls, the second into the ring's head with stats[first:].  normalize=True, so that slice carries weight."""
    from speaker_verification_amd.pipeline import VerificationPipeline
    cfg = dict(channels=channels, normalize=True, vad="absolute", K=K)
    pipe = P.make_pipe(cfg, micro_batch=4 * K)
    clips = P.equal_world()
    want = P.alone(pipe, clips)
    assert P.bad_count(pipe) == 0
    cap = 3 * len(clips[0])
    plan = pipe._ragged_batches(np.array([len(x) for x in clips]), cap)
    assert [len(ids) for ids, _ in plan] == [3, 3, 3]
    calls, per_push = [0], []
    for name in ("cube_gather", "cube_gather_delta"):
        real = getattr(eng, name)

        def spy(*a, _real=real, **kw):
            calls[0] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(eng, name, spy)
    real_push = VerificationPipeline._CubeRing.push

    def push(self, *a, **kw):
        before = calls[0]
        assert self.step == 4 * K and self.cap == 8 * K
        real_push(self, *a, **kw)
        per_push.append(calls[0] - before)
    monkeypatch.setattr(VerificationPipeline._CubeRing, "push", push)
    assert pipe.eng is eng
    got = P.run_ragged(pipe, clips, cap)
    assert per_push == [1, 1, 2], per_push                             # the third push wrapped
    assert torch.equal(got, want), _mismatch(got, want)
    assert P.bad_count(pipe) == 0


def test_alone_rows_against_the_cpu_oracle(eng):
    """Configuration b's alone rows against the CPU oracle chain (vad -> / 32768 -> preemphasis -> lmfe -> cmvn -> cube at the
    device-drawn crops -> C3D2) at the bar test_ragged_embeddings_of_very_long_clips uses, 5e-5 of the embedding scale.  The
    clip that is too short to crop is a cube of zeros on both sides."""
    from oracle import model_ref, speechpy_ref as ref, vad_ref
    from speaker_verification_amd import constants as c
    pipe = pipe_of("b")
    got, _ = alone_of("b", "ragged")
    got = got.cpu().numpy()
    cubes = []
    for i, x in enumerate(P.ragged_world()):
        _, _, voiced = vad_ref.vad_energy(np.asarray(x), 16000, c.VAD_FRAME_MS, c.VAD_PADDING_MS, c.VAD_ENERGY_THRESHOLD)
        feat = ref.cmvn(ref.lmfe(ref.preemphasis(voiced / 32768.0, cof=0.98), 16000, c.FRAME_LEN, c.FRAME_STEP, c.NUM_COEF,
                                 c.NUM_FFT), variance_normalization=True)
        crops = eng.draw_crops(np.array([feat.shape[0]], dtype=np.int32), c.CUBE_CROPS, c.CUBE_FRAMES, pipe.crop_seed, 0,
                               utt_index=np.array([P.F + i])).cpu().numpy()[0]
        if i == P.SHORT:
            assert (crops == -1).all()
            cubes.append(np.zeros((1, c.CUBE_CROPS, c.CUBE_FRAMES, c.NUM_COEF), dtype=np.float32))
        else:
            assert crops.min() >= 0 and crops.max() + c.CUBE_FRAMES <= feat.shape[0]
            cubes.append(np.asarray(model_ref.feature_cube(feat, crops), dtype=np.float32))
    state = {k: v.detach().cpu() for k, v in pipe.model.state_dict().items()}
    want = model_ref.c3d2_embed(state, np.stack(cubes)).numpy()
    scale = np.abs(want).max(1, keepdims=True)
    print("alone rows vs the CPU oracle: max |diff| / scale %.2e (bar 5e-5)" % float((np.abs(got - want) / scale).max()))
    assert np.all(np.abs(got - want) <= 5e-5 * scale)
