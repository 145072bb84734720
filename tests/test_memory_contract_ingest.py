"""The memory contract of include/svk.h (Conventions) for svk_vad_energy (vad.hip) and svk_ingest_resample (ingest.hip), called
directly on guarded arenas (tests/memory_contract.py) in the environments A, B and C, placed for the vector paths (256-byte
boundaries) and for the scalar ones (one element past a boundary).  Every comparison is on bytes, against the Engine wrapper's
result for the same call on ordinary tensors; PCM the header lets no call read -- the gaps between clips, the padding of strided
rows, the samples past a clip's length and, for the VAD, the partial frame at a clip's end -- holds the payload pattern."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

F32, I16, I32, I64, U8 = torch.float32, torch.int16, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


# ---- svk_vad_energy ----------------------------------------------------------------------------------------------------------
RING, RING_THRESH, THRESHOLD = 3, 2, 100000          # three voiced frames in a row trigger; mean square above 1e5 is voiced
LOUD = {1: ((0, 1),), 12: ((2, 10),), 40: ((3, 13), (20, 31)), 0: ()}        # frames of a clip -> its loud runs [a, b)
CLIP_FRAMES = (12, 0, 1, 40)
EXTRA = 3                                             # max_vad_frames exceeds every clip's frame count by this much


def _vad_batch(fsamp, odd):
    """Four clips in one flat buffer, gaps between them, the last one flush against the end; every clip ends in a partial
    frame.  -> (pcm [total] int16, offsets int64, lengths int32, frames per clip)."""
    g = torch.Generator().manual_seed(fsamp + odd)
    offs, lens, at = [], [], 5 if odd else 8
    for i, k in enumerate(CLIP_FRAMES):
        offs.append(at)
        lens.append(k * fsamp + (fsamp // 3 + i if k else fsamp // 2))          # a partial last frame
        at += lens[-1] + 24 + 2 * i
        at += (1 - at % 2) if odd else (-at) % 8
        assert (at % 2 == 1) if odd else (at % 8 == 0)
    total = offs[-1] + lens[-1]
    pcm = torch.randint(-9, 10, (total,), generator=g, dtype=I32)
    for off, k in zip(offs, CLIP_FRAMES):
        for a, b in LOUD[k]:
            pcm[off + a * fsamp:off + b * fsamp] = torch.randint(-3000, 3001, ((b - a) * fsamp,), generator=g, dtype=I32)
    for off, n, k in zip(offs, lens, CLIP_FRAMES):                               # the partial frame is loud: if the rule
        pcm[off + k * fsamp:off + n] = 20000                                     # looked at it, it would count as voiced
    return pcm.to(I16), torch.tensor(offs, dtype=I64), torch.tensor(lens, dtype=I32)


def _vad_reference(eng, pcm, offs, lens, fsamp, max_vf):
    longest = max_vf * fsamp + 1                     # the wrapper sizes its outputs from it: (2 longest - 1) // (2 fsamp) = max_vf
    kw = dict(lengths=lens.numpy(), offsets=offs, frame_samples=fsamp, ring_len=RING, want_segments=True, longest=longest)
    copy = eng.vad_energy(pcm, THRESHOLD, compact=True, **kw)
    index = eng.vad_energy(pcm, THRESHOLD, compact="index", **kw)
    assert tuple(copy["keep"].shape) == (len(lens), max_vf)
    ref = {k: copy[k].cpu() for k in ("keep", "seg", "n_vad_frames", "voiced", "voiced_len")}
    ref["src_frame"] = index["src_frame"].cpu()
    assert torch.equal(index["voiced_len"].cpu(), ref["voiced_len"]) and torch.equal(index["keep"].cpu(), ref["keep"])
    return ref


# which optional outputs a variant passes: (d_seg, d_n_vad_frames, d_voiced, d_src_frame)
VAD_OUTPUTS = {"all": (1, 1, 1, 1), "no-seg": (0, 1, 1, 1), "no-count": (1, 0, 1, 1), "index-only": (1, 1, 0, 1),
               "copy-only": (1, 1, 1, 0), "keep-only": (0, 0, 0, 0)}
# (SVK_VAD_SPLIT, frame_samples): the small kernel, the split trio, vad_kernel with a frame of whole 16-byte vectors (its
# one-vector-per-lane loop on aligned clips, its general loop on the others) and with a frame that is none
VAD_ROUTES = (("", 160), ("1", 160), ("2", 160), ("2", 100))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("partial", ("data", "pattern"))
@pytest.mark.parametrize("odd", (0, 1), ids=("aligned-clips", "odd-offsets"))
@pytest.mark.parametrize("route,fsamp", VAD_ROUTES, ids=("small", "split", "one-kernel-160", "one-kernel-100"))
def test_vad_energy(eng, monkeypatch, route, fsamp, odd, partial, placed):
    """The partial frame at a clip's end is never read (vad.py:54 yields whole frames only): with the pattern in its place the
    results are the same bytes.  d_keep is 0 and d_seg -1 from a clip's frame count to max_vad_frames; d_voiced beyond the kept
    samples (the gaps between clips included) and d_src_frame beyond the kept count keep the prefill."""
    if route:
        monkeypatch.setenv("SVK_VAD_SPLIT", route)
    else:
        monkeypatch.delenv("SVK_VAD_SPLIT", raising=False)
    pcm, offs, lens = _vad_batch(fsamp, odd)
    n, total, max_vf = len(CLIP_FRAMES), pcm.numel(), max(CLIP_FRAMES) + EXTRA
    ref = _vad_reference(eng, pcm, offs, lens, fsamp, max_vf)
    assert ref["n_vad_frames"].tolist() == list(CLIP_FRAMES) and int(ref["voiced_len"][3]) > int(ref["voiced_len"][0]) > 0
    assert int(ref["seg"][3].max()) == 1, "the long clip holds two segments"
    kept = [int(v) // fsamp for v in ref["voiced_len"]]
    live, in_voiced = torch.zeros(total, dtype=torch.bool), np.zeros(total, dtype=bool)
    for u in range(n):
        o = int(offs[u])
        live[o:o + (int(lens[u]) if partial == "data" else CLIP_FRAMES[u] * fsamp)] = True
        in_voiced[o:o + kept[u] * fsamp] = True
    past = np.arange(max_vf)[None, :] >= np.asarray(CLIP_FRAMES)[:, None]
    past_kept = np.arange(max_vf)[None, :] >= np.asarray(kept)[:, None]
    for variant, (w_seg, w_nvf, w_voiced, w_src) in VAD_OUTPUTS.items():
        for env in M.ENV_NAMES:
            c = M.Contract(eng, env, scalar=placed == "scalar")
            dp, do, dl = c.input_where("d_pcm", pcm, live), c.input("d_offsets", offs), c.input("d_lengths", lens)
            keep = c.output("d_keep", U8, (n, max_vf))
            seg = c.output("d_seg", I32, (n, max_vf)) if w_seg else None
            nvf = c.output("d_n_vad_frames", I32, (n,)) if w_nvf else None
            voiced = c.output("d_voiced", I16, (total,)) if w_voiced else None
            vlen = c.output("d_voiced_len", I32, (n,)) if w_voiced or w_src else None
            src = c.output("d_src_frame", I32, (n, max_vf)) if w_src else None
            c.call(eng.lib.svk_vad_energy, dp, do, dl, 0, 0, n, fsamp, RING, RING_THRESH, THRESHOLD, max_vf, keep, seg, nvf, voiced,
                   vlen, src)
            what = "svk_vad_energy %s frame %d %s partial frame %s outputs %s, %s, environment %s" % (
                route or "small", fsamp, "odd" if odd else "aligned", partial, variant, placed, env)
            M.same_bits(keep.bits(), M.bits(ref["keep"]), what + ": d_keep")
            assert not keep.bits()[past].any(), what + ": d_keep past the clip's frames is 0"
            if seg is not None:
                M.same_bits(seg.bits(), M.bits(ref["seg"]), what + ": d_seg")
                assert (seg.tensor.cpu().numpy()[past] == -1).all(), what + ": d_seg past the clip's frames is -1"
            if nvf is not None:
                M.same_bits(nvf.bits(), M.bits(ref["n_vad_frames"]), what + ": d_n_vad_frames")
            if vlen is not None:
                M.same_bits(vlen.bits(), M.bits(ref["voiced_len"]), what + ": d_voiced_len")
            if voiced is not None:
                got = voiced.bits()
                M.same_bits(got[in_voiced], M.bits(ref["voiced"])[in_voiced], what + ": d_voiced, the kept samples")
                M.keeps_prefill(voiced, got[~in_voiced], what + ": d_voiced beyond the kept samples")
            if src is not None:
                got = src.bits()
                M.same_bits(got[~past_kept], M.bits(ref["src_frame"])[~past_kept], what + ": d_src_frame")
                M.keeps_prefill(src, got[past_kept], what + ": d_src_frame beyond the kept count")


# ---- svk_ingest_resample -----------------------------------------------------------------------------------------------------
CLIP_IN, IN_STRIDE, IN_LEN = 1900, 1907, (1203, 0, 1900)       # the last clip is full: its last frame lies against the guard
# (up, down): the two decimation instances (20 down + 1 taps) and the general kernel
RATIOS = ((1, 2), (1, 3), (160, 147), (1, 4))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("cut", (0, 37), ids=("natural-count", "cut-short"))
@pytest.mark.parametrize("out_dtype", ("f32", "i16"))
@pytest.mark.parametrize("n_ch", (1, 2, 3))
@pytest.mark.parametrize("up,down", RATIOS, ids=["%d-%d" % r for r in RATIOS])
def test_ingest_resample(eng, up, down, n_ch, out_dtype, cut, placed):
    """in_stride > clip_in and d_in_len shorter than clip_in: the padding and the frames beyond a clip's length hold the
    pattern; out_stride > clip_out: the padding between the output rows keeps the prefill (Contract.verify)."""
    from speaker_verification_amd.ingest import resample_taps
    n = len(IN_LEN)
    taps = torch.from_numpy(np.asarray(resample_taps(up, down), dtype=np.float32))
    assert taps.numel() == 20 * max(up, down) + 1
    g = torch.Generator().manual_seed(up + down + n_ch)
    frames = (n - 1) * IN_STRIDE + CLIP_IN
    pcm = torch.randint(-20000, 20001, (frames, n_ch), generator=g, dtype=I32).to(I16)
    rows = torch.stack([pcm[u * IN_STRIDE:u * IN_STRIDE + CLIP_IN] for u in range(n)])           # [n][clip_in][n_ch]
    lens = torch.tensor(IN_LEN, dtype=I32)
    want, want_len = eng.resample(rows if n_ch > 1 else rows[:, :, 0], up, down, taps.numpy(), IN_LEN, out_dtype)
    natural = (CLIP_IN * up + down - 1) // down
    clip_out, out_stride = natural - cut, natural - cut + 5
    assert tuple(want.shape) == (n, natural)
    live = torch.zeros((frames, n_ch), dtype=torch.bool)
    for u, k in enumerate(IN_LEN):
        live[u * IN_STRIDE:u * IN_STRIDE + k] = True
    dt = F32 if out_dtype == "f32" else I16
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        dp, dl, dh = c.input_where("d_pcm", pcm, live), c.input("d_in_len", lens), c.input("d_taps", taps)
        out, out_len = c.output("d_out", dt, (n, clip_out), stride=out_stride), c.output("d_out_len", I32, (n,))
        c.call(eng.lib.svk_ingest_resample, dp, n_ch, IN_STRIDE, dl, CLIP_IN, n, dh, taps.numel(), up, down, out,
               1 if out_dtype == "f32" else 0, out_stride, clip_out, out_len)
        what = "svk_ingest_resample %d/%d %d channels %s clip_out %d, %s, environment %s" % (up, down, n_ch, out_dtype, clip_out, placed, env)
        M.same_bits(out.bits(), M.bits(want[:, :clip_out]), what + ": d_out")
        M.same_bits(out_len.bits(), M.bits(torch.clamp(want_len.cpu(), max=clip_out)), what + ": d_out_len")


@pytest.mark.parametrize("placed", M.PLACED)
def test_ingest_resample_of_a_batch_without_frames_writes_only_the_lengths(eng, placed):
    """clip_out == 0: d_out_len becomes 0 for every clip, nothing else is touched and no other pointer is looked at."""
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        out, out_len = c.output("d_out", F32, (3, 4)), c.output("d_out_len", I32, (3,))
        c.call(eng.lib.svk_ingest_resample, None, 1, 0, None, 0, 3, None, 41, 1, 2, out, 1, 4, 0, out_len)
        what = "svk_ingest_resample clip_out 0, %s, environment %s" % (placed, env)
        assert not out_len.bits().any(), what + ": d_out_len"
        M.keeps_prefill(out, out.bits(), what + ": d_out")
