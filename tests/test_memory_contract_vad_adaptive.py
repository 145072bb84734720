"""The memory contract of include/svk.h (Conventions) for svk_vad_adaptive ("level-adaptive energy VAD"; csrc/vad.hip), in the form of
tests/test_memory_contract_ingest.py::test_vad_energy and on its batch: called directly on guarded arenas
(tests/memory_contract.py) in the environments A, B and C, placed for the vector paths and for the scalar ones, on the
short-clip kernel, the long-clip kernels and the general route, with every optional output present or NULL -- d_levels and
d_energy included (without d_energy the frame energies of the last two routes go through the handle's workspace, with it through
the caller's buffer).  Every comparison is on bytes, against the Engine wrapper's result for the same call on ordinary tensors.
The gaps between clips and the partial frame at a clip's end hold the payload pattern and are never read; d_energy from a clip's
frame count on keeps the prefill."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M                  # noqa: E402  (tests/ is on sys.path)
import test_memory_contract_ingest as ING    # noqa: E402  (the batch, the routes and the output variants of test_vad_energy)
import vad_adaptive_ref as R                 # noqa: E402

pytestmark = pytest.mark.gpu

I16, I32, I64, U8 = torch.int16, torch.int32, torch.int64, torch.uint8
P = R.DEFAULT
# (d_levels, d_energy) on top of ING.VAD_OUTPUTS' (d_seg, d_n_vad_frames, d_voiced, d_src_frame)
EXTRA_OUTPUTS = {"levels+energy": (1, 1), "levels": (1, 0), "energy": (0, 1), "neither": (0, 0)}
# every variant of the shared outputs with both extra ones, and every combination of the extra ones with all shared outputs
VARIANTS = [(v, "levels+energy") for v in ING.VAD_OUTPUTS] + [("all", e) for e in EXTRA_OUTPUTS if e != "levels+energy"] + [
    ("keep-only", "neither")]


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _reference(eng, pcm, offs, lens, fsamp, max_vf):
    longest = max_vf * fsamp + 1                     # the wrapper sizes its outputs from it: (2 longest - 1) // (2 fsamp) = max_vf
    kw = dict(lengths=lens.numpy(), offsets=offs, frame_samples=fsamp, ring_len=ING.RING, want_segments=True, longest=longest)
    copy = eng.vad_adaptive(pcm, P, compact=True, want_energy=True, **kw)
    index = eng.vad_adaptive(pcm, P, compact="index", **kw)
    assert tuple(copy["keep"].shape) == (len(lens), max_vf)
    ref = {k: copy[k].cpu() for k in ("keep", "seg", "n_vad_frames", "voiced", "voiced_len", "levels", "energy")}
    ref["src_frame"] = index["src_frame"].cpu()
    assert torch.equal(index["voiced_len"].cpu(), ref["voiced_len"]) and torch.equal(index["keep"].cpu(), ref["keep"])
    assert torch.equal(index["levels"].cpu(), ref["levels"])
    return ref


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("partial", ("data", "pattern"))
@pytest.mark.parametrize("odd", (0, 1), ids=("aligned-clips", "odd-offsets"))
@pytest.mark.parametrize("route,fsamp", ING.VAD_ROUTES, ids=("small", "split", "general-160", "general-100"))
def test_vad_adaptive(eng, monkeypatch, route, fsamp, odd, partial, placed):
    if route:
        monkeypatch.setenv("SVK_VAD_SPLIT", route)
    else:
        monkeypatch.delenv("SVK_VAD_SPLIT", raising=False)
    pcm, offs, lens = ING._vad_batch(fsamp, odd)
    frames = ING.CLIP_FRAMES
    n, total, max_vf = len(frames), pcm.numel(), max(frames) + ING.EXTRA
    ref = _reference(eng, pcm, offs, lens, fsamp, max_vf)
    assert ref["n_vad_frames"].tolist() == list(frames) and int(ref["voiced_len"][3]) > int(ref["voiced_len"][0]) > 0
    assert int(ref["seg"][3].max()) == 1, "the long clip holds two segments"
    for u in range(n):                                # the wrapper's result is the rule's (the Python-integer reference)
        want = R.vad(pcm[int(offs[u]):int(offs[u]) + int(lens[u])].numpy(), fsamp, ING.RING, P)
        assert tuple(ref["levels"][u].tolist()) == want["levels"] and ref["energy"][u, :frames[u]].tolist() == want["energy"]
    kept = [int(v) // fsamp for v in ref["voiced_len"]]
    live, in_voiced = torch.zeros(total, dtype=torch.bool), np.zeros(total, dtype=bool)
    for u in range(n):
        o = int(offs[u])
        live[o:o + (int(lens[u]) if partial == "data" else frames[u] * fsamp)] = True
        in_voiced[o:o + kept[u] * fsamp] = True
    past = np.arange(max_vf)[None, :] >= np.asarray(frames)[:, None]
    past_kept = np.arange(max_vf)[None, :] >= np.asarray(kept)[:, None]
    for variant, extra in VARIANTS:
        w_seg, w_nvf, w_voiced, w_src = ING.VAD_OUTPUTS[variant]
        w_levels, w_energy = EXTRA_OUTPUTS[extra]
        for env in M.ENV_NAMES:
            c = M.Contract(eng, env, scalar=placed == "scalar")
            dp, do, dl = c.input_where("d_pcm", pcm, live), c.input("d_offsets", offs), c.input("d_lengths", lens)
            keep = c.output("d_keep", U8, (n, max_vf))
            seg = c.output("d_seg", I32, (n, max_vf)) if w_seg else None
            nvf = c.output("d_n_vad_frames", I32, (n,)) if w_nvf else None
            voiced = c.output("d_voiced", I16, (total,)) if w_voiced else None
            vlen = c.output("d_voiced_len", I32, (n,)) if w_voiced or w_src else None
            src = c.output("d_src_frame", I32, (n, max_vf)) if w_src else None
            levels = c.output("d_levels", I64, (n, 3)) if w_levels else None
            energy = c.output("d_energy", I64, (n, max_vf)) if w_energy else None
            c.call(eng.lib.svk_vad_adaptive, dp, do, dl, 0, 0, n, fsamp, ING.RING, ING.RING_THRESH, P.floor_q16, P.peak_q16,
                   P.above_floor_q16, P.below_peak_q16, P.min_threshold, max_vf, keep, seg, nvf, voiced, vlen, src, levels, energy)
            what = "svk_vad_adaptive %s frame %d %s partial frame %s outputs %s, %s, %s, environment %s" % (
                route or "small", fsamp, "odd" if odd else "aligned", partial, variant, extra, placed, env)
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
            if levels is not None:
                M.same_bits(levels.bits(), M.bits(ref["levels"]), what + ": d_levels")
            if energy is not None:
                got = energy.bits()
                M.same_bits(got[~past], M.bits(ref["energy"])[~past], what + ": d_energy")
                M.keeps_prefill(energy, got[past], what + ": d_energy from the clip's frame count on")
