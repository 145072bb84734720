"""svk_vad_adaptive (include/svk.h, "level-adaptive energy VAD") against the Python-integer reference of tests/vad_adaptive_ref.py on every kernel route:
the short-clip kernel, the long-clip kernels (SVK_VAD_SPLIT=1 and clips beyond 512 frames) and the general route
(SVK_VAD_SPLIT=2 and frame lengths that are no multiple of 8 or exceed 512).  Integer arithmetic: every comparison is exact.

  * the case list (tests/test_vad_adaptive_host.py holds it to reaching the edges and to catching every mutant of the rule):
    levels, energy, keep, seg, n_vad_frames, voiced_len, voiced[:voiced_len] and src_frame equal the reference's, ragged clips
    at offsets 0, 1, 4 and 7 samples past a multiple of 8, nothing written outside a clip's own slot of `voiced`;
  * below_peak_q16 = 0 is svk_vad_energy with threshold = min_threshold, bit for bit, on clips with frames exactly at the
    absolute threshold;
  * gain invariance on the synthetic speakers, and the regression the feature answers: the absolute rule keeps no frame of a
    clip recorded 24 dB down;
  * every refusal returns its code, names the parameter and writes nothing.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import vad_adaptive_ref as R           # noqa: E402  (tests/ is on sys.path)
import vad_cases as V                  # noqa: E402

pytestmark = pytest.mark.gpu

RESIDUES = (0, 1, 4, 7)                # clip offsets mod 8 inside one batch


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def set_route(monkeypatch, route):
    if route is None:
        monkeypatch.delenv("SVK_VAD_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SVK_VAD_SPLIT", route)


def lay_out(clips, seed):
    """Ragged clips in one buffer, loud where no clip lies.  -> (host int16, offsets, lengths, mask of the clips' own samples)."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(c) for c in clips], dtype=np.int32)
    offs, cur = [], 0
    for i, n in enumerate(lens):
        cur += (RESIDUES[i % 4] - cur) % 8
        offs.append(cur)
        cur += int(n) + 3
    total = cur + 8
    host = rng.choice(np.array([-30000, 30000], dtype=np.int16), total)
    inside = np.zeros(total, dtype=bool)
    for c, o in zip(clips, offs):
        host[o:o + len(c)] = c
        inside[o:o + len(c)] = True
    return host, np.array(offs, dtype=np.int64), lens, inside


def run(eng, clips, fsamp, ring, p, compact, seed=0):
    """One Engine.vad_adaptive call on the laid-out clips -> (dict of host arrays, offsets, inside mask)."""
    host, offs, lens, inside = lay_out(clips, seed)
    x = torch.from_numpy(host).to(eng.device)
    kw = dict(frame_samples=fsamp, ring_len=ring, want_segments=True, compact=compact, lengths=lens, offsets=offs, want_energy=True)
    vo = None
    if compact is True:
        vo = torch.full((len(host),), V.SENTINEL, dtype=torch.int16, device=eng.device)
        kw.update(voiced_out=vo)
    r = eng.vad_adaptive(x, p, **kw)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in ("keep", "seg", "n_vad_frames", "voiced_len", "levels", "energy")}
    if compact is True:
        assert r["voiced"].data_ptr() == vo.data_ptr()
        out["voiced"] = vo.cpu().numpy()
    else:
        assert r["voiced"] is None
        out["src_frame"] = r["src_frame"].cpu().numpy()
    return out, offs, inside


@pytest.mark.parametrize("compact", (True, "index"), ids=("copy", "index"))
@pytest.mark.parametrize("case", R.gpu_cases(), ids=[c.name for c in R.gpu_cases()])
def test_ragged_batch_equals_the_reference(eng, monkeypatch, case, compact):
    set_route(monkeypatch, case.route)
    ref = R.reference(case)
    got, offs, inside = run(eng, case.clips, case.fsamp, case.ring, case.params, compact, seed=len(case.clips))
    max_vf = got["keep"].shape[1]
    assert max_vf >= max(len(r["keep"]) for r in ref)
    if compact is True:
        assert (got["voiced"][~inside] == V.SENTINEL).all(), "svk_vad_adaptive wrote outside a clip's own slot of `voiced`"
    for u, (r, o) in enumerate(zip(ref, offs)):
        nf, what = len(r["keep"]), "%s, clip %d (%d frames)" % (case.name, u, len(r["keep"]))
        assert got["n_vad_frames"][u] == nf, what
        assert tuple(int(v) for v in got["levels"][u]) == r["levels"], what + ": levels"
        assert [int(v) for v in got["energy"][u, :nf]] == r["energy"], what + ": energy"
        np.testing.assert_array_equal(got["keep"][u], np.concatenate([r["keep"], np.zeros(max_vf - nf, dtype=bool)]).astype(np.uint8),
                                      err_msg=what + ": keep")
        np.testing.assert_array_equal(got["seg"][u], np.concatenate([r["seg"], np.full(max_vf - nf, -1, dtype=np.int32)]),
                                      err_msg=what + ": seg")
        kept = int(r["keep"].sum())
        assert got["voiced_len"][u] == kept * case.fsamp == len(r["voiced"]), what
        if compact is True:
            np.testing.assert_array_equal(got["voiced"][o:o + kept * case.fsamp], r["voiced"], err_msg=what + ": voiced")
        else:
            np.testing.assert_array_equal(got["src_frame"][u, :kept], r["src_frame"], err_msg=what + ": src_frame")


@pytest.mark.parametrize("compact", (True, "index"), ids=("copy", "index"))
@pytest.mark.parametrize("route,fsamp,counts", [(None, 160, (0, 1, 64, 65, 130, 512)), ("1", 8, (0, 1, 65, 513, 1100)),
                                                ("2", 100, (0, 1, 64, 129)), (None, 480, (0, 1, 33, 127)), ("2", 160, (1, 65, 513))])
def test_without_a_peak_term_it_is_the_absolute_rule(eng, monkeypatch, route, fsamp, counts, compact):
    """below_peak_q16 = 0: T = min_threshold frame_samples for every clip, and every output equals svk_vad_energy's with
    threshold = min_threshold.  The clips hold frames exactly at that threshold and one step above it."""
    set_route(monkeypatch, route)
    a = 500 if fsamp >= 100 else 3
    clips = [c for c, _ in V.clips_for(fsamp, 10, a * a, counts, seed=fsamp)]
    host, offs, lens, _ = lay_out(clips, 1)
    x = torch.from_numpy(host).to(eng.device)
    kw = dict(frame_samples=fsamp, ring_len=10, want_segments=True, compact=compact, lengths=lens, offsets=offs)
    want = eng.vad_energy(x, a * a, **kw)
    got = eng.vad_adaptive(x, R.Params(6554, 62259, 655360, 0, a * a), **kw)
    torch.cuda.synchronize()
    for k in ("keep", "seg", "n_vad_frames", "voiced_len"):
        assert torch.equal(got[k], want[k]), k
    assert int(want["keep"].sum()) > 0 and (got["levels"][:, 2] == a * a * fsamp).all()
    vlen = want["voiced_len"].cpu().numpy()
    if compact is True:
        g, w = got["voiced"].cpu().numpy(), want["voiced"].cpu().numpy()
        for o, n in zip(offs, vlen):
            np.testing.assert_array_equal(g[o:o + n], w[o:o + n])
    else:
        g, w = got["src_frame"].cpu().numpy(), want["src_frame"].cpu().numpy()
        for u, n in enumerate(vlen // fsamp):
            np.testing.assert_array_equal(g[u, :n], w[u, :n])


def test_gain_invariance_and_the_quiet_clip_the_absolute_rule_drops(eng, monkeypatch):
    """q = a synthetic speaker's clip 24 dB down, and 8 q: the same keep, seg and src_frame under the default parameters, the
    levels of 8 q within [64 L, 64 L + 63] of q's -- while the absolute rule at the default threshold keeps no frame of q."""
    from speaker_verification_amd import constants as c, synth
    from speaker_verification_amd.vad import AdaptiveEnergyVad
    set_route(monkeypatch, None)
    q = np.stack([synth.speaker_clip(s, u) >> 4 for s, u in ((0, 0), (1, 2), (5, 1))])
    assert np.abs(q).max() * 8 <= 32767
    vad = AdaptiveEnergyVad()
    a = eng.vad_adaptive(q, vad, compact="index", want_segments=True)
    b = eng.vad_adaptive((q * 8).astype(np.int16), vad, compact="index", want_segments=True)
    absolute = eng.vad_energy(q, c.VAD_ENERGY_THRESHOLD, compact="index")
    torch.cuda.synchronize()
    assert int(absolute["keep"].sum()) == 0 and int(absolute["voiced_len"].sum()) == 0
    kept = a["keep"].sum(dim=1).cpu().numpy()
    assert (kept >= 60).all() and (kept <= 99).all(), kept
    for k in ("keep", "seg", "voiced_len"):
        assert torch.equal(a[k], b[k]), k
    for u, n in enumerate(kept):
        assert torch.equal(a["src_frame"][u, :n], b["src_frame"][u, :n])
    la, lb = a["levels"].cpu().numpy(), b["levels"].cpu().numpy()
    assert (lb >= 64 * la).all() and (lb <= 64 * la + 63).all() and (la[:, 2] > 0).all()
    for u in range(3):
        assert tuple(int(v) for v in la[u]) == R.vad(q[u], 480, 10, R.DEFAULT)["levels"]


def test_speech_flags_and_the_collector_take_the_adaptive_rule(eng, monkeypatch):
    """vad.AdaptiveEnergyVad through the reference's call surface (vad.py:60-129): frame_generator -> vad_collector."""
    from speaker_verification_amd import synth, vad as vad_mod
    set_route(monkeypatch, None)
    clip = synth.speaker_clip(2, 1) >> 4
    frames = list(vad_mod.frame_generator(30, clip.tobytes(), 16000))
    r = R.vad(clip, 480, 10, R.DEFAULT)
    assert len(frames) == len(r["flags"])
    v = vad_mod.AdaptiveEnergyVad()
    # (speech_flags sees the frames without the partial one behind them: one pad sample, the same whole frames)
    np.testing.assert_array_equal(v.speech_flags(frames, 16000), r["flags"])
    segments = list(vad_mod.vad_collector(16000, 30, 300, v, frames))
    want = [b"".join(frames[i].bytes for i in np.nonzero(r["seg"] == k)[0]) for k in range(int(r["seg"].max()) + 1)]
    assert segments == want and len(want) >= 1
    res = vad_mod.energy_vad_batch(clip[None, :], vad=v)
    assert int(res["voiced_len"][0]) == int(r["keep"].sum()) * 480 and "levels" in res


# ---- refusals ----------------------------------------------------------------------------------------------------------------
GOOD = dict(n_utt=2, frame_samples=160, ring_len=10, ring_thresh=9, floor_q16=6554, peak_q16=62259, above_floor_q16=655360,
            below_peak_q16=207, min_threshold=0, max_vad_frames=20, d_pcm=True, d_keep=True)
BAD_ARG, UNSUPPORTED = -1, -2
REFUSALS = [
    (dict(floor_q16=-1), BAD_ARG, "floor_q16"), (dict(floor_q16=65537, peak_q16=65536), BAD_ARG, "floor_q16"),
    (dict(peak_q16=65537), BAD_ARG, "peak_q16"), (dict(floor_q16=40000, peak_q16=30000), BAD_ARG, "floor_q16"),
    (dict(above_floor_q16=65535), BAD_ARG, "above_floor_q16"), (dict(above_floor_q16=(1 << 40) + 1), BAD_ARG, "above_floor_q16"),
    (dict(below_peak_q16=-1), BAD_ARG, "below_peak_q16"), (dict(below_peak_q16=65537), BAD_ARG, "below_peak_q16"),
    (dict(min_threshold=-1), BAD_ARG, "min_threshold"), (dict(min_threshold=1 << 62), BAD_ARG, "min_threshold"),
    (dict(d_pcm=False), BAD_ARG, "d_pcm"), (dict(d_keep=False), BAD_ARG, "d_keep"),
    (dict(frame_samples=65537), UNSUPPORTED, "frame_samples"), (dict(max_vad_frames=8193), UNSUPPORTED, "VAD frames"),
]


@pytest.mark.parametrize("change,code,word", REFUSALS, ids=["%s=%s" % next(iter(ch.items())) for ch, _, _ in REFUSALS])
def test_refusals_name_the_parameter_and_write_nothing(eng, change, code, word):
    a = dict(GOOD, **change)
    n, mv = a["n_utt"], 20                                  # (the buffers keep their size whatever max_vad_frames claims)
    pcm = torch.full((n, 160 * mv + 1), 9000, dtype=torch.int16, device=eng.device)
    outs = {"keep": torch.full((n, mv), 0x5A, dtype=torch.uint8, device=eng.device),
            "seg": torch.full((n, mv), 0x5A5A, dtype=torch.int32, device=eng.device),
            "nvf": torch.full((n,), 0x5A5A, dtype=torch.int32, device=eng.device),
            "voiced": torch.full_like(pcm, 0x5A5A), "vlen": torch.full((n,), 0x5A5A, dtype=torch.int32, device=eng.device),
            "src": torch.full((n, mv), 0x5A5A, dtype=torch.int32, device=eng.device),
            "levels": torch.full((n, 3), 0x5A5A, dtype=torch.int64, device=eng.device),
            "energy": torch.full((n, mv), 0x5A5A, dtype=torch.int64, device=eng.device)}
    before = {k: v.clone() for k, v in outs.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731
    eng._stream()
    rc = eng.lib.svk_vad_adaptive(eng.ctx, ptr(pcm) if a["d_pcm"] else None, None, None, pcm.shape[1], pcm.shape[1], n,
                                  a["frame_samples"], a["ring_len"], a["ring_thresh"], a["floor_q16"], a["peak_q16"],
                                  a["above_floor_q16"], a["below_peak_q16"], a["min_threshold"], a["max_vad_frames"],
                                  ptr(outs["keep"]) if a["d_keep"] else None, ptr(outs["seg"]), ptr(outs["nvf"]), ptr(outs["voiced"]),
                                  ptr(outs["vlen"]), ptr(outs["src"]), ptr(outs["levels"]), ptr(outs["energy"]))
    torch.cuda.synchronize()
    message = eng.lib.svk_last_error(eng.ctx).decode()
    assert rc == code and word in message, (rc, message)
    for k in outs:
        assert torch.equal(outs[k], before[k]), "a refused call wrote " + k


def test_no_clips_launches_nothing(eng):
    assert eng.lib.svk_vad_adaptive(eng.ctx, None, None, None, 0, 0, 0, 160, 10, 9, 6554, 62259, 655360, 207, 0, 20, None, None, None,
                                    None, None, None, None, None) == 0
