"""The memory contract of include/svk.h (Conventions) for svk_frontend_run (frontend.hip), called directly on guarded arenas
(tests/memory_contract.py) in the environments A, B and C, placed for the vector paths (256-byte boundaries) and for the
scalar ones (one element past a boundary).  d_pcm is ONE flat buffer: the clips sit at chosen offsets with gaps between them
that hold the payload pattern (0, NaN / -1, a finite other number), and the last clip ends flush against the trailing guard.
Every comparison is on bytes, against the Engine wrapper's result for the same call on ordinary tensors whose gaps hold
other samples.  The instance is steered with the switches the library reads at every call (SVK_FE_GENERIC, SVK_FE_F32STAGE,
SVK_FE_WAVES); SVK_FRONTEND_TILE is read when a plan is made, so each forced tile size has an Engine of its own.  The
compiled instances exist for tiles of 8 frames only, so every route that means one forces that tile, and every call asserts
the instance that ran from the line the library prints under SVK_FE_DEBUG."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

F32, I16, I32, I64 = torch.float32, torch.int16, torch.int32, torch.int64
MFE, LMFE, MFCC = 0, 1, 2
STRIDE = 160
FRAMES = (7, None, 17, 0, 1, 9)        # per clip; None: a clip shorter than a frame, 0: exactly frame_len samples (no frame: Q3)
MAX_FRAMES = max(f for f in FRAMES if f) + 3
SWITCHES = ("SVK_FE_GENERIC", "SVK_FE_F32STAGE", "SVK_FE_WAVES", "SVK_FRONTEND_TILE")


def _spec(which, **kw):
    """A: MFCC-13 at nfft 512, 20 ms frames; B: LMFE-40 at nfft 1024, 25 ms frames -- the two compiled instances."""
    from speaker_verification_amd.engine import FrontendSpec
    if which == "A":
        return FrontendSpec(16000, 320, STRIDE, 512, 40, 13, MFCC, **kw)
    return FrontendSpec(16000, 400, STRIDE, 1024, 40, 13, kw.pop("out_kind", LMFE), **kw)


def _lengths(flen):
    """Samples per clip: none a multiple of 8 but the clip of exactly frame_len samples."""
    tail = {7: 3, 17: 3, 1: 3, 9: 5}
    lens = [flen - 19 if f is None else flen + STRIDE * f + tail.get(f, 0) for f in FRAMES]
    assert all(n % 8 for n, f in zip(lens, FRAMES) if f != 0)
    return lens


@pytest.fixture(scope="module")
def engines():
    from speaker_verification_amd.engine import Engine, get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    made = {None: get_engine(0)}

    def get(tile=None):
        if tile not in made:
            made[tile] = Engine(0)
        return made[tile]
    return get


def _set(monkeypatch, env, tile):
    monkeypatch.setenv("SVK_FE_DEBUG", "1")
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    if tile is not None:
        monkeypatch.setenv("SVK_FRONTEND_TILE", str(tile))


def _instance(which, kw, kind, env, tile, want_energy):
    """The instance pick_instance (frontend.hip) chooses: a compiled one for tiles of 8 frames when the generic one is not
    forced, int16 samples are staged raw (no f32 staging, pre-emphasis shift 1), the configuration is the compiled one and --
    LMFE-40, which computes no frame energy -- d_energy is NULL; else the generic one.  None: the tile is the library's choice."""
    if tile is None:
        return None
    pre2 = kw.get("preemph") and kw.get("preemph_shift", 1) != 1
    if tile != 8 or "SVK_FE_GENERIC" in env or pre2 or (kind == "i16" and "SVK_FE_F32STAGE" in env) or "out_kind" in kw:
        return "generic"
    if which == "B" and want_energy:
        return "generic"
    return ("mfcc13" if which == "A" else "lmfe40") + (" (f32)" if kind == "f32" else "")


def _ran(capfd):
    """The instance name of the ONE svk_frontend_run call since the last look."""
    m = re.findall(r"svk_frontend_run: (.+) instance, (\d+) waves/CU", capfd.readouterr().err)
    assert len(m) == 1, m
    return m[0][0], int(m[0][1])


def _layout(form, flen):
    """-> (offsets | None, lengths | None, clip_stride, clip_len, where each clip starts, samples per clip)."""
    lens = _lengths(flen)
    if form.startswith("offsets"):
        odd, at, offs = form.endswith("odd"), 0, []
        for i, n in enumerate(lens):
            at += 8 + 8 * i
            at += (1 - at % 2) if odd else (-at) % 8
            offs.append(at)
            at += n
        return offs, lens, 0, 0, offs, lens
    if form == "stride":               # d_offsets NULL: clip i at i * clip_stride (odd: every other clip off a 4-byte boundary)
        stride = max(lens) + 11
        return None, lens, stride, 0, [i * stride for i in range(len(lens))], lens
    n9 = flen + STRIDE * 9 + 5          # both NULL: three clips of clip_len samples
    return None, None, n9 + 6, n9, [i * (n9 + 6) for i in range(3)], [n9] * 3


def _pcm(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "i16":
        return torch.randint(-8000, 8001, (n,), generator=g, dtype=I32).to(I16)
    return torch.randn((n,), generator=g, dtype=F32) * 0.1


# name -> (spec, its keywords, PCM type, switches, forced tile, max_frames)
PRE1, PRE2 = dict(preemph=True, preemph_shift=1), dict(preemph=True, preemph_shift=2)
ROUTES = {
    "A-i16": ("A", {}, "i16", {}, 8, MAX_FRAMES), "B-i16": ("B", {}, "i16", {}, 8, MAX_FRAMES),
    "A-f32": ("A", {}, "f32", {}, 8, MAX_FRAMES), "B-f32": ("B", {}, "f32", {}, 8, MAX_FRAMES),
    "B-mfe-i16": ("B", dict(out_kind=MFE), "i16", {}, 8, MAX_FRAMES),
    "A-i16-generic": ("A", {}, "i16", {"SVK_FE_GENERIC": "1"}, 8, MAX_FRAMES),
    "B-i16-generic": ("B", {}, "i16", {"SVK_FE_GENERIC": "1"}, 8, MAX_FRAMES),
    "A-f32-generic": ("A", {}, "f32", {"SVK_FE_GENERIC": "1"}, 8, MAX_FRAMES),
    "A-i16-f32stage": ("A", {}, "i16", {"SVK_FE_F32STAGE": "1"}, 8, MAX_FRAMES),
    "B-i16-f32stage": ("B", {}, "i16", {"SVK_FE_F32STAGE": "1"}, 8, MAX_FRAMES),
    "A-i16-own-tile": ("A", {}, "i16", {}, None, MAX_FRAMES), "B-i16-own-tile": ("B", {}, "i16", {}, None, MAX_FRAMES),
    "A-i16-tile16": ("A", {}, "i16", {}, 16, MAX_FRAMES), "B-i16-tile16": ("B", {}, "i16", {}, 16, MAX_FRAMES),
    "B-f32-tile16": ("B", {}, "f32", {}, 16, MAX_FRAMES),
    "A-pre1-i16": ("A", PRE1, "i16", {}, 8, MAX_FRAMES), "B-pre1-i16": ("B", PRE1, "i16", {}, 8, MAX_FRAMES),
    "A-pre1-f32": ("A", PRE1, "f32", {}, 8, MAX_FRAMES), "A-pre2-i16": ("A", PRE2, "i16", {}, 8, MAX_FRAMES),
    "B-pre2-f32": ("B", PRE2, "f32", {}, 8, MAX_FRAMES), "B-pre1-i16-tile16": ("B", PRE1, "i16", {}, 16, MAX_FRAMES),
    # 6 clips x 50 tiles of 8 frames exceed the chip's workgroups: more than one wave per workgroup, and SVK_FE_WAVES = 1
    "B-i16-many-tiles": ("B", {}, "i16", {}, 8, 400), "B-i16-many-tiles-one-wave": ("B", {}, "i16", {"SVK_FE_WAVES": "1"}, 8, 400),
    "A-i16-many-tiles": ("A", {}, "i16", {}, 8, 400), "A-i16-many-tiles-one-wave": ("A", {}, "i16", {"SVK_FE_WAVES": "1"}, 8, 400),
}


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("form", ("offsets-aligned", "offsets-odd", "stride", "uniform"))
@pytest.mark.parametrize("route", tuple(ROUTES))
def test_frontend_run(engines, monkeypatch, capfd, route, form, placed):
    """Samples outside the clips are not read: pre-emphasis is circular over the clip, so a read of the wrong neighbour -- the
    sample in front of the clip, or the one behind it -- shows here.  d_feat and d_energy rows at or past n_frames are zeros in
    every environment, d_n_frames is exact, d_energy and d_n_frames may be NULL."""
    which, kw, kind, env, tile, max_frames = ROUTES[route]
    spec, eng = _spec(which, **kw), engines(tile)
    _set(monkeypatch, env, tile)
    handle, _ = eng.plan(spec)
    offs, lens, clip_stride, clip_len, starts, sizes = _layout(form, spec.frame_len)
    n, total = len(starts), starts[-1] + sizes[-1]
    full = _pcm(kind, max(total, n * clip_stride), len(route))        # the wrapper's buffer: other samples in the gaps
    live = torch.zeros(total, dtype=torch.bool)
    for s, k in zip(starts, sizes):
        live[s:s + k] = True
    assert not live.all() and live[-1]
    frames = [spec.num_frames(k) for k in sizes]
    assert form == "uniform" or frames == [f or 0 for f in FRAMES]
    refs = {}
    for want_energy in (True, False):
        if offs is not None:
            got = eng.features(full[:total], spec, lengths=np.asarray(lens, np.int32), offsets=np.asarray(offs, np.int64),
                               max_frames=max_frames, want_energy=want_energy)
        else:
            got = eng.features(full[:n * clip_stride].view(n, clip_stride), spec, lengths=None if lens is None else np.asarray(lens, np.int32),
                               clip_len=clip_len or None, max_frames=max_frames, want_energy=want_energy)
        refs[want_energy] = [None if t is None else M.bits(t) for t in got]
    rows_past = np.arange(max_frames)[None, :] >= np.asarray(frames)[:, None]
    for want_energy, want_counts in ((True, True), (False, True), (True, False), (False, False)):
        ref_feat, ref_counts, ref_energy = refs[want_energy]
        assert ref_counts.astype(np.int32).tolist() == frames
        for name in M.ENV_NAMES:
            capfd.readouterr()
            c = M.Contract(eng, name, scalar=placed == "scalar")
            dp = c.input_where("d_pcm", full[:total], live)
            do = c.input("d_offsets", torch.tensor(offs, dtype=I64)) if offs is not None else None
            dl = c.input("d_lengths", torch.tensor(lens, dtype=I32)) if lens is not None else None
            feat = c.output("d_feat", F32, (n, max_frames, spec.num_cols))
            energy = c.output("d_energy", F32, (n, max_frames)) if want_energy else None
            counts = c.output("d_n_frames", I32, (n,)) if want_counts else None
            c.call(eng.lib.svk_frontend_run, handle, dp, 0 if kind == "i16" else 1, do, dl, clip_stride, clip_len, n, max_frames,
                   feat, energy, counts, None, 0, 0)
            ran, waves = _ran(capfd)
            expect = _instance(which, kw, kind, env, tile, want_energy)
            assert expect is None or ran == expect, "%s ran the %s instance, not %s" % (route, ran, expect)
            assert waves == 1 or "SVK_FE_WAVES" not in env
            if max_frames > MAX_FRAMES and "SVK_FE_WAVES" not in env and form != "uniform" and eng.num_cu < 300:      # (300 tiles)
                assert waves > 1, "more tiles than CUs, yet one wave per workgroup"
            what = "svk_frontend_run %s %s energy %s n_frames %s, %s, environment %s" % (route, form, want_energy, want_counts, placed, name)
            got = feat.bits()
            M.same_bits(got, ref_feat, what + ": d_feat")
            assert not got[rows_past].any(), what + ": d_feat rows at or past n_frames are +0"
            if energy is not None:
                M.same_bits(energy.bits(), ref_energy, what + ": d_energy")
                assert not energy.bits()[rows_past].any(), what + ": d_energy rows at or past n_frames are +0"
            if counts is not None:
                M.same_bits(counts.bits(), ref_counts, what + ": d_n_frames")


# ---- gathered input ----------------------------------------------------------------------------------------------------------
CHUNK = 160
VAD_FRAMES = (30, 12, 40)
LOUD = {30: ((2, 9), (14, 27)), 12: ((1, 10),), 40: ((3, 13), (20, 35))}


def _voiced_batch():
    """Three clips of whole VAD frames in a flat int16 buffer, gaps between them, offsets on 16-byte boundaries."""
    g = torch.Generator().manual_seed(99)
    offs, lens, at = [], [], 0
    for k in VAD_FRAMES:
        at += 40
        offs.append(at)
        lens.append(k * CHUNK + 7)
        at += lens[-1] + (-(at + lens[-1])) % 8
    total = offs[-1] + lens[-1]
    pcm = torch.randint(-9, 10, (total,), generator=g, dtype=I32)
    for off, k in zip(offs, VAD_FRAMES):
        for a, b in LOUD[k]:
            pcm[off + a * CHUNK:off + b * CHUNK] = torch.randint(-6000, 6001, ((b - a) * CHUNK,), generator=g, dtype=I32)
    return pcm.to(I16), np.asarray(offs, np.int64), np.asarray(lens, np.int32)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("want_energy", (True, False), ids=("energy", "no-energy"))
@pytest.mark.parametrize("generic", (False, True), ids=("compiled", "generic"))
@pytest.mark.parametrize("which", ("A", "B"))
def test_gathered_input(engines, monkeypatch, capfd, which, generic, want_energy, placed):
    """d_src_chunk from a real svk_vad_energy call.  Entries past a clip's chunk count hold the pattern (-1 in B, a large index
    in C: read, either would leave the buffer), PCM frames no entry names hold it too; the features are the compacted copy's,
    byte for byte.  (LMFE-40's compiled instance runs only without d_energy: the id says `compiled` for what is not forced
    to the generic one, the assertion below says what ran.)"""
    eng, spec = engines(8), _spec(which)
    env = {"SVK_FE_GENERIC": "1"} if generic else {}
    _set(monkeypatch, env, 8)
    handle, _ = eng.plan(spec)
    pcm, offs, lens = _voiced_batch()
    n, total = len(offs), pcm.numel()
    kw = dict(lengths=lens, offsets=offs, frame_samples=CHUNK, ring_len=3, longest=int(lens.max()))
    copy, index = eng.vad_energy(pcm, 100000, compact=True, **kw), eng.vad_energy(pcm, 100000, compact="index", **kw)
    vlen, table = copy["voiced_len"].cpu(), index["src_frame"].cpu()
    kept = [int(v) // CHUNK for v in vlen]
    assert all(0 < k < f for k, f in zip(kept, VAD_FRAMES)) and int(vlen.max()) >= spec.frame_len + 9 * STRIDE
    max_frames = spec.num_frames(int(vlen.max())) + 3
    want = [None if t is None else M.bits(t) for t in
            eng.features(copy["voiced"], spec, lengths=vlen, offsets=offs, max_frames=max_frames, want_energy=want_energy)]
    named, live = torch.arange(table.shape[1])[None, :] < torch.tensor(kept)[:, None], torch.zeros(total, dtype=torch.bool)
    for u in range(n):
        for f in table[u, :kept[u]].tolist():
            live[int(offs[u]) + f * CHUNK:int(offs[u]) + (f + 1) * CHUNK] = True
    assert not live.all()
    for name in M.ENV_NAMES:
        c = M.Contract(eng, name, scalar=placed == "scalar")
        dp, do, dl = c.input_where("d_pcm", pcm, live), c.input("d_offsets", torch.from_numpy(offs)), c.input("d_lengths", vlen)
        dt = c.input_where("d_src_chunk", table, named)
        feat = c.output("d_feat", F32, (n, max_frames, spec.num_cols))
        energy = c.output("d_energy", F32, (n, max_frames)) if want_energy else None
        counts = c.output("d_n_frames", I32, (n,))
        capfd.readouterr()
        c.call(eng.lib.svk_frontend_run, handle, dp, 0, do, dl, 0, 0, n, max_frames, feat, energy, counts, dt, CHUNK, table.shape[1])
        ran, expect = _ran(capfd)[0], _instance(which, {}, "i16", env, 8, want_energy)
        assert ran == expect, "the %s instance ran, not %s" % (ran, expect)
        what = "svk_frontend_run gathered %s %s, %s, environment %s" % (which, ran, placed, name)
        for arena, ref, out in ((feat, want[0], "d_feat"), (counts, want[1], "d_n_frames"), (energy, want[2], "d_energy")):
            if arena is not None:
                M.same_bits(arena.bits(), ref, what + ": " + out)
