"""The fused front end (csrc/frontend.hip, svk_frontend_run) against float64 on every instance and staging path
(tests/frontend_f64_ref.py: the float64 reference, the plain float32 restatement that serves as yardstick, the bar).

CPU (default pass):
  * the reference is oracle.speechpy_ref.mfe / lmfe / mfcc on int16 input to 1e-12 relative;
  * the yardstick passes its own bar and every planted fault (frontend_f64_ref.MUTANTS) fails it on the GPU tests' own
    inputs: the bar has teeth before any GPU is involved;
  * no element of any log-domain case is left out as ill-conditioned.
GPU (-m gpu): every launch goes through Engine.features; the instance is steered with the switches the library reads at
every call (SVK_FE_GENERIC, SVK_FE_F32STAGE, SVK_FE_WAVES) or at plan creation (SVK_FRONTEND_TILE: one Engine per tile
size, so that no plan made under another setting is reused).  What can be asserted exactly is: frame counts, zero rows,
the all-zero clip, and bit identity between paths that do the same arithmetic on the same samples.  Lines starting with
"ULPS" carry, per launch, the worst kernel error / yardstick ratio (the bar is 4; where an emulation of the path's own
order of operations exceeds 4 on the same input, twice the emulation's ratio and at most 16: frontend_f64_ref.margin).

One defect came out of these tests and is fixed in frontend.hip: at nfft 512 two frames share a complex transform, and a
frame of exact zeros beside a non-zero one came back with ~5e-15 of its partner's power instead of 0 (log-mel -20 where
the reference has log(eps) = -36).  The case that shows it is the generic nfft-512 launch with preemph_shift = 2 on the
clip whose only non-zero sample is its last (frame 0 holds one sample, frame 1 none): 2e5 x the yardstick before.
"""
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import frontend_f64_ref as R                                   # noqa: E402  (tests/ is on sys.path)
from oracle import speechpy_ref as ref                         # noqa: E402
from speaker_verification_amd import synth                     # noqa: E402
from speaker_verification_amd.engine import FrontendSpec       # noqa: E402

FS = 16000
MFE, LMFE, MFCC = R.MFE, R.LMFE, R.MFCC
EPS32 = np.float32(R.EPS64)
# float32 log(eps), eps = 2^-52, as each PCM type's kernels take it (fast_log in frontend.hip), bit for bit: integer PCM
# multiplies the exact log2 = -52 by float32(ln 2) (v_log_f32 x ln 2: one more rounding, what NumPy's float32 log returns
# too); float PCM takes the library logarithm, which returns the correctly rounded value.  The two are neighbours.
LOG_EPS32 = {False: np.float32(-52.0) * np.float32(np.log(2.0)), True: np.float32(np.log(R.EPS64))}
assert abs(int(LOG_EPS32[False].view(np.int32)) - int(LOG_EPS32[True].view(np.int32))) == 1
assert LOG_EPS32[False] < np.log(R.EPS64) < LOG_EPS32[True]


def spec_a(out_kind=MFCC, **kw):
    """MFCC-13 / nfft 512 / 20 ms: the configuration SpecMfcc13 is compiled for."""
    kw.setdefault("num_ceps", 13)
    kw.setdefault("num_filters", 40)
    kw.setdefault("frame_len", 320)
    kw.setdefault("frame_stride", 160)
    return FrontendSpec(kw.pop("fs", FS), kw.pop("frame_len"), kw.pop("frame_stride"), kw.pop("nfft", 512),
                        kw.pop("num_filters"), kw.pop("num_ceps"), out_kind, **kw)


def spec_b(out_kind=LMFE, **kw):
    """LMFE-40 / nfft 1024 / 25 ms: the configuration SpecLmfe40 is compiled for."""
    kw.setdefault("num_ceps", 13)
    kw.setdefault("frame_len", 400)
    kw.setdefault("nfft", 1024)
    return spec_a(out_kind, **kw)


# ---- inputs: built once, read-only ---------------------------------------------------------------------------------
def _tone_noise(seed, n, sigma=300.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return np.rint(8000.0 * np.sin(2 * np.pi * 1000.37 * t / FS) + sigma * rng.standard_normal(n)).astype(np.int16)


COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 25, 33, 40, 47, 56, 64, 65, 72, 81, 90)
_BATCHES = {}


def ragged_batch(name):
    """"i320" / "i400": 26 int16 clips of at most 1 s whose frame counts at (flen, hop 160) are 0 (len = flen - 1 and
    len = flen), COUNTS and the most 1 s holds; noise, speaker and tone-plus-noise in turn; then an all-zero clip, a
    full-scale square wave and a clip whose only non-zero sample is its last.  "f320" / "f400": the same divided by 32768
    as float32, plus one quiet clip scaled by 2^-40.  -> (list of clips, index of the all-zero clip)."""
    if name == "ticket":
        return ticket_batch(), None
    if name not in _BATCHES:
        flen = int(name[1:])
        lens = [flen - 1, flen] + [flen + 160 * T + (37 * T) % 160 for T in COUNTS] + [FS]
        clips = []
        for i, n in enumerate(lens):
            clips.append((synth.noise_clip(300 + i, n), synth.speaker_clip(i, 0, n), _tone_noise(i, n))[i % 3])
        zero = len(clips)
        clips.append(np.zeros(flen + 160 * 20 + 5, dtype=np.int16))
        clips.append(np.where((np.arange(flen + 160 * 30 + 11) // 25) % 2 == 0, 32767, -32767).astype(np.int16))
        last = np.zeros(flen + 160 * 12 + 3, dtype=np.int16)
        last[-1] = 12345
        clips.append(last)
        if name[0] == "f":
            clips = [(x / 32768.0).astype(np.float32) for x in clips]
            clips.append((synth.noise_clip(77, flen + 160 * 35 + 1) / 32768.0 * 2.0 ** -40).astype(np.float32))
        for x in clips:
            x.setflags(write=False)
        _BATCHES[name] = (clips, zero)
    return _BATCHES[name]


def feat_is_f32_pcm(batch):
    return ragged_batch(batch)[0][0].dtype == np.float32


def batch_for(spec, f32=False):
    return ("f" if f32 else "i") + ("400" if spec.nfft == 1024 else "320")


def ticket_batch():
    """"ticket": 64 int16 clips of 1 s (one a little shorter), ~800 frame tiles of 8.  (6 000 frames: the tone sits on more
    noise than in the ragged batch, so that no narrow filter of any frame falls below 1e-9 of its frame's energy.)"""
    if "ticket" not in _BATCHES:
        clips = [(synth.noise_clip(700 + i, FS), synth.speaker_clip(i, 2, FS), _tone_noise(40 + i, FS, 1500.0))[i % 3]
                 for i in range(64)]
        clips[17] = clips[17][:FS - 333]
        for x in clips:
            x.setflags(write=False)
        _BATCHES["ticket"] = (clips, None)
    return _BATCHES["ticket"][0]


_CASES = {}


def case(batch, spec):
    """(float64 references, float32 yardsticks) of every clip of `batch` under `spec`, computed once and shared by the CPU
    and the GPU tests.  (They hold both dc_elimination settings and all three output kinds.)"""
    key = (batch,) + tuple(v for s, v in zip(spec.__slots__, spec.key()) if s not in ("out_kind", "dc_elimination"))
    if key not in _CASES:
        clips = ragged_batch(batch)[0] if isinstance(batch, str) else batch
        _CASES[key] = ([R.reference(x, spec) for x in clips], [R.restatement32(x, spec) for x in clips])
    return _CASES[key]


def trimmed(res, M):
    """A reference dict with `max_frames` applied."""
    if M is None or res["n_frames"] <= M:
        return res
    out = {k: (v[:M] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    out["n_frames"] = M
    return out


# ---- every GPU launch that is held to the bar, named once: the CPU pass walks the same list ---------------------------
PRE = dict(preemph=True, preemph_cof=0.98)

# Section 2 of the product {A, B} x {tile 8, 16} x {raw int16, int16 through f32 staging, int16 with shift 2, float32} x
# {MFE, LMFE, MFCC} x {dc on, off} x {energy asked, not}.  Pruned to what selects different code:
#   * the staging decides how samples reach the FFT; everything after the power tile is the same code for all four.  So
#     every (configuration, tile, staging) runs once, with pre-emphasis, as MFCC with dc_elimination and energy output (the
#     longest tail: energy MFMAs, log, DCT, c0), and raw int16 / float32 once more without pre-emphasis (PRE = false reader);
#   * output kind, dc_elimination and the energy request decide the tail only: their 6 distinct combinations (MFE, LMFE,
#     MFCC without dc, each with and without energy; MFCC with dc is above) run on raw int16 for every (configuration, tile);
#   * dc_elimination does nothing to MFE / LMFE, and MFCC with dc always needs the energy: not repeated.
STAGINGS = ("raw16", "i16 f32stage", "i16 shift2", "f32")


def generic_cases():
    out = []
    for cfg in ("A", "B"):
        mk = spec_a if cfg == "A" else spec_b
        for tile in (8, 16):
            for st in STAGINGS:
                kw = dict(PRE, preemph_shift=2) if st == "i16 shift2" else dict(PRE)
                out.append((cfg, tile, st, mk(MFCC, **kw), True))
                if st in ("raw16", "f32") and tile == 8:
                    out.append((cfg, tile, st, mk(MFCC), True))
            for kind, extra in ((MFE, {}), (LMFE, {}), (MFCC, dict(dc_elimination=False))):
                for energy in (True, False):
                    out.append((cfg, tile, "raw16", mk(kind, **dict(PRE, **extra)), energy))
    return out


def _id(c):
    cfg, tile, st, spec, energy = c
    return "%s-tile%d-%s-%s%s%s%s" % (cfg, tile, st.replace(" ", "_"), ("mfe", "lmfe", "mfcc")[spec.out_kind],
                                       "" if spec.dc_elimination else "_nodc", "-pre" if spec.preemph else "",
                                       "-energy" if energy else "")


GENERIC_CASES = generic_cases()

GEOMETRIES = [
    ("flen 50 (one register step)", spec_a(frame_len=50, **PRE)),
    ("flen 511", spec_a(frame_len=511, **PRE)),
    ("flen 513 cut to 512", spec_a(frame_len=513)),        # (with pre-emphasis two elements of this batch are ill-conditioned)
    ("flen 1100 cut to 1024", spec_b(MFCC, frame_len=1100, **PRE)),
    ("odd stride 161 at nfft 1024", spec_b(MFCC, frame_stride=161, **PRE)),
    ("stride 80", spec_a(frame_stride=80, **PRE)),
    ("stride 80 at nfft 1024", spec_b(MFCC, frame_stride=80, **PRE)),
    ("stride 400", spec_a(frame_stride=400, **PRE)),
    ("stride 400 at nfft 1024", spec_b(MFCC, frame_stride=400, **PRE)),
    ("26 filters 100..7000 Hz", spec_a(num_filters=26, low_freq=100, high_freq=7000, **PRE)),
    ("1 filter", spec_a(num_filters=1, num_ceps=1, dc_elimination=False)),
    ("17 filters", spec_a(num_filters=17, num_ceps=17, dc_elimination=False, **PRE)),
    ("33 filters at nfft 1024", spec_b(MFCC, num_filters=33, num_ceps=16, **PRE)),
    ("64 filters 64 cepstra", spec_a(num_filters=64, num_ceps=64, dc_elimination=False, **PRE)),
    ("64 filters log-mel at nfft 1024", spec_b(LMFE, num_filters=64, **PRE)),
    ("1 cepstrum", spec_a(num_ceps=1)),
    ("16 cepstra", spec_a(num_ceps=16, dc_elimination=False)),
    ("17 cepstra", spec_b(MFCC, num_ceps=17)),
    ("40 cepstra of 40 filters", spec_a(num_ceps=40, **PRE)),
    ("fs 8000 at nfft 1024 (bin 256)", spec_b(MFCC, fs=8000, frame_len=200, frame_stride=80, **PRE)),
    ("fs 8000 at nfft 1024 log-mel", spec_b(LMFE, fs=8000, frame_len=200, frame_stride=80)),
    ("input_scale 2^-15", spec_b(MFCC, input_scale=2.0 ** -15, **PRE)),
    ("input_scale 2^-15 mel energies", spec_a(MFE, input_scale=2.0 ** -15)),
]

def ticket_specs():
    """The flagship log-mel front end (pre-emphasis, int16 read as [-1, 1)) and the plain MFCC one."""
    return [spec_b(**dict(PRE, input_scale=1.0 / 32768.0)), spec_a()]


SPECIALISED = [("mfcc13", spec_a, False), ("lmfe40", spec_b, False), ("mfcc13 (f32)", spec_a, True),
               ("lmfe40 (f32)", spec_b, True)]


def all_bar_cases():
    """(batch name, spec) of every launch the GPU tests hold to the bar."""
    out = []
    for _, mk, f32 in SPECIALISED:
        for kw in ({}, PRE):
            out.append((batch_for(mk(), f32), mk(**kw)))
    out += [(batch_for(s, st == "f32"), s) for _, _, st, s, _ in GENERIC_CASES]
    out += [(batch_for(s), s) for _, s in GEOMETRIES]
    ticket_batch()
    out += [("ticket", s) for s in ticket_specs()]
    return out


_MARGINS = {}


def margin_of(batch, spec):
    """(margin, the emulation's ratio or None) of a launch on `batch` (R.margin), computed once."""
    key = (batch, spec.key())
    if key not in _MARGINS:
        _MARGINS[key] = R.margin(ragged_batch(batch)[0], *case(batch, spec), spec)
    return _MARGINS[key]


def judge(what, gots, batch, spec, M=None, energy=True):
    refs, yards = case(batch, spec)
    refs, yards = [trimmed(r, M) for r in refs], [trimmed(y, M) for y in yards]
    margin, emul = margin_of(batch, spec)
    v = R.compare(gots, refs, yards, spec, margin=margin, energy=energy)
    note = "" if emul is None else "  [the path's emulation: %.2f%s]" % (emul, ", margin raised" if margin > R.K else "")
    print("ULPS %-62s features %5.2f  energy %5.2f  x yardstick (bar %.3g)%s%s" %
          (what, v["ratio_feat"], v["ratio_energy"], margin, note, "" if v["ok"] else "  FAILS: " + v["why"]))
    return v


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracle():
    """On int16 input the oracle is float64 throughout, like the reference: mel energies, frame energies, log-mel and the
    cepstra (both dc_elimination settings) agree to 1e-12 relative (the cepstra, which cross zero, relative to the largest
    one), the frame counts exactly -- including len = flen - 1, len = flen (0 frames) and len = flen + stride (1)."""
    clips = ragged_batch("i400")[0]
    picks = [clips[i] for i in (0, 1, 2, 5, 9, 13, 20, 22, 23)]
    specs = [(spec_a(), 0.020, 0.010), (spec_b(MFCC, num_ceps=40), 0.025, 0.010),
             (spec_a(num_filters=26, low_freq=100, high_freq=7000), 0.020, 0.010),
             (spec_b(MFCC, fs=8000, frame_len=200, frame_stride=80), 0.025, 0.010)]
    for spec, fl, fs_ in specs:
        kw = dict(frame_length=fl, frame_stride=fs_, num_filters=spec.num_filters, fft_length=spec.nfft,
                  low_frequency=spec.low_freq, high_frequency=spec.high_freq)
        for x in picks:
            r = R.reference(x, spec)
            mel, energy = ref.mfe(x, spec.fs, **kw)
            assert r["n_frames"] == mel.shape[0] == R.num_frames(x.size, spec)
            if r["n_frames"] == 0:
                continue
            np.testing.assert_allclose(r["mel"], mel, rtol=1e-12, atol=0)
            np.testing.assert_allclose(r["energy"], energy, rtol=1e-12, atol=0)
            np.testing.assert_allclose(r["logmel"], ref.lmfe(x, spec.fs, **kw), rtol=1e-12, atol=0)
            for dc, mine in ((True, r["ceps_dc"]), (False, r["ceps_nodc"])):
                want = ref.mfcc(x, spec.fs, num_cepstral=spec.num_ceps, dc_elimination=dc, **kw)
                np.testing.assert_allclose(mine, want, rtol=0, atol=1e-12 * np.abs(want).max())
    # pre-emphasis: the oracle's is float64 on int16 input when given the widened float32 coefficient
    x = picks[5]
    s = spec_a(**PRE)
    want = ref.mfcc(ref.preemphasis(x, cof=float(np.float32(0.98))), FS)
    np.testing.assert_allclose(R.reference(x, s)["ceps_dc"], want, rtol=0, atol=1e-12 * np.abs(want).max())
    assert R.num_frames(319, spec_a()) == 0 and R.num_frames(320, spec_a()) == 0 and R.num_frames(480, spec_a()) == 1


def test_yardstick_passes_its_own_bar_and_nothing_is_left_out():
    """restatement32 against the reference on every input the GPU tests use: ratio <= 1 by construction, and the share of
    elements left out as ill-conditioned (mel < 1e-9 of the frame's energy) is 0 on every case -- the log-domain ones
    and the linear ones alike.  Prints the yardstick's own worst errors (DESIGN.md quotes them)."""
    worst = dict(logmel=0.0, loge=0.0, ceps=0.0, mel_over_e=np.inf)
    for batch, spec in all_bar_cases():
        refs, yards = case(batch, spec)
        v = R.compare([R.as_result(y, spec) for y in yards], refs, yards, spec)
        assert v["ok"] and v["ratio_feat"] <= 1.0 and v["ratio_energy"] <= 1.0, (batch, spec.key(), v)
        assert v["left_out"] == 0.0, (batch, spec.key(), v["left_out"])
        for r, y in zip(refs, yards):
            if r["n_frames"] == 0:
                continue
            worst["logmel"] = max(worst["logmel"], np.abs(y["logmel"] - r["logmel"]).max())
            worst["loge"] = max(worst["loge"], np.abs(np.log(y["energy"].astype(np.float64)) - np.log(r["energy"])).max())
            worst["ceps"] = max(worst["ceps"], np.abs(y["ceps_dc"] - r["ceps_dc"]).max(), np.abs(y["ceps_nodc"] - r["ceps_nodc"]).max())
            worst["mel_over_e"] = min(worst["mel_over_e"], (r["mel"] / r["energy"][:, None]).min())
    print("YARDSTICK worst |float32 - float64|: log-mel %.3g, log frame energy %.3g, cepstra %.3g; smallest mel / frame "
          "energy %.3g" % (worst["logmel"], worst["loge"], worst["ceps"], worst["mel_over_e"]))
    assert worst["mel_over_e"] >= R.COND


# mutant -> the specs under which it must fail the bar, on the ragged batch those specs' GPU tests use
MUTANT_SPECS = {
    "no_wrap": [spec_a(**PRE), spec_b(**PRE), spec_b(MFCC, **dict(PRE, preemph_shift=2))],
    "preemph_per_frame": [spec_a(**PRE), spec_b(**PRE)],
    "energy_no_nyquist": [spec_a(), spec_b(MFE, **PRE)],
    "energy_no_dc": [spec_a(), spec_b(MFE, **PRE)],
    "frame_more": [spec_a(), spec_b()],
    "frame_fewer": [spec_a(), spec_b()],
    "filter_last_bin": [spec_a(), spec_b(), spec_a(MFE)],
    "bins_from_256": [spec_b(MFCC, fs=8000, frame_len=200, frame_stride=80, **PRE),
                      spec_b(LMFE, fs=8000, frame_len=200, frame_stride=80)],
    "dct_row0": [spec_a(num_ceps=16, dc_elimination=False), spec_a(num_filters=17, num_ceps=17, dc_elimination=False, **PRE)],
    "c0_kept": [spec_a(), spec_a(**PRE)],
    "c0_replaced": [spec_a(num_ceps=16, dc_elimination=False), spec_b(MFCC, dc_elimination=False, **PRE)],
    "fold": [spec_a(frame_len=513), spec_b(MFCC, frame_len=1100, **PRE)],
    "scale_once": [spec_b(MFCC, input_scale=2.0 ** -15, **PRE), spec_a(MFE, input_scale=2.0 ** -15)],
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_fail_the_bar(mutant):
    """Each planted fault, on the inputs of the GPU tests, fails the bar that the kernel has to pass (for both PCM types
    where the fault does not depend on one)."""
    for spec in MUTANT_SPECS[mutant]:
        for f32 in (False, True):
            batch = batch_for(spec, f32)
            clips = ragged_batch(batch)[0]
            refs, yards = case(batch, spec)
            gots = [R.as_result(R.restatement32(x, spec, mutant), spec) for x in clips]
            v = R.compare(gots, refs, yards, spec)
            print("MUTANT %-18s %s %s: %s (features %.3g, energy %.3g x yardstick)" %
                  (mutant, batch, _id(("-", 0, "", spec, True)), v["why"] or "passes", v["ratio_feat"], v["ratio_energy"]))
            assert not v["ok"], (mutant, batch, spec.key(), v)


def test_emulations_justify_every_raised_margin():
    """The margin of a launch is K unless an emulation of the path's own order of operations exceeds K on the same input
    (R.margin); then it is twice the emulation's ratio and at most 16.  Two paths have one:
      * R.emulation_packed512, the nfft-512 path (two frames per complex transform, untangled afterwards), judged on its
        linear MFE output.  It exceeds K where a quiet frame shares its transform with a loud one (a speaker clip's first
        frame beside the onset of its first burst: the error is 2^-24 of the PARTNER's amplitude); the same arithmetic
        with one frame per transform (pack=False) does not: the packing is the cause.
      * R.emulation_dct_mfma, fast_log's two roundings and the cepstral product in the MFMA chain's accumulation order,
        on the yardstick's own mel energies.  It exceeds K on the float
        batches only: the quiet clip's log-mels are near -63 and nearly constant, so a cosine row's partial sums reach ~200
        before they cancel, and a chain with ONE accumulator rounds at that size where a SIMD matrix product (the
        yardstick) keeps several shorter sums.
    Every other launch keeps K = 4, the whole nfft-512 emulation (all outputs) stays inside 2 K on every input."""
    raised = {MFE: 0, MFCC: 0}
    seen = set()
    for batch, spec in all_bar_cases():
        if (batch, spec.key()) in seen:
            continue
        seen.add((batch, spec.key()))
        clips = ragged_batch(batch)[0]
        refs, yards = case(batch, spec)
        margin, emul = margin_of(batch, spec)
        what = "%s %s flen %d hop %d, %d filters, %d cepstra" % (batch, _id(("-", 0, "", spec, True)), spec.frame_len,
                                                                 spec.frame_stride, spec.num_filters, spec.num_ceps)
        if spec.out_kind == LMFE or (spec.out_kind == MFE and spec.nfft != 512):
            assert (margin, emul) == (R.K, None)
        else:
            assert margin == (R.K if emul <= R.K else min(16.0, 2.0 * emul)) and R.K <= margin <= 16.0
            print("EMULATION %-72s %.2f x yardstick -> margin %.3g" % (what, emul, margin))
        if spec.nfft == 512:
            v = R.compare([R.as_result(R.emulation_packed512(x, spec), spec) for x in clips], refs, yards, spec,
                          margin=max(2 * R.K, margin))
            assert v["ok"] and v["left_out"] == 0.0, (what, v)
        if margin > R.K:
            raised[spec.out_kind] += 1
            if spec.out_kind == MFE:
                alone = R.compare([R.as_result(R.emulation_packed512(x, spec, pack=False), spec) for x in clips], refs,
                                  yards, spec)
                print("EMULATION   the same with one frame per transform: %.2f" % alone["ratio_feat"])
                assert alone["ok"], alone
            else:
                assert batch[0] == "f", what                           # the quiet float clip, nothing else
    assert raised[MFE] >= 1 and raised[MFCC] >= 1


def test_mutant_list_is_complete():
    assert set(MUTANT_SPECS) == set(R.MUTANTS)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """tile -> Engine.  SVK_FRONTEND_TILE is read when a plan is made and an Engine keeps its plans, so each forced tile
    size has an Engine of its own; None is the process-wide engine with the library's own choice."""
    from speaker_verification_amd.engine import Engine, get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    made = {None: get_engine(0)}

    def get(tile=None):
        if tile not in made:
            made[tile] = Engine(0)
        return made[tile]
    return get


def set_env(mp, generic=None, tile=None, f32stage=None, waves=None):
    for name, v in (("SVK_FE_GENERIC", generic), ("SVK_FRONTEND_TILE", tile), ("SVK_FE_F32STAGE", f32stage),
                    ("SVK_FE_WAVES", waves)):
        if v is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(v))
    mp.setenv("SVK_FE_DEBUG", "1")


def padded(clips):
    L = (max(x.size for x in clips) + 7) // 8 * 8
    pcm = np.zeros((len(clips), L), dtype=clips[0].dtype)
    for i, x in enumerate(clips):
        pcm[i, :x.size] = x
    return pcm, np.array([x.size for x in clips], dtype=np.int32)


def launch(eng, capfd, clips, spec, **kw):
    """Engine.features on the padded batch -> (feat, n_frames, energy or None as NumPy, instance name, waves, grid)."""
    eng.plan(spec)                                   # the fused kernel, or an error: never the staged fall-back
    pcm, lens = padded(clips)
    kw.setdefault("lengths", lens)
    sys.stdout.write(capfd.readouterr().out)
    feat, nf, en = eng.features(pcm, spec, **kw)
    torch.cuda.synchronize()
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    m = re.findall(r"svk_frontend_run: (.+) instance, (\d+) waves/CU, grid (\d+)", cap.err)
    assert len(m) == 1, cap.err
    return (feat.cpu().numpy(), nf.cpu().numpy(), None if en is None else en.cpu().numpy(), m[0][0], int(m[0][1]),
            int(m[0][2]))


def exact_checks(feat, nf, en, batch, spec, M=None, zero=None):
    """Frame counts, zero rows and the all-zero clip, bit for bit.  -> per-clip results for the bar."""
    refs, _ = case(batch, spec)
    gots = []
    for i, r in enumerate(refs):
        T = r["n_frames"] if M is None else min(r["n_frames"], M)
        assert int(nf[i]) == T, (i, int(nf[i]), T)
        assert not feat[i, T:].view(np.uint32).any(), "clip %d: rows past frame %d are not +0" % (i, T)
        if en is not None:
            assert not en[i, T:].view(np.uint32).any(), "clip %d: energy past frame %d is not +0" % (i, T)
        gots.append(dict(n_frames=T, feat=feat[i, :T], energy=None if en is None else en[i, :T]))
    if zero is not None:
        z = gots[zero]
        assert z["n_frames"] > 0
        log_eps = LOG_EPS32[feat_is_f32_pcm(batch)].view(np.uint32)
        if spec.out_kind == MFE:
            assert (z["feat"].view(np.uint32) == EPS32.view(np.uint32)).all()
        elif spec.out_kind == LMFE:
            assert (z["feat"].view(np.uint32) == log_eps).all()
        elif spec.dc_elimination:
            assert (z["feat"][:, 0].view(np.uint32) == log_eps).all()
        if en is not None:
            assert (z["energy"].view(np.uint32) == EPS32.view(np.uint32)).all()
    return gots


def run_case(eng, capfd, what, batch, spec, want_energy=True, M=None, expect=None):
    clips, zero = ragged_batch(batch)
    feat, nf, en, inst, waves, grid = launch(eng, capfd, clips, spec, want_energy=want_energy, max_frames=M)
    if expect is not None:
        assert inst == expect, (what, inst)
    gots = exact_checks(feat, nf, en, batch, spec, M, zero)
    v = judge("%s [%s, %d waves]" % (what, inst, waves), gots, batch, spec, M, energy=en is not None)
    assert v["left_out"] == 0.0
    assert v["ok"], (what, v)
    return feat, nf, en


@gpu
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "preemph"])
@pytest.mark.parametrize("name,mk,f32", SPECIALISED, ids=[s[0].replace(" ", "") for s in SPECIALISED])
def test_specialised_instances(engines, monkeypatch, capfd, name, mk, f32, pre):
    """The four compile-time specialised instances, with and without the fused pre-emphasis, each asserted to have run by
    the library's debug line; against the generic instance at rtol = atol = 1e-6 (the transform is instantiated with a
    different step count: no bit equality expected); and the log-mel configuration leaves its instance for the generic one
    as soon as the frame energies are asked for."""
    eng = engines()
    spec = mk(**(PRE if pre else {}))
    batch = batch_for(spec, f32)
    set_env(monkeypatch)
    energy = spec.out_kind == MFCC                     # SpecLmfe40 computes no frame energy
    feat, nf, _ = run_case(eng, capfd, "specialised %s%s" % (name, " pre" if pre else ""), batch, spec, energy, expect=name)
    set_env(monkeypatch, generic=1)
    gen, nf_g, _ = run_case(eng, capfd, "generic for %s%s" % (name, " pre" if pre else ""), batch, spec, energy,
                            expect="generic")
    assert np.array_equal(nf, nf_g)
    np.testing.assert_allclose(feat, gen, rtol=1e-6, atol=1e-6)
    if spec.out_kind == LMFE:
        set_env(monkeypatch)
        run_case(eng, capfd, "%s with energy asked" % name, batch, spec, True, expect="generic")


@gpu
@pytest.mark.parametrize("c", GENERIC_CASES, ids=[_id(c) for c in GENERIC_CASES])
def test_generic_instance(engines, monkeypatch, capfd, c):
    """The generic instance at the two standard configurations: tile 8 / 16, the four ways PCM is staged, the three output
    kinds, dc_elimination and the energy request -- the product pruned as the comment above GENERIC_CASES says."""
    cfg, tile, st, spec, energy = c
    set_env(monkeypatch, generic=1, tile=tile, f32stage=1 if st == "i16 f32stage" else None)
    run_case(engines(tile), capfd, "generic " + _id(c), batch_for(spec, st == "f32"), spec, energy, expect="generic")


@gpu
@pytest.mark.parametrize("what,spec", GEOMETRIES, ids=[g[0].replace(" ", "_") for g in GEOMETRIES])
def test_geometries(engines, monkeypatch, capfd, what, spec):
    """Geometries off the standard ones on the generic instance: frames of one register step, frames cut to nfft, the
    unaligned pair read of an odd hop, short and long hops, one to four filter tiles with a ragged last one, one and two
    (to four) cepstral tiles, the fifth untangling step of a bank that reaches bin 256, input_scale."""
    set_env(monkeypatch, generic=1)
    run_case(engines(), capfd, what, batch_for(spec), spec, True, expect="generic")


@gpu
@pytest.mark.parametrize("M", [40, 120])
def test_max_frames_below_and_above(engines, monkeypatch, capfd, M):
    """max_frames below the longest clip's count (rows and n_frames clamp) and above it (zero fill), on a specialised and
    on a generic instance."""
    set_env(monkeypatch)
    run_case(engines(), capfd, "max_frames %d mfcc13" % M, "i320", spec_a(**PRE), True, M=M, expect="mfcc13")
    run_case(engines(), capfd, "max_frames %d generic B" % M, "f400", spec_b(MFCC, **PRE), True, M=M, expect="generic")


# ---- bit for bit --------------------------------------------------------------------------------------------------------
def features(eng, *a, **kw):
    feat, nf, en = eng.features(*a, **kw)
    return feat, nf, en


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@gpu
@pytest.mark.parametrize("staging", ["raw16", "i16 f32stage", "f32"])
def test_offsets_alignment_and_clip_len_are_bit_identical(engines, monkeypatch, staging):
    """The same samples addressed in different ways give the same bits: a padded matrix with lengths; the clips
    concatenated at multiples of 8 samples and addressed by offsets (16-byte aligned staging); every start shifted by
    one sample (the patched, scalar staging); clip_len without lengths against lengths all equal."""
    eng = engines()
    f32 = staging == "f32"
    set_env(monkeypatch, f32stage=1 if staging == "i16 f32stage" else None)
    for spec in (spec_a(**PRE), spec_b(**PRE), spec_a(MFE)):
        clips = ragged_batch(batch_for(spec, f32))[0]
        pcm, lens = padded(clips)
        M = spec.num_frames(pcm.shape[1])
        base = features(eng, pcm, spec, lengths=lens, max_frames=M, want_energy=True)
        slots = (lens.astype(np.int64) + 7) // 8 * 8
        for shift in (0, 1):
            offs = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64) + shift
            buf = np.zeros(int(slots.sum()) + 8, dtype=pcm.dtype)
            for o, x in zip(offs, clips):
                buf[o:o + x.size] = x
            got = features(eng, buf, spec, lengths=lens, offsets=offs, max_frames=M, want_energy=True)
            assert same(base, got), (staging, spec.key(), shift)
        n = pcm.shape[1] - 37
        a = features(eng, pcm, spec, clip_len=n, want_energy=True)
        b = features(eng, pcm, spec, lengths=np.full(len(clips), n, dtype=np.int32), max_frames=spec.num_frames(n),
                     want_energy=True)
        assert same(a, b), (staging, spec.key())


@gpu
def test_batch_position_and_wave_count_are_bit_identical(engines, monkeypatch):
    """A clip alone gives the bits it gives at each position of a batch, and one wave per workgroup gives the bits of
    the library's own wave count."""
    eng = engines()
    for spec, f32 in ((spec_a(**PRE), False), (spec_b(**PRE), False), (spec_b(MFCC, **PRE), True)):
        set_env(monkeypatch)
        clips = ragged_batch(batch_for(spec, f32))[0][8:20]
        pcm, lens = padded(clips)
        M = spec.num_frames(pcm.shape[1])
        base = features(eng, pcm, spec, lengths=lens, max_frames=M, want_energy=True)
        x = clips[5]
        for pos in range(len(clips)):
            moved = list(clips)
            moved[pos] = x
            p2, l2 = padded(moved)
            got = features(eng, p2, spec, lengths=l2, max_frames=M, want_energy=True)
            alone = features(eng, p2[pos:pos + 1], spec, lengths=l2[pos:pos + 1], max_frames=M, want_energy=True)
            assert same([t[pos:pos + 1] for t in got], alone), (spec.key(), pos)
            assert same([t[pos] for t in got], [t[5] for t in base]), (spec.key(), pos)
        set_env(monkeypatch, waves=1)
        assert same(base, features(eng, pcm, spec, lengths=lens, max_frames=M, want_energy=True)), spec.key()


@gpu
def test_gathered_input_is_bit_identical(engines, monkeypatch):
    """d_src_chunk: an identity chunk table against plain input, and a table that picks every other 160-sample chunk of a
    longer buffer against that selection copied out contiguously; gathered lengths that are no multiple of the chunk, a
    clip with 0 chunks, with pre-emphasis (its wrap reads the LAST gathered sample)."""
    eng = engines()
    set_env(monkeypatch)
    chunk, n_chunks = 160, 50
    clips = [synth.noise_clip(500, 2 * chunk * n_chunks), synth.speaker_clip(3, 1, 2 * chunk * n_chunks),
             _tone_noise(9, 2 * chunk * n_chunks), synth.noise_clip(501, 2 * chunk * n_chunks)]
    long = np.stack(clips)
    lens = np.array([chunk * n_chunks, chunk * 31 + 77, 0, chunk * 7 + 159], dtype=np.int32)
    for spec in (spec_a(**PRE), spec_b(**PRE), spec_a(MFE), spec_b(MFCC)):
        M = spec.num_frames(chunk * n_chunks)
        plain = long[:, :chunk * n_chunks].copy()
        ident = torch.arange(n_chunks, dtype=torch.int32, device=eng.device).repeat(len(clips), 1).contiguous()
        a = features(eng, plain, spec, lengths=lens, max_frames=M, want_energy=True)
        b = features(eng, plain, spec, lengths=lens, max_frames=M, want_energy=True, gather=(ident, chunk))
        assert same(a, b), spec.key()
        assert int(a[1][2]) == 0 and not bool(b[0][2].any())
        # every other chunk, odd ones for odd clips
        table = np.stack([2 * np.arange(n_chunks) + (u & 1) for u in range(len(clips))]).astype(np.int32)
        picked = np.stack([long[u].reshape(-1, chunk)[table[u]].reshape(-1) for u in range(len(clips))])
        c = features(eng, picked, spec, lengths=lens, max_frames=M, want_energy=True)
        d = features(eng, long, spec, lengths=lens, max_frames=M, want_energy=True,
                     gather=(eng.to_device(table), chunk))
        assert same(c, d), spec.key()
        if spec.preemph:
            assert not torch.equal(a[0], c[0])                     # (the selection is another signal)


@gpu
@pytest.mark.parametrize("waves", [1, None], ids=["one_wave", "library_waves"])
def test_ticket_loop_later_rounds(engines, monkeypatch, capfd, waves):
    """More frame tiles than one round of the ticket loop hands out: 64 clips of 1 s at tile 8 are ~800 tiles; with one
    wave per workgroup a round is one tile per CU, so rounds 1.. are entered.  Against the reference with the bar, and
    bit for bit against the same clips run in batches of 8."""
    eng = engines()
    clips = ticket_batch()
    for spec in ticket_specs():
        set_env(monkeypatch, waves=waves)
        want_energy = spec.out_kind == MFCC
        feat, nf, en, inst, n_waves, grid = launch(eng, capfd, clips, spec, want_energy=want_energy)
        tiles = len(clips) * -(-spec.num_frames(FS) // 8)
        assert inst == ("mfcc13" if spec.out_kind == MFCC else "lmfe40") and (waves is None or n_waves == 1)
        if waves == 1:
            assert tiles > 2 * grid * n_waves, (tiles, grid, n_waves)       # the third round is entered
        key = "ticket"
        gots = exact_checks(feat, nf, en, key, spec)
        v = judge("ticket loop %s, %d tiles, grid %d [%s, %d waves]" % (_id(("-", 8, "", spec, want_energy)), tiles, grid,
                                                                        inst, n_waves), gots, key, spec,
                  energy=en is not None)
        assert v["ok"] and v["left_out"] == 0.0, v
        pcm, lens = padded(clips)
        M = feat.shape[1]
        for lo in range(0, len(clips), 8):
            part = eng.features(pcm[lo:lo + 8], spec, lengths=lens[lo:lo + 8], max_frames=M, want_energy=want_energy)
            assert np.array_equal(part[0].cpu().numpy().view(np.uint32), feat[lo:lo + 8].view(np.uint32)), (spec.key(), lo)
            assert np.array_equal(part[1].cpu().numpy(), nf[lo:lo + 8])
            if want_energy:
                assert np.array_equal(part[2].cpu().numpy().view(np.uint32), en[lo:lo + 8].view(np.uint32))
