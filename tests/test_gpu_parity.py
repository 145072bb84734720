"""GPU parity: every libsvk.so kernel, called through the C-ABI (ctypes) and through the
drop-in Python surface, against the CPU oracle and the committed golden vectors.

Tolerances (north-star): MFCC / log-mel allclose(rtol=1e-4, atol=1e-4) against the float64
reference (the kernels compute in f32; element-wise RELATIVE error alone is not meaningful
for cepstra that cross zero -- SURVEY.md section 7); cosine |d| <= 1e-5; VAD masks bit-exact;
EER equal.  The cosine tests here compare with the oracle's float32 product (the reference's own
numbers and the goldens); the score matrix is held to float64, on every kernel and branch of
svk_cosine_scores, in tests/test_scoring_float64.py (svk_l2_dist too).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import model_ref, scoring_ref, speechpy_ref as ref, vad_ref   # noqa: E402
from speaker_verification_amd import constants as c, synth                  # noqa: E402
from speaker_verification_amd import utils as _utils                        # noqa: E402,F401  (like the reference's utils.py:15 it seeds
#   the global NumPy RNG AT IMPORT: imported here, so that no test's own np.random.seed() is undone by a lazy first import)

FEAT_TOL = dict(rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(params=["default path", "long-clip path forced", "general one-kernel path forced"])
def clip_paths(request, monkeypatch):
    """svk_vad_energy / svk_cmvn pick a multi-kernel path for long clips (chunks of a clip on separate workgroups) and
    svk_vad_energy a small-LDS kernel for clips of at most 512 frames; the tests that take this fixture run with the
    library's own choice, with the long-clip path forced onto short clips, and with the general one-workgroup-per-clip
    kernels (sequential hysteresis walk; what unusual frame geometries still take)."""
    if request.param == "long-clip path forced":
        monkeypatch.setenv("SVK_VAD_SPLIT", "1")
        monkeypatch.setenv("SVK_CMVN_SPLIT", "1")
    elif request.param == "general one-kernel path forced":
        monkeypatch.setenv("SVK_VAD_SPLIT", "2")
        monkeypatch.setenv("SVK_CMVN_SPLIT", "0")
    return request.param


@pytest.fixture(scope="module")
def sp():
    from speaker_verification_amd import speechpy
    return speechpy


def test_native_library_is_loaded(eng):
    """The HIP extension must be the thing that ran (the driver checks /proc/self/maps too)."""
    with open("/proc/self/maps") as fh:
        assert "libsvk.so" in fh.read()
    assert eng.num_cu >= 64 and eng.wave == 64


# ---- fused front end against the golden vectors (reference outputs) ---------------------------
def test_mfcc_config_A_golden(sp, golden):
    g = golden["speechpy"]
    one = synth.noise_clip(*g["one_seed"])
    np.testing.assert_allclose(sp.feature.mfcc(one, 16000), g["mfcc_A"], **FEAT_TOL)
    np.testing.assert_allclose(sp.feature.mfcc(one, 16000, dc_elimination=False), g["mfcc_A_nodc"], **FEAT_TOL)
    np.testing.assert_allclose(sp.feature.mfcc(one, 16000, num_cepstral=40), g["mfcc_A_40"], **FEAT_TOL)
    np.testing.assert_allclose(sp.feature.mfcc(one, 16000, num_filters=26, low_frequency=100.0,
                                               high_frequency=7000.0), g["mfcc_A_lowhigh"], **FEAT_TOL)
    f, e = sp.feature.mfe(one, 16000)
    np.testing.assert_allclose(f, g["mfe_A_feat"], rtol=1e-4)
    np.testing.assert_allclose(e, g["mfe_A_energy"], rtol=1e-4)
    np.testing.assert_allclose(sp.feature.lmfe(one, 16000), g["lmfe_A"], **FEAT_TOL)
    spk = synth.speaker_clip(*g["spk_seed"])
    np.testing.assert_allclose(sp.feature.mfcc(spk, 16000), g["mfcc_A_spk"], **FEAT_TOL)


def test_lmfe_config_B_golden(sp, golden):
    g = golden["speechpy"]
    one_f32 = (synth.noise_clip(*g["one_seed"]) / 32768.0).astype(np.float32)
    np.testing.assert_allclose(sp.feature.lmfe(one_f32, 16000, 0.025, 0.01, 40, 1024), g["lmfe_B_f32"], **FEAT_TOL)
    np.testing.assert_allclose(sp.feature.mfcc(one_f32, 16000, 0.025, 0.01, 13, 40, 1024), g["mfcc_B_f32"],
                               **FEAT_TOL)
    spk = synth.speaker_clip(*g["spk_seed"])
    np.testing.assert_allclose(sp.feature.lmfe(spk, 16000, 0.025, 0.01, 40, 1024), g["lmfe_B_spk"], **FEAT_TOL)


def test_known_answers_3s(sp, golden):
    g = golden["speechpy"]
    sig = (np.random.default_rng(0).standard_normal(48000) * 3000).astype(np.int16)
    m = sp.feature.mfcc(sig, 16000)
    assert m.shape == (298, 13) and m.dtype == np.float64
    np.testing.assert_allclose(m, g["kat_mfcc_A_3s"], **FEAT_TOL)
    assert m.sum() == pytest.approx(4545.562374768052, abs=0.05)
    b = sp.feature.lmfe(sig.astype(np.float32) / 32768, 16000, 0.025, 0.01, 40, 1024)
    assert b.shape == (297, 40)
    np.testing.assert_allclose(b, g["kat_lmfe_B_3s"], **FEAT_TOL)
    # fused pre-emphasis + separate CMVN == the reference chain preemphasis -> mfcc -> cmvn(var)
    pre = sp.feature.mfcc(sp.processing.preemphasis(sig, cof=0.98), 16000)
    np.testing.assert_allclose(sp.processing.cmvn(pre, True), g["kat_mfcc_A_3s_pre_cmvn"], rtol=1e-3, atol=1e-3)


def test_zero_and_short_clips(sp, golden):
    g = golden["speechpy"]
    z = sp.feature.mfcc(np.zeros(1600, dtype=np.int16), 16000)
    np.testing.assert_allclose(z, g["mfcc_A_zero"], rtol=0, atol=1e-5)          # Q7: log(eps) in c0, 0 elsewhere
    assert z[0, 0] == pytest.approx(-36.04365338911715, abs=1e-5)
    assert sp.feature.mfcc(np.zeros(320, dtype=np.int16), 16000).shape == (0, 13)   # feature.py:144-145
    assert sp.feature.mfcc(np.zeros(10, dtype=np.int16), 16000).shape == (0, 13)
    f, e = sp.feature.mfe(np.zeros(100, dtype=np.int16), 16000)
    assert f.shape == (0, 40) and e.shape == (0,)


# ---- batched front end through the engine (C-ABI) against the oracle ------------------------------
@pytest.mark.parametrize("kind,nfft,fl,ncep", [("mfcc", 512, 0.020, 13), ("lmfe", 1024, 0.025, 40),
                                               ("mfe", 512, 0.020, 13), ("mfcc", 1024, 0.025, 40)])
def test_batched_ragged(eng, kind, nfft, fl, ncep):
    from speaker_verification_amd.speechpy import feature
    lens = [48000, 16000, 9999, 2723, 400, 320, 47999, 33333]
    L = max(lens)
    pcm = np.zeros((len(lens), L), dtype=np.int16)
    for i, n in enumerate(lens):
        pcm[i, :n] = synth.speaker_clip(i, 0, n) if i % 2 else synth.noise_clip(100 + i, n)
    feat, n_frames, energy = feature.features_batch(pcm, 16000, kind=kind, frame_length=fl, num_cepstral=ncep,
                                                    fft_length=nfft, lengths=np.array(lens, dtype=np.int32),
                                                    want_energy=True)
    feat, n_frames, energy = feat.cpu().numpy(), n_frames.cpu().numpy(), energy.cpu().numpy()
    fn = {"mfcc": ref.mfcc, "lmfe": ref.lmfe, "mfe": lambda *a, **k: ref.mfe(*a, **k)[0]}[kind]
    for i, n in enumerate(lens):
        kw = dict(frame_length=fl, frame_stride=0.01, num_filters=40, fft_length=nfft)
        if kind == "mfcc":
            kw["num_cepstral"] = ncep
        want = fn(pcm[i, :n], 16000, **kw)
        assert n_frames[i] == want.shape[0], (i, n)
        if kind == "mfe":
            np.testing.assert_allclose(feat[i, :want.shape[0]], want, rtol=1e-4)
        else:
            np.testing.assert_allclose(feat[i, :want.shape[0]], want, **FEAT_TOL)
        assert not feat[i, want.shape[0]:].any()                                   # padded rows are zero
        np.testing.assert_allclose(energy[i, :want.shape[0]], ref.mfe(pcm[i, :n], 16000, **{
            k: v for k, v in kw.items() if k != "num_cepstral"})[1], rtol=1e-4)


def test_fused_preemphasis_matches_reference_chain(eng):
    from speaker_verification_amd.speechpy import feature
    pcm = np.stack([synth.noise_clip(5, 16000), synth.speaker_clip(2, 0, 16000)])
    feat, _, _ = feature.features_batch(pcm, 16000, kind="mfcc", preemphasis_cof=0.98)
    for i in range(2):
        want = ref.mfcc(ref.preemphasis(pcm[i], cof=0.98), 16000)
        np.testing.assert_allclose(feat[i].cpu().numpy(), want, **FEAT_TOL)
    # float32 PCM in [-1, 1)
    f32 = (pcm / 32768.0).astype(np.float32)
    feat, _, _ = feature.features_batch(f32, 16000, kind="lmfe", frame_length=0.025, fft_length=1024,
                                        preemphasis_cof=0.97)
    for i in range(2):
        want = ref.lmfe(ref.preemphasis(f32[i], cof=0.97), 16000, 0.025, 0.01, 40, 1024)
        np.testing.assert_allclose(feat[i].cpu().numpy(), want, **FEAT_TOL)


def want_rows(n_samples, frame_length, fs=16000, stride=160):
    flen = int(round(fs * frame_length))
    return max(0, (n_samples - flen) // stride) if n_samples >= flen else 0


@pytest.mark.parametrize("kind,nfft,fl", [("mfcc", 512, 0.020), ("lmfe", 1024, 0.025)])
def test_specialised_instances_match_generic_and_oracle(eng, kind, nfft, fl, monkeypatch):
    """The two standard configurations run compile-time specialised kernel instances (frontend.hip,
    SpecMfcc13 / SpecLmfe40); SVK_FE_GENERIC forces the generic instance on the same input."""
    from speaker_verification_amd.speechpy import feature
    lens = [48000, 47999, 16001, 9999, 2723, 1280 + 320, 400, 319, 33333, 48000]
    pcm = np.zeros((len(lens), max(lens)), dtype=np.int16)
    for i, n in enumerate(lens):
        pcm[i, :n] = synth.speaker_clip(i, 1, n) if i % 2 else synth.noise_clip(200 + i, n)
    kw = dict(kind=kind, frame_length=fl, fft_length=nfft, preemphasis_cof=0.98,
              lengths=np.array(lens, dtype=np.int32))
    # without the fused pre-emphasis (the plain speechpy call) the same specialised instance runs
    plain = {k: v for k, v in kw.items() if k != "preemphasis_cof"}
    a, _, _ = feature.features_batch(pcm, 16000, **plain)
    monkeypatch.setenv("SVK_FE_GENERIC", "1")
    b, _, _ = feature.features_batch(pcm, 16000, **plain)
    monkeypatch.delenv("SVK_FE_GENERIC")
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(a[0].cpu().numpy(), (ref.mfcc if kind == "mfcc" else ref.lmfe)(
        pcm[0], 16000, frame_length=fl, frame_stride=0.01, num_filters=40, fft_length=nfft), **FEAT_TOL)
    # float32 signals in [-1, 1) (what librosa hands the reference's lmfe call) have their own two instances
    f32 = (pcm / 32768.0).astype(np.float32)
    fa, _, _ = feature.features_batch(f32, 16000, **kw)
    monkeypatch.setenv("SVK_FE_GENERIC", "1")
    fb, _, _ = feature.features_batch(f32, 16000, **kw)
    monkeypatch.delenv("SVK_FE_GENERIC")
    np.testing.assert_allclose(fa.cpu().numpy(), fb.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(fa[1, :want_rows(lens[1], fl)].cpu().numpy(), (ref.mfcc if kind == "mfcc" else ref.lmfe)(
        ref.preemphasis(f32[1, :lens[1]], cof=0.98), 16000, frame_length=fl, frame_stride=0.01, num_filters=40,
        fft_length=nfft), **FEAT_TOL)
    spec, nf_spec, _ = feature.features_batch(pcm, 16000, **kw)
    monkeypatch.setenv("SVK_FE_GENERIC", "1")
    gen, nf_gen, _ = feature.features_batch(pcm, 16000, **kw)
    monkeypatch.delenv("SVK_FE_GENERIC")
    assert torch.equal(nf_spec, nf_gen)
    np.testing.assert_allclose(spec.cpu().numpy(), gen.cpu().numpy(), rtol=1e-6, atol=1e-6)
    fn = ref.mfcc if kind == "mfcc" else ref.lmfe
    for i, n in enumerate(lens):
        want = fn(ref.preemphasis(pcm[i, :n], cof=0.98), 16000, frame_length=fl, frame_stride=0.01, num_filters=40,
                  fft_length=nfft)
        assert int(nf_spec[i]) == want.shape[0]
        np.testing.assert_allclose(spec[i, :want.shape[0]].cpu().numpy(), want, **FEAT_TOL)
        assert not spec[i, want.shape[0]:].any()


def test_long_clips_front_end(eng):
    """VoxCeleb clips run to 145 s: one 60 s and one 7 s clip in a batch (thousands of frame tiles per clip,
    more tiles than waves in flight), both configurations, against the oracle."""
    from speaker_verification_amd.speechpy import feature
    lens = [60 * 16000 + 123, 7 * 16000]
    pcm = np.zeros((2, lens[0]), dtype=np.int16)
    pcm[0] = synth.noise_clip(31, lens[0])
    pcm[1, :lens[1]] = synth.speaker_clip(3, 2, lens[1])
    for kind, nfft, fl, fn in (("mfcc", 512, 0.020, ref.mfcc), ("lmfe", 1024, 0.025, ref.lmfe)):
        feat, nf, _ = feature.features_batch(pcm, 16000, kind=kind, frame_length=fl, fft_length=nfft,
                                             preemphasis_cof=0.98, lengths=np.array(lens, dtype=np.int32))
        for i, n in enumerate(lens):
            want = fn(ref.preemphasis(pcm[i, :n], cof=0.98), 16000, frame_length=fl, frame_stride=0.01,
                      num_filters=40, fft_length=nfft)
            assert int(nf[i]) == want.shape[0]
            np.testing.assert_allclose(feat[i, :want.shape[0]].cpu().numpy(), want, **FEAT_TOL)
            assert not feat[i, want.shape[0]:].any()


def test_ragged_embeddings_of_very_long_clips(eng):
    """SURVEY 8f-2 / load_data.py:23-53: VoxCeleb utterances run from 4 to 145 s.  A 145 s, a 4 s and a 31 s clip through
    `embed_ragged` (host list) and `embed_ragged_resident` (one device buffer + offsets): EMBEDDINGS against the CPU
    oracle chain (vad -> /32768 -> preemphasis -> lmfe -> cmvn -> cube at the device-drawn crops -> C3D2)."""
    from speaker_verification_amd.model import calibrate_batchnorm, perturb_inference_state, seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    model = seeded_model(61, n_labels=8)
    model.load_state_dict(perturb_inference_state(model.state_dict(), 62))
    pipe = VerificationPipeline(model, use_vad=True, normalize=True, preemph_cof=0.98, crop_rng="device", crop_seed=5,
                                micro_batch=2)
    lens = [145 * 16000, 4 * 16000, 31 * 16000 + 77]
    clips = [np.concatenate([synth.speaker_clip(20 + k, u) for u in range(-(-n // 48000))])[:n] for k, n in enumerate(lens)]
    # calibrated BatchNorm statistics (a well-conditioned embedding, as in the end-to-end test)
    base = VerificationPipeline(model, use_vad=True, normalize=True, preemph_cof=0.98, crop_rng="device", crop_seed=5)
    _, cal = base.crops_and_cubes(np.stack([c_[:48000] for c_ in clips] + [synth.speaker_clip(30, 1), synth.speaker_clip(31, 2)]))
    calibrate_batchnorm(pipe.model, cal)
    pipe.refresh_model()
    first = 700
    got = pipe.embed_ragged(clips, first_utt=first).cpu().numpy()
    slots = [(n + 7) // 8 * 8 for n in lens]
    offs = np.concatenate([[0], np.cumsum(slots)[:-1]])
    buf = np.zeros(sum(slots), dtype=np.int16)
    for k, x in enumerate(clips):
        buf[offs[k]:offs[k] + x.size] = x
    got_r = pipe.embed_ragged_resident(buf, offs, np.array(lens), first_utt=first).cpu().numpy()
    np.testing.assert_array_equal(got_r, got)                          # the same kernels on the same bytes
    # the arena on the device already; and a host arena uploaded in PIECES on a side stream (three upload groups here, the
    # clips of a piece running while the next travels), the clips in another arena order than list order
    got_d = pipe.embed_ragged_resident(torch.as_tensor(buf, device=eng.device), offs, np.array(lens), first_utt=first).cpu().numpy()
    np.testing.assert_array_equal(got_d, got)
    got_p = pipe.embed_ragged_resident(buf, offs, np.array(lens), max_batch_samples=600_000, first_utt=first).cpu().numpy()
    np.testing.assert_array_equal(got_p, got)
    rev = np.array([2, 0, 1])
    got_s = pipe.embed_ragged_resident(buf, offs[rev], np.array(lens)[rev], max_batch_samples=600_000, first_utt=first).cpu().numpy()
    for k, src_k in enumerate(rev):                                    # (crop draws are keyed by the index in the caller's list)
        assert got_s[k].shape == got[src_k].shape and np.isfinite(got_s[k]).all()
    assert int(pipe.bad_clips.item()) == 0
    state = {k: v.detach().cpu() for k, v in pipe.model.state_dict().items()}
    for k, x in enumerate(clips):
        _, _, voiced = vad_ref.vad_energy(x, 16000, c.VAD_FRAME_MS, c.VAD_PADDING_MS, c.VAD_ENERGY_THRESHOLD)
        feat = ref.cmvn(ref.lmfe(ref.preemphasis(voiced / 32768.0, cof=0.98), 16000, c.FRAME_LEN, c.FRAME_STEP, c.NUM_COEF,
                                 c.NUM_FFT), variance_normalization=True)
        crops = eng.draw_crops(np.array([feat.shape[0]], dtype=np.int32), c.CUBE_CROPS, c.CUBE_FRAMES, 5, 0,
                               utt_index=np.array([first + k])).cpu().numpy()[0]
        assert crops.min() >= 0 and crops.max() + 80 <= feat.shape[0] and (k != 0 or crops.max() > 5000)
        want = model_ref.c3d2_embed(state, model_ref.feature_cube(feat, crops)[None]).numpy()[0]
        err = np.abs(got[k] - want).max() / np.abs(want).max()
        print("ragged clip of %5.1f s: %d frames, embedding max |diff| / scale %.2e" % (lens[k] / 16000, feat.shape[0], err))
        np.testing.assert_allclose(got[k], want, rtol=0, atol=5e-5 * np.abs(want).max())
    with pytest.raises(ValueError):
        pipe.embed_ragged_resident(buf, offs + 1, np.array(lens))       # offsets must be 16-byte aligned


def test_long_clip_paths_equal_the_one_kernel_paths(eng, monkeypatch):
    """The multi-kernel VAD (bit for bit) and CMVN (float64 sums in another order: 1e-6) against the one-workgroup-per-clip
    kernels on clips of 145 s, 40 s, 3 s and 0.5 s, addressed by offsets and as a padded matrix; VAD also against the oracle."""
    lens = [145 * 16000 + 5, 40 * 16000, 48000, 8000]
    clips = [np.concatenate([synth.speaker_clip(50 + k, u) for u in range(-(-n // 48000))])[:n] for k, n in enumerate(lens)]
    slots = [(n + 7) // 8 * 8 for n in lens]
    offs = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64)
    buf = np.zeros(sum(slots), dtype=np.int16)
    for k, x in enumerate(clips):
        buf[offs[k]:offs[k] + x.size] = x
    out = {}
    for mode in ("0", "1"):     # (SVK_VAD_SPLIT=0: clips this long take the general one-kernel path)
        monkeypatch.setenv("SVK_VAD_SPLIT", mode)
        monkeypatch.setenv("SVK_CMVN_SPLIT", mode)
        res = eng.vad_energy(buf, c.VAD_ENERGY_THRESHOLD, lengths=np.array(lens, dtype=np.int32), offsets=offs, want_segments=True)
        vlen = res["voiced_len"].cpu().numpy()
        voiced = res["voiced"].cpu().numpy()
        feat = torch.randn((4, 14600, 40), device=eng.device, generator=torch.Generator(device=eng.device).manual_seed(1)) * 3 - 7
        nf = np.array([14499, 3999, 297, 0], dtype=np.int32)
        eng.cmvn_(feat, nf, variance=True)
        out[mode] = (res["keep"].cpu().numpy(), res["seg"].cpu().numpy(), res["n_vad_frames"].cpu().numpy(), vlen,
                     [voiced[offs[k]:offs[k] + vlen[k]] for k in range(4)], feat.cpu().numpy())
    for a, b in zip(out["0"][:4], out["1"][:4]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(out["0"][4], out["1"][4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(out["1"][5], out["0"][5], rtol=0, atol=2e-6)
    for k in (0, 3):
        keep, seg, v = vad_ref.vad_energy(clips[k], 16000, c.VAD_FRAME_MS, c.VAD_PADDING_MS, c.VAD_ENERGY_THRESHOLD)
        np.testing.assert_array_equal(out["1"][0][k, :keep.size].astype(bool), keep)
        np.testing.assert_array_equal(out["1"][4][k], v)


def test_vad_main_chunks_a_file_tree(eng, tmp_path, monkeypatch):
    """vad.main() (vad.py:135-168): id list -> voiced segments as `wav_chunked/<name>_<i>.wav` + the new id list, against
    the oracle's collector file by file (the reference's own collector is pinned to that oracle by the golden VAD cases)."""
    import wave
    from speaker_verification_amd import constants, vad
    root, data = tmp_path / "root", tmp_path / "data"
    (data / "wav" / "id10001" / "rec").mkdir(parents=True)
    (data / "wav" / "id10002" / "rec").mkdir(parents=True)
    root.mkdir()
    clips = {"id10001/rec/00001.wav": (synth.speaker_clip(3, 0, 64000), 16000), "id10001/rec/00002.wav": (synth.speaker_clip(3, 1, 90001), 16000),
             "id10002/rec/00001.wav": (synth.speaker_clip(4, 0, 40000, fs=8000), 8000), "id10002/rec/00002.wav": (synth.noise_clip(5, 20000, 50.0), 16000)}
    for name, (pcm, rate) in clips.items():
        vad.write_wave(str(data / "wav" / name), pcm.tobytes(), rate)
    np.savetxt(root / "100_first_ids_100_samples.txt", np.array(list(clips)), fmt="%s")
    monkeypatch.setattr(constants, "ROOT", str(root))
    monkeypatch.setattr(constants, "DATA_ORIGIN", str(data))
    monkeypatch.chdir(tmp_path)
    written = vad.main()
    assert [ln.strip() for ln in open(tmp_path / "100_speakers_100_samples_chunked_ids.txt")] == written
    want_names = []
    for name, (pcm, rate) in clips.items():
        keep, seg, _ = vad_ref.vad_energy(pcm, rate, c.VAD_FRAME_MS, c.VAD_PADDING_MS, c.VAD_ENERGY_THRESHOLD)
        n = int(rate * 0.03)
        for i in range(int(seg.max()) + 1 if seg.size else 0):
            out = name.replace(".wav", "_%d.wav" % i)
            want_names.append(out)
            with wave.open(str(data / "wav_chunked" / out), "rb") as wf:
                assert wf.getframerate() == rate and wf.getnchannels() == 1
                got = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16)
            np.testing.assert_array_equal(got, np.concatenate([pcm[f * n:(f + 1) * n] for f in np.nonzero(seg == i)[0]]))
    assert written == want_names and len(written) >= 3                     # the quiet noise clip yields no segment


def test_full_size_batch_properties(eng):
    """BASELINE config 2 shape (1 024 x 3 s): determinism, row independence, no NaN."""
    from speaker_verification_amd.speechpy import feature
    base = np.stack([synth.noise_clip(s) for s in range(8)])
    pcm = np.tile(base, (128, 1))
    a, nf, _ = feature.features_batch(pcm, 16000, kind="mfcc")
    b, _, _ = feature.features_batch(pcm, 16000, kind="mfcc")
    assert a.shape == (1024, 298, 13) and bool((nf == 298).all())
    assert torch.equal(a, b)                                            # bitwise repeatable
    assert torch.equal(a[:8], a[512:520])                               # same clip -> same bits anywhere in the batch
    assert bool(torch.isfinite(a).all())
    np.testing.assert_allclose(a[3].cpu().numpy(), ref.mfcc(base[3], 16000), **FEAT_TOL)


# ---- stage-level drop-ins ------------------------------------------------------------------------
def test_processing_stages(sp, golden):
    g = golden["speechpy"]
    short = synth.noise_clip(*g["short_seed"])
    out = sp.processing.preemphasis(short, shift=1, cof=0.98)
    assert out.dtype == np.float64 and out.shape == short.shape
    np.testing.assert_allclose(out, g["pre_short_i16"], rtol=1e-6, atol=1e-3)
    f32 = sp.processing.preemphasis((short / 32768.0).astype(np.float32), shift=1, cof=0.98)
    assert f32.dtype == np.float32
    np.testing.assert_allclose(f32, g["pre_short_f32"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(sp.processing.preemphasis(short, shift=3, cof=0.5), g["pre_short_shift3"],
                               rtol=1e-6, atol=1e-3)
    x = short.astype(float)
    ones = lambda n: np.ones((n,))                                           # noqa: E731
    np.testing.assert_array_equal(sp.processing.stack_frames(x, 16000, 0.020, 0.010, ones, False), g["frames_nopad"])
    np.testing.assert_array_equal(sp.processing.stack_frames(x, 16000, 0.020, 0.020, ones, True), g["frames_pad"])
    np.testing.assert_allclose(sp.processing.stack_frames(x, 16000, 0.025, 0.010, np.hamming, True),
                               g["frames_hamming"], rtol=1e-6, atol=1e-3)
    fr = g["frames_nopad"]
    scale = float(np.abs(g["fftmag_512"]).max())
    np.testing.assert_allclose(sp.processing.fft_spectrum(fr, 512), g["fftmag_512"], rtol=1e-4, atol=2e-6 * scale)
    pmax = float(g["pow_512"].max())
    np.testing.assert_allclose(sp.processing.power_spectrum(fr, 512), g["pow_512"], rtol=1e-4, atol=2e-6 * pmax)
    np.testing.assert_allclose(sp.processing.power_spectrum(g["frames_hamming"], 1024), g["pow_1024"], rtol=1e-4,
                               atol=2e-6 * float(g["pow_1024"].max()))
    np.testing.assert_allclose(sp.processing.power_spectrum(fr, 256), g["pow_256_crop"], rtol=1e-4,
                               atol=2e-6 * float(g["pow_256_crop"].max()))     # direct-DFT path, cropped frames
    np.testing.assert_allclose(sp.processing.log_power_spectrum(fr, 512, True), g["logpow_512_norm"], rtol=0, atol=2e-2)


def test_reference_own_tests(sp):
    """What /root/reference/speech_feature_extraction/tests/test_speechpy.py asserts."""
    rng = np.random.default_rng(1)
    signal = rng.normal(0, 0.1, 200000)
    pre = sp.processing.preemphasis(signal, cof=0.98)
    assert pre.ndim == 1 and pre.shape == signal.shape
    frames = sp.processing.stack_frames(signal, sampling_frequency=16000, frame_length=0.02, frame_stride=0.02,
                                        filter=lambda x: np.ones((x,)), zero_padding=True)
    assert frames.shape[0] == int(np.ceil((signal.shape[0] - 320) / 320))
    fv = rng.random((50, 100))
    norm = sp.processing.cmvn(fv, variance_normalization=True)
    assert norm.shape == fv.shape
    assert np.allclose(np.mean(norm, axis=0), 0, atol=1e-6) and np.allclose(np.std(norm, axis=0), 1, atol=1e-5)
    assert sp.feature.mfcc(signal, sampling_frequency=16000, frame_length=0.020, num_cepstral=13, frame_stride=0.01,
                           num_filters=40, fft_length=512, low_frequency=0, high_frequency=None).shape[1] == 13
    for mod, names in ((sp.processing, "preemphasis stack_frames fft_spectrum power_spectrum log_power_spectrum "
                                       "derivative_extraction cmvn cmvnw"),
                       (sp.feature, "filterbanks mfcc mfe lmfe extract_derivative_feature"),
                       (sp.functions, "frequency_to_mel mel_to_frequency triangle zero_handling")):
        for name in names.split():
            assert hasattr(mod, name)


def test_postprocessing(sp, golden, clip_paths):
    g = golden["speechpy"]
    base = g["mfcc_A"]
    np.testing.assert_allclose(sp.processing.cmvn(base, False), g["cmvn_mean"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sp.processing.cmvn(base, True), g["cmvn_var"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sp.processing.cmvn(g["cmvn_wide_in"], True), g["cmvn_wide_var"], rtol=1e-4, atol=1e-5)
    out = sp.processing.cmvnw(base, win_size=301, variance_normalization=True)
    assert out.dtype == np.float32
    np.testing.assert_allclose(out, g["cmvnw_var"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(sp.processing.cmvnw(base, 31, True), g["cmvnw_var_w31"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(sp.processing.cmvnw(base, 301, False), g["cmvnw_mean"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(sp.processing.derivative_extraction(base, 2), g["deriv_w2"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sp.feature.extract_derivative_feature(g["lmfe_A"]), g["deriv_cube"], rtol=1e-5,
                               atol=1e-5)
    with pytest.raises(AssertionError):
        sp.processing.cmvnw(base, win_size=300)


def test_cmvnw_derivative_batched(eng):
    rng = np.random.default_rng(4)
    feat = (rng.standard_normal((3, 120, 13)) * 2 + 0.5).astype(np.float32)
    nf = np.array([120, 37, 5], dtype=np.int32)
    for win, var in ((31, True), (301, False), (9, True)):
        got = eng.cmvnw(feat, win_size=win, variance=var, n_frames=nf).cpu().numpy()
        for i, n in enumerate(nf):
            want = ref.cmvnw(feat[i, :n].astype(np.float64), win_size=win, variance_normalization=var)
            np.testing.assert_allclose(got[i, :n], want, rtol=1e-4, atol=1e-4)
            np.testing.assert_array_equal(got[i, n:], feat[i, n:])
    d = eng.derivative(feat, 2).cpu().numpy()
    for i in range(3):
        np.testing.assert_allclose(d[i], ref.derivative_extraction(feat[i].astype(np.float64), 2), rtol=1e-5, atol=1e-5)
    power = np.abs(rng.standard_normal((7, 257))).astype(np.float32) ** 2
    power[0, :3] = 0.0
    lp = eng.log_power_(eng.to_device(power).clone(), normalize=True).cpu().numpy()
    want = 10 * np.log10(np.maximum(power.astype(np.float64), 1e-20))
    np.testing.assert_allclose(lp, want - want.max(), rtol=0, atol=2e-4)
    assert lp.max() == 0.0


def test_cmvn_batched_ragged(eng, clip_paths):
    rng = np.random.default_rng(3)
    feat = rng.standard_normal((5, 60, 13)).astype(np.float32) * 3 + 1
    nf = np.array([60, 1, 17, 0, 59], dtype=np.int32)
    dev = eng.to_device(feat).clone()
    eng.cmvn_(dev, nf, variance=True)
    got = dev.cpu().numpy()
    for i, n in enumerate(nf):
        if n:
            np.testing.assert_allclose(got[i, :n], ref.cmvn(feat[i, :n].astype(np.float64), True), rtol=1e-4, atol=1e-5)
        np.testing.assert_array_equal(got[i, n:], feat[i, n:])               # rows past n_frames untouched


# ---- VAD: bit-exact ---------------------------------------------------------------------------------
def test_front_end_reads_voiced_frames_through_the_index(eng, clip_paths):
    """svk_vad_energy's index output (d_src_frame) + svk_frontend_run's gathered input (d_src_chunk): the front end reads the
    kept 30 ms frames where they lie -- the same keep mask and lengths as the copying form, src_frame = the kept frames in
    order, and BIT-IDENTICAL features to those computed from the compacted copy (same samples, same arithmetic); fixed-length
    and ragged batches, all three VAD paths, both fused configurations, with pre-emphasis (its circular wrap reads the LAST
    voiced sample), a silent clip, a clip that is kept whole and a 70 s clip."""
    from speaker_verification_amd import _lib
    from speaker_verification_amd.engine import spec_from_seconds
    thr = c.VAD_ENERGY_THRESHOLD
    specs = (spec_from_seconds(16000, 0.025, 0.01, 1024, 40, 40, _lib.OUT_LMFE, preemph=True, preemph_cof=0.98, input_scale=1.0 / 32768.0),
             spec_from_seconds(16000, 0.020, 0.01, 512, 40, 13, _lib.OUT_MFCC))
    pcm, _ = synth.corpus(3, 3)
    pcm[4] = 0                                                              # a silent clip: nothing kept
    pcm[5] = synth.noise_clip(5)                                            # loud throughout: every frame kept
    dev = eng.to_device(pcm)
    res_c = eng.vad_energy(dev, thr, compact=True)
    res_i = eng.vad_energy(dev, thr, compact="index")
    assert res_i["voiced"] is None and torch.equal(res_c["keep"], res_i["keep"]) and torch.equal(res_c["voiced_len"], res_i["voiced_len"])
    keep, src = res_i["keep"].cpu().numpy(), res_i["src_frame"].cpu().numpy()
    vlen = res_i["voiced_len"].cpu().numpy()
    assert vlen[4] == 0 and vlen[5] == keep.shape[1] * res_i["frame_samples"]
    for u in range(pcm.shape[0]):
        kept = np.nonzero(keep[u])[0]
        np.testing.assert_array_equal(src[u, :kept.size], kept)
    for spec in specs:
        f_c, n_c, _ = eng.features(res_c["voiced"], spec, lengths=res_c["voiced_len"])
        f_i, n_i, _ = eng.features(dev, spec, lengths=res_i["voiced_len"], gather=(res_i["src_frame"], res_i["frame_samples"]))
        assert torch.equal(n_c, n_i) and torch.equal(f_c, f_i), spec.key()
        assert int(n_i[4]) == 0 and not bool(f_i[4].any())
    # ragged: clips of 1.3 .. 70 s back to back at 16-byte-aligned offsets
    rng = np.random.default_rng(23)
    lens = np.array([20800, 48000, 1120000, 64007, 333333, 9000], dtype=np.int32)
    clips = [np.tile(synth.speaker_clip(7 + k, k), -(-int(n) // 48000))[:n] for k, n in enumerate(lens)]
    slots = (lens.astype(np.int64) + 7) // 8 * 8
    offs = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64)
    buf = np.zeros(int(slots.sum()), dtype=np.int16)
    for o, x in zip(offs, clips):
        buf[o:o + x.size] = x
    dbuf = eng.to_device(buf)
    r_c = eng.vad_energy(dbuf, thr, lengths=lens, offsets=offs, compact=True)
    r_i = eng.vad_energy(dbuf, thr, lengths=lens, offsets=offs, compact="index")
    assert torch.equal(r_c["keep"], r_i["keep"]) and torch.equal(r_c["voiced_len"], r_i["voiced_len"])
    spec = specs[0]
    T = spec.num_frames(int(lens.max()))
    f_c, n_c, _ = eng.features(r_c["voiced"], spec, lengths=r_c["voiced_len"], offsets=offs, max_frames=T)
    f_i, n_i, _ = eng.features(dbuf, spec, lengths=r_i["voiced_len"], offsets=offs, max_frames=T, gather=(r_i["src_frame"], r_i["frame_samples"]))
    assert torch.equal(n_c, n_i) and torch.equal(f_c, f_i) and int(n_i.max()) > 3000
    # what the gathered form is not built for is refused, not silently computed from something else
    with pytest.raises(_lib.SvkError):
        eng.features(dev.to(torch.float32), specs[0], lengths=res_i["voiced_len"], gather=(res_i["src_frame"], res_i["frame_samples"]))
    with pytest.raises(_lib.SvkError):
        eng.features(dev, specs[0], lengths=res_i["voiced_len"], gather=(res_i["src_frame"], 484))
    with pytest.raises(ValueError):
        eng.features(dev, specs[0], gather=(res_i["src_frame"], res_i["frame_samples"]))


def test_cmvn_folded_into_the_cube_gather(eng, clip_paths):
    """svk_cmvn_stats + svk_cube_gather_cmvn (utils.py:382-397 CMVN feeding utils.py:351-379 FeatureCube in one pass over the
    20 x 80 rows the cube holds) against svk_cmvn in place followed by svk_cube_gather: bit-identical on every CMVN path,
    ragged frame counts, a clip with no frames, a too-short clip (crop -1 -> zero cube), 40 and 13 columns; the statistics
    against the float64 oracle."""
    rng = np.random.default_rng(17)
    for n, T, C in ((7, 300, 40), (5, 1500, 40), (4, 260, 13)):
        feat = (rng.standard_normal((n, T, C)) * 3.0 - 5.0).astype(np.float32)
        nf = rng.integers(100, T + 1, size=n).astype(np.int32)
        nf[0], nf[1] = T, 0
        crops = np.stack([rng.integers(0, max(1, int(t) - 80), size=20) for t in nf]).astype(np.int32)
        crops[1] = -1
        crops[2] = -1                                                   # declared too short although it has frames
        raw = eng.to_device(feat)
        stats = eng.cmvn_stats(raw, nf, variance=True)
        assert torch.equal(raw, eng.to_device(feat))                    # the features stay raw
        got = eng.cube_gather(raw, crops, 80, stats=stats)
        want = eng.cube_gather(eng.cmvn_(raw.clone(), nf, variance=True), crops, 80)
        assert torch.equal(got, want), (n, T, C, clip_paths)
        assert not got[1].any() and not got[2].any()
        for u in range(n):
            if nf[u] > 0:
                x = feat[u, :nf[u]].astype(np.float64)
                np.testing.assert_allclose(stats[u, 0].cpu().numpy(), x.mean(0), rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(stats[u, 1].cpu().numpy(), 1.0 / (x.std(0) + 2.0 ** -30), rtol=1e-9)
        mean_only = eng.cmvn_stats(raw, nf, variance=False)
        assert torch.equal(eng.cube_gather(raw, crops, 80, stats=mean_only),
                           eng.cube_gather(eng.cmvn_(raw.clone(), nf, variance=False), crops, 80))
    with pytest.raises(ValueError):
        eng.cube_gather(raw, crops, 80, stats=stats[:, :1])
    assert eng.lib.svk_cmvn_stats(eng.ctx, None, 1, 10, 4, None, 1, None) == -1
    assert eng.lib.svk_cube_gather_cmvn(eng.ctx, None, 1, 100, 40, None, 20, 80, None, None) == -1


def test_vad_bit_exact(eng, golden, clip_paths):
    g = golden["vad"]
    thr = int(g["threshold"][0])
    clips = [synth.speaker_clip(s, u) for s, u in ((0, 0), (1, 4), (7, 2), (3, 3), (9, 1))]
    clips += [synth.noise_clip(3, 48000, 3000.0), synth.noise_clip(4, 48000, 100.0)]
    pat = np.zeros(48000, dtype=np.int16)
    pat[:g["pattern_pcm"].size] = g["pattern_pcm"][:48000]
    clips.append(pat)
    pcm = np.stack(clips)
    res = eng.vad_energy(pcm, thr, want_segments=True)
    keep, seg = res["keep"].cpu().numpy(), res["seg"].cpu().numpy()
    voiced, vlen = res["voiced"].cpu().numpy(), res["voiced_len"].cpu().numpy()
    assert (res["n_vad_frames"].cpu().numpy() == 99).all()                      # Q12
    for i in range(pcm.shape[0]):
        k, s, v = vad_ref.vad_energy(pcm[i], 16000, 30, 300, thr)
        np.testing.assert_array_equal(keep[i].astype(bool), k)                     # Q13
        np.testing.assert_array_equal(seg[i], s)
        assert vlen[i] == v.size
        np.testing.assert_array_equal(voiced[i, :v.size], v)
    np.testing.assert_array_equal(keep[0].astype(bool), g["spk_0_0_keep"])         # the reference's own collector
    np.testing.assert_array_equal(keep[1].astype(bool), g["spk_1_4_keep"])
    np.testing.assert_array_equal(seg[2], g["spk_7_2_seg"])


def test_vad_edge_lengths_and_long_clip(eng, golden, clip_paths):
    g = golden["vad"]
    thr = int(g["threshold"][0])
    long = synth.speaker_clip(5, 0, 112000)
    res = eng.vad_energy(long[None], thr, want_segments=True)
    np.testing.assert_array_equal(res["keep"][0].cpu().numpy().astype(bool), g["spk_5_0_long_keep"])
    np.testing.assert_array_equal(res["seg"][0].cpu().numpy(), g["spk_5_0_long_seg"])
    for n, name in ((47999, "len_47999"), (48001, "len_48001"), (480, "len_480"), (481, "len_481"), (100, "len_100")):
        clip = synth.speaker_clip(2, 1 if n == 47999 else 2, n) if n > 1000 else synth.noise_clip(6, n)
        res = eng.vad_energy(clip[None], thr)
        nf = int(res["n_vad_frames"][0].item())
        assert nf == int(g[name + "_nframes"][0])
        np.testing.assert_array_equal(res["keep"][0].cpu().numpy()[:nf].astype(bool), g[name + "_keep"])
    # ragged batch through `lengths`
    pcm = np.zeros((2, 48000), dtype=np.int16)
    pcm[0] = synth.speaker_clip(0, 0)
    pcm[1, :30000] = synth.speaker_clip(1, 4)[:30000]
    res = eng.vad_energy(pcm, thr, lengths=np.array([48000, 30000], dtype=np.int32))
    k1, _, v1 = vad_ref.vad_energy(pcm[1, :30000], 16000, 30, 300, thr)
    assert int(res["n_vad_frames"][1].item()) == k1.size
    np.testing.assert_array_equal(res["keep"][1].cpu().numpy()[:k1.size].astype(bool), k1)
    assert int(res["voiced_len"][1].item()) == v1.size


def test_vad_dropin_collector(golden):
    from speaker_verification_amd import vad
    pcm = synth.speaker_clip(1, 4)
    frames = list(vad.frame_generator(30, pcm.tobytes(), 16000))
    assert len(frames) == 99 and len(frames[0].bytes) == 960
    segs = list(vad.vad_collector(16000, 30, 300, vad.EnergyVad(250000), frames))
    np.testing.assert_array_equal([len(s) // 2 for s in segs], golden["vad"]["spk_1_4_seglens"])
    _, _, voiced = vad_ref.vad_energy(pcm, 16000, 30, 300, 250000)
    assert b"".join(segs) == voiced.tobytes()
    assert vad.EnergyVad(250000).is_speech(frames[0].bytes, 16000) == vad_ref.energy_is_speech(
        np.frombuffer(frames[0].bytes, dtype=np.int16), 250000)


# ---- cube, model, scoring ----------------------------------------------------------------------------
def test_cube_gather(eng, golden):
    g = golden["c3d2_embed"]
    feat = np.random.default_rng(int(g["cube_feat_seed"][0])).standard_normal((297, 40))
    cube = eng.cube_gather(feat[None].astype(np.float32), g["cube_idx"][None].astype(np.int32)).cpu().numpy()
    assert cube.shape == (1, 1, 20, 80, 40)
    np.testing.assert_array_equal(cube[0], g["cube_out"])                     # float32 copy: bit-exact
    # batched, T not a multiple of anything
    feats = np.random.default_rng(1).standard_normal((3, 123, 40)).astype(np.float32)
    idx = np.random.default_rng(2).integers(0, 123 - 80, size=(3, 20)).astype(np.int32)
    cube = eng.cube_gather(feats, idx).cpu().numpy()
    for u in range(3):
        np.testing.assert_array_equal(cube[u], model_ref.feature_cube(feats[u], idx[u]))


def test_pipeline_properties_at_batch_scale(eng):
    """1 024 clips through VAD -> front end -> cube -> C3D2 (BASELINE config 3 shape): bitwise repeatable,
    a clip's embedding does not depend on its neighbours, VAD bookkeeping adds up."""
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    pcm, _ = synth.corpus_device(1024, eng.device, utts_per_speaker=8)
    pipe = VerificationPipeline(seeded_model(31, n_labels=8), use_vad=True, normalize=True, preemph_cof=0.98,
                                crop_rng="device", micro_batch=512)
    a = pipe.embed(pcm)
    b = pipe.embed(pcm)
    assert a.shape == (1024, 128) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert int(pipe.bad_clips.item()) == 0
    half = pipe.embed(pcm[:512])                                     # same micro-batch shape, other neighbours later
    assert torch.equal(half, a[:512])
    solo = pipe.embed(pcm[100:101], first_utt=100)                   # batch of one: the same bits (one clip, one embedding)
    assert torch.equal(solo[0], a[100])
    res = eng.vad_energy(pcm, c.VAD_ENERGY_THRESHOLD)
    kept = res["keep"].sum(dim=1).to(torch.int32)
    assert torch.equal(kept * res["frame_samples"], res["voiced_len"])
    assert int(res["voiced_len"].min()) > 81 * 160 + 400             # every clip keeps enough for a cube


def test_ragged_pipeline_and_vad_offsets(eng, clip_paths):
    """Clips of different lengths packed back to back (offsets / lengths form of the C-ABI): VAD masks
    equal the oracle's per clip, and embed_ragged equals embedding every clip on its own."""
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    lens = [48000, 20011, 70000, 33333, 25000, 48000, 61234]
    clips = [synth.speaker_clip(s, 1, n) for s, n in enumerate(lens)]
    # VAD through offsets
    offs, at = [], 0
    for x in clips:
        offs.append(at)
        at += (x.size + 7) // 8 * 8
    buf = np.zeros(at, dtype=np.int16)
    for o, x in zip(offs, clips):
        buf[o:o + x.size] = x
    res = eng.vad_energy(buf, c.VAD_ENERGY_THRESHOLD, lengths=np.array(lens, dtype=np.int32),
                         offsets=np.array(offs, dtype=np.int64))
    keep, vlen, voiced = res["keep"].cpu().numpy(), res["voiced_len"].cpu().numpy(), res["voiced"].cpu().numpy()
    for i, x in enumerate(clips):
        k, _, v = vad_ref.vad_energy(x, 16000, 30, 300, c.VAD_ENERGY_THRESHOLD)
        np.testing.assert_array_equal(keep[i, :k.size].astype(bool), k)
        assert vlen[i] == v.size
        np.testing.assert_array_equal(voiced[offs[i]:offs[i] + v.size], v)
    # pipeline
    pipe = VerificationPipeline(seeded_model(21, n_labels=8), use_vad=True, crop_rng="device", micro_batch=4)
    ragged = pipe.embed_ragged(clips, first_utt=1000).cpu().numpy()
    assert int(pipe.bad_clips.item()) == 0
    for k, x in enumerate(clips):
        alone = pipe.embed(x[None], first_utt=1000 + k).cpu().numpy()[0]
        np.testing.assert_array_equal(ragged[k], alone)


def test_utils_transforms(eng, golden, monkeypatch):
    """utils.FeatureCube / CMVN / ToTensor with the reference's sample-dict protocol and RNG."""
    from speaker_verification_amd import constants, utils
    g = golden["c3d2_embed"]
    feat = np.random.default_rng(int(g["cube_feat_seed"][0])).standard_normal((297, 40))
    np.random.seed(int(g["cube_np_seed"][0]))
    out = utils.FeatureCube((80, 40, 20))({"feature": feat, "label": 5})
    assert out["label"] == 5 and out["feature"].dtype == np.float32
    np.testing.assert_array_equal(out["feature"], g["cube_out"])          # the reference's own FeatureCube output
    assert utils.ToTensor()(out)[1] == 5
    same = utils.CMVN()({"feature": feat, "label": 1})                    # shipped constants: identity (Q16)
    assert same["feature"] is feat
    monkeypatch.setattr(constants, "NORMALIZE", True)
    normed = utils.CMVN()({"feature": feat, "label": 1})["feature"]
    np.testing.assert_allclose(normed, ref.cmvn(feat, True), rtol=1e-4, atol=1e-5)
    monkeypatch.setattr(constants, "DERIVATIVE", True)
    stacked = utils.CMVN()({"feature": feat, "label": 1})["feature"]
    want = ref.extract_derivative_feature(feat)
    for ch in range(3):
        np.testing.assert_allclose(stacked[:, :, ch], ref.cmvn(want[:, :, ch], True), rtol=1e-3, atol=1e-4)
    np.random.seed(3)
    cube3 = utils.FeatureCube3C((80, 40, 20, 3))({"feature": want, "label": 2})["feature"]
    np.random.seed(3)
    idx = np.random.randint(297 - 80, size=20)
    assert cube3.shape == (3, 20, 80, 40)
    for u in (0, 7, 19):
        np.testing.assert_array_equal(cube3[:, u], want.transpose(2, 0, 1)[:, idx[u]:idx[u] + 80].astype(np.float32))


def test_general_fft_lengths(sp):
    """fft lengths / filter counts outside the fused kernel go through the stage kernels
    (framing -> svk_spectrum -> svk_mel_features) and still match the reference: nfft 256 and 2048 run the
    Stockham kernel (spectrum_pow2_kernel), nfft 400 the direct DFT (spectrum_dft_kernel)."""
    sig8k = synth.noise_clip(21, 8000)
    np.testing.assert_allclose(sp.feature.mfcc(sig8k, 8000, fft_length=256),
                               ref.mfcc(sig8k, 8000, fft_length=256), **FEAT_TOL)
    sig = synth.speaker_clip(4, 0, 9000)
    np.testing.assert_allclose(sp.feature.lmfe(sig, 16000, fft_length=2048, num_filters=80),
                               ref.lmfe(sig, 16000, fft_length=2048, num_filters=80), **FEAT_TOL)
    f, e = sp.feature.mfe(sig, 16000, frame_length=0.025, fft_length=400)         # not a power of two
    fr, er = ref.mfe(sig, 16000, frame_length=0.025, fft_length=400)
    np.testing.assert_allclose(f, fr, rtol=1e-4)
    np.testing.assert_allclose(e, er, rtol=1e-4)
    np.testing.assert_allclose(sp.feature.mfcc(sig, 16000, fft_length=256, dc_elimination=False, num_cepstral=20),
                               ref.mfcc(sig, 16000, fft_length=256, dc_elimination=False, num_cepstral=20), **FEAT_TOL)


def test_audio_dataset(tmp_path):
    """load_data.AudioDataset: WAV files -> lmfe(25 ms / 10 ms / 40 / 1024) -> transforms, like load_data.py:50-87."""
    from speaker_verification_amd import load_data, utils, vad

    class Compose:                                   # torchvision.transforms.Compose is absent here
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    names = ["id10001/a.wav", "id10002/b.wav", "id10001/missing.wav"]
    clips = {names[0]: synth.speaker_clip(1, 0, 20000), names[1]: synth.speaker_clip(2, 0, 32000)}
    for rel, pcm in clips.items():
        os.makedirs(os.path.dirname(tmp_path / rel), exist_ok=True)
        vad.write_wave(str(tmp_path / rel), pcm.tobytes(), 16000)
    listing = tmp_path / "ids.txt"
    listing.write_text("\n".join(names) + "\n")
    ds = load_data.AudioDataset(str(listing), str(tmp_path), {"id10001": 0, "id10002": 1})
    assert len(ds) == 2                                                       # the missing file is skipped
    feat, label = ds[1]
    want = ref.lmfe((clips[names[1]] / 32768.0).astype(np.float32), 16000, 0.025, 0.01, 40, 1024)
    assert label == 1
    np.testing.assert_allclose(feat, want, **FEAT_TOL)
    np.random.seed(5)
    ds2 = load_data.AudioDataset(str(listing), str(tmp_path), {"id10001": 0, "id10002": 1},
                                 transform=Compose([utils.CMVN(), utils.FeatureCube((80, 40, 20)), utils.ToTensor()]))
    cube, label = ds2[0]
    assert cube.shape == (1, 20, 80, 40) and cube.dtype == np.float32 and label == 0
    sig, sr = vad.read_wave(str(tmp_path / names[0]))
    assert sr == 16000 and sig == clips[names[0]].tobytes()
    vad.write_wave(str(tmp_path / "silence8k.wav"), b"\0" * 4000, 8000)
    up = load_data.load_wav(str(tmp_path / "silence8k.wav"))           # 8 kHz file: resampled to 16 kHz on the device
    assert up.shape == (4000,) and up.dtype == np.float32 and not up.any()


def test_ingest_resample_parity(eng):
    """svk_ingest_resample against the CPU restatement of scipy.signal.resample_poly: mono 48 kHz,
    stereo 44.1 kHz, up-sampling from 8 kHz, ragged lengths; float32 and int16 outputs."""
    from oracle import ingest_ref
    from speaker_verification_amd import ingest
    rng = np.random.default_rng(11)
    for fs_in, n_ch, lens in [(48000, 1, [48000, 30011, 3, 1]), (44100, 2, [44100, 12345, 441]),
                              (8000, 1, [8000, 4001]), (32000, 3, [9999])]:
        n = max(lens)
        shape = (len(lens), n) if n_ch == 1 else (len(lens), n, n_ch)
        pcm = (rng.standard_normal(shape) * 6000).clip(-32768, 32767).astype(np.int16)
        up, down = ingest.rational_ratio(fs_in, 16000)
        out, out_len = ingest.resample_batch(pcm, fs_in, 16000, lengths=np.array(lens, dtype=np.int32))
        o16, _ = ingest.resample_batch(pcm, fs_in, 16000, lengths=np.array(lens, dtype=np.int32), out_dtype="i16")
        out, out_len, o16 = out.cpu().numpy(), out_len.cpu().numpy(), o16.cpu().numpy()
        for i, L in enumerate(lens):
            want = ingest_ref.resample_poly(ingest_ref.to_mono(pcm[i, :L]), up, down)
            assert out_len[i] == len(want) == -(-L * up // down)
            np.testing.assert_allclose(out[i, :len(want)], want, rtol=0, atol=2e-6)      # f32 sums of <= 61 terms in [-1, 1)
            assert not out[i, len(want):].any() and not o16[i, len(want):].any()
            d = o16[i, :len(want)].astype(np.int32) - ingest_ref.to_int16(want).astype(np.int32)
            assert np.abs(d).max() <= 1 and np.mean(d != 0) < 0.01                        # ties at .5 LSB only
    # size-independent properties at a full 3 s batch: unit DC gain away from the edges, linearity
    const = np.full((64, 48000), 12000, dtype=np.int16)
    y, _ = ingest.resample_batch(const, 48000, 16000)
    np.testing.assert_allclose(y[:, 40:-40].cpu().numpy(), 12000 / 32768.0, rtol=0, atol=2e-6)
    a = (rng.standard_normal((8, 44100)) * 3000).astype(np.int16)
    ya, _ = ingest.resample_batch(a, 44100, 16000)
    y2, _ = ingest.resample_batch((2 * a).astype(np.int16), 44100, 16000)
    np.testing.assert_allclose(y2.cpu().numpy(), 2 * ya.cpu().numpy(), rtol=0, atol=4e-6)


def test_pipeline_ingest_feeds_the_int16_path(eng):
    """48 kHz stereo recordings -> pipeline.ingest -> embed: same embeddings as feeding the oracle's
    16 kHz int16 rendering of the same audio (up to the <= 1 LSB rounding ties of the resampler)."""
    from oracle import ingest_ref
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    mono16 = np.stack([synth.speaker_clip(s, 0) for s in range(4)])
    stereo48 = np.repeat(np.repeat(mono16, 3, axis=1)[:, :, None], 2, axis=2)       # crude 48 kHz stereo source
    model = seeded_model(0, n_labels=8).to(eng.device).eval()
    pipe = VerificationPipeline(model, use_vad=False, crop_rng="device", crop_seed=5)
    pcm16, lens = pipe.ingest(stereo48, 48000)
    assert pcm16.dtype == torch.int16 and pcm16.shape == (4, 48000) and bool((lens == 48000).all())
    want = np.stack([ingest_ref.to_int16(ingest_ref.resample_poly(ingest_ref.to_mono(stereo48[i]), 1, 3))
                     for i in range(4)])
    d = pcm16.cpu().numpy().astype(np.int32) - want.astype(np.int32)
    assert np.abs(d).max() <= 1 and np.mean(d != 0) < 0.01
    emb_a = pipe.embed(pcm16)
    emb_b = pipe.embed(want)
    assert emb_a.shape == (4, 128) and bool(torch.isfinite(emb_a).all())
    np.testing.assert_allclose(emb_a.cpu().numpy(), emb_b.cpu().numpy(), rtol=1e-3, atol=1e-3)


def test_overlapped_front_end_gives_the_same_embeddings(eng):
    """pipeline(overlap_front=True): cube building on a side stream, network on the main one -- same
    kernels, same inputs, same results as the serial schedule."""
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    pcm, _ = synth.corpus_device(96, eng.device)
    model = seeded_model(2, n_labels=8).to(eng.device).eval()
    serial = VerificationPipeline(model, crop_rng="device", crop_seed=7, micro_batch=24, preemph_cof=0.98)
    both = VerificationPipeline(model, crop_rng="device", crop_seed=7, micro_batch=24, preemph_cof=0.98,
                                overlap_front=True)
    want = serial.embed(pcm)
    for _ in range(3):                                  # repeated: a missing cross-stream dependency shows as a diff
        got = both.embed(pcm)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def test_overlapped_front_end_behind_a_busy_main_stream(eng):
    """The same with the main stream busy when the call starts: every launch of the call is then queued before the first one
    runs, and the side stream gets as far ahead as its dependencies let it.  It may run one micro-batch ahead of the network
    and no further (while nothing held it back, the last micro-batch missed the one-stream bits in most such calls)."""
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    pcm, _ = synth.corpus_device(96, eng.device)
    model = seeded_model(2, n_labels=8).to(eng.device).eval()
    kw = dict(crop_rng="device", crop_seed=7, micro_batch=24, preemph_cof=0.98)
    want = VerificationPipeline(model, **kw).embed(pcm)
    both = VerificationPipeline(model, overlap_front=True, **kw)
    busy = torch.randn((4096, 4096), device=eng.device)
    for _ in range(6):
        for _ in range(4):
            busy = (busy @ busy).clamp_(-1, 1)
        got = both.embed(pcm)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def test_load_wav_resamples_on_device(tmp_path):
    """load_data.load_wav (utils.py:170-173 drop-in) on a stereo 44.1 kHz file and on a mono 16 kHz one."""
    import wave
    from oracle import ingest_ref
    from speaker_verification_amd import load_data
    rng = np.random.default_rng(3)
    frames = (rng.standard_normal((22050, 2)) * 5000).astype(np.int16)
    for path, rate, data in [(str(tmp_path / "a.wav"), 44100, frames), (str(tmp_path / "b.wav"), 16000, frames[:, :1])]:
        with wave.open(path, "wb") as wf:
            wf.setnchannels(data.shape[1])
            wf.setsampwidth(2)
            wf.setframerate(rate)
            wf.writeframes(np.ascontiguousarray(data).tobytes())
    got = load_data.load_wav(str(tmp_path / "a.wav"))
    want = ingest_ref.resample_poly(ingest_ref.to_mono(frames), 160, 441)
    assert got.dtype == np.float32 and got.shape == want.shape == (8000,)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    same = load_data.load_wav(str(tmp_path / "b.wav"))
    assert np.array_equal(same, frames[:, 0].astype(np.float32) / np.float32(32768.0))


def test_error_paths(eng):
    """Unsupported configurations fail loudly with the library's message; nothing falls back."""
    from speaker_verification_amd import _lib
    from speaker_verification_amd._lib import SvkError
    from speaker_verification_amd.engine import spec_from_seconds
    from speaker_verification_amd.speechpy import feature, processing
    sig = synth.noise_clip(1, 4000)
    with pytest.raises(SvkError, match="fft_length 512 or 1024"):                # the fused kernel itself refuses ...
        eng.plan(spec_from_seconds(16000, 0.02, 0.01, 256, 40, 13, _lib.OUT_MFCC))
    with pytest.raises(SvkError, match="filters"):
        eng.plan(spec_from_seconds(16000, 0.02, 0.01, 512, 80, 13, _lib.OUT_MFCC))
    # ... and the entry points route such configurations to the staged kernels instead (feature.py:77-99 computes)
    f, nf, _ = feature.features_batch(np.stack([sig, sig[::-1]]), 16000, fft_length=256)
    assert f.shape == (2, 23, 13) and nf.tolist() == [23, 23]
    np.testing.assert_allclose(f[1].cpu().numpy(), ref.mfcc(sig[::-1], 16000, fft_length=256), **FEAT_TOL)
    with pytest.raises(AssertionError):
        feature.mfcc(sig, 16000, high_frequency=9000)                     # feature.py:58
    with pytest.raises(AssertionError):
        processing.stack_frames(np.zeros((4, 4)), 16000)                  # processing.py:90
    with pytest.raises(SvkError, match="VAD frames"):
        eng.vad_energy(np.zeros((1, 480 * 9000), dtype=np.int16), 1000)
    with pytest.raises(TypeError):
        eng.vad_energy(np.zeros((1, 4800), dtype=np.float32), 1000)


def test_staged_fall_through_does_not_pin_its_inputs(eng):
    """`Engine.plan` used to cache the SvkError of a configuration the fused kernel refuses and re-raise the
    SAME object on every call; each raise chained a traceback whose frames held the caller's PCM.  Now a fresh exception
    per call: after N calls on the staged path no input survives."""
    import gc
    import weakref
    from speaker_verification_amd import _lib
    from speaker_verification_amd.engine import spec_from_seconds
    spec = spec_from_seconds(16000, 0.025, 0.01, 400, 40, 13, _lib.OUT_MFCC)      # nfft 400: not a fused configuration
    with pytest.raises(_lib.SvkError) as first:
        eng.plan(spec)
    with pytest.raises(_lib.SvkError) as second:
        eng.plan(spec)
    assert first.value is not second.value and first.value.code == _lib.SVK_ERR_UNSUPPORTED == second.value.code
    assert str(first.value) == str(second.value)
    del first, second
    refs = []
    for k in range(5):
        pcm = torch.from_numpy(synth.noise_clip(k, 8000)).to(eng.device)
        refs.append(weakref.ref(pcm))
        feat, nf, _ = eng.features(pcm, spec)
        assert feat.shape == (1, int(nf[0]), 13)
        del pcm, feat, nf
    gc.collect()
    assert [r() is None for r in refs] == [True] * 5


def test_concatenated_ragged_offsets(eng):
    """The `d_offsets` form of the C-ABI: clips of different lengths back to back in one buffer."""
    from speaker_verification_amd import _lib
    from speaker_verification_amd.engine import spec_from_seconds
    lens = np.array([16000, 5000, 48000, 801], dtype=np.int32)
    pad = [(-n) % 8 for n in lens]                                        # keep 16-byte alignment of each clip
    offs, chunks, pos = [], [], 0
    for i, n in enumerate(lens):
        offs.append(pos)
        chunks.append(synth.noise_clip(50 + i, int(n)))
        chunks.append(np.zeros(pad[i], dtype=np.int16))
        pos += int(n) + pad[i]
    buf = np.concatenate(chunks)
    spec = spec_from_seconds(16000, 0.020, 0.01, 512, 40, 13, _lib.OUT_MFCC)
    feat, nf, _ = eng.features(buf, spec, lengths=lens, offsets=np.array(offs, dtype=np.int64))
    feat, nf = feat.cpu().numpy(), nf.cpu().numpy()
    # one clip deliberately left unaligned exercises the scalar staging path
    buf2 = np.concatenate([np.zeros(3, dtype=np.int16), chunks[0]])
    f2, _, _ = eng.features(buf2, spec, lengths=lens[:1], offsets=np.array([3], dtype=np.int64))
    for i, n in enumerate(lens):
        want = ref.mfcc(buf[offs[i]:offs[i] + n], 16000)
        assert nf[i] == want.shape[0]
        np.testing.assert_allclose(feat[i, :nf[i]], want, **FEAT_TOL)
    np.testing.assert_allclose(f2[0].cpu().numpy(), ref.mfcc(chunks[0], 16000), **FEAT_TOL)


def test_cosine_scores(eng, golden):
    g = golden["scoring"]
    got = eng.cosine_scores(g["test"], g["enroll"]).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (42, 6)
    np.testing.assert_allclose(got, g["sims"], rtol=0, atol=1e-5)             # the reference's own scores
    rng = np.random.default_rng(8)
    for nt, ns, d in ((4874, 40, 128), (33, 17, 128), (5, 3, 100), (16, 16, 64), (1, 1, 7)):
        t = rng.standard_normal((nt, d)).astype(np.float32)
        e = rng.standard_normal((ns, d)).astype(np.float32)
        t[0] = 0                                                              # zero row: sklearn gives 0, not NaN
        got = eng.cosine_scores(t, e).cpu().numpy()
        np.testing.assert_allclose(got, scoring_ref.cosine_matrix(t, e), rtol=0, atol=1e-5)
        assert not got[0].any()


def test_cosine_scores_tiled_kernel(eng):
    """Problems with >= 2^22 pairs take the LDS-tiled kernel (dim <= 128: fragments hoisted; larger: streamed)."""
    rng = np.random.default_rng(9)
    for nt, ns, d in ((4100, 1030, 128), (2050, 2100, 200), (8200, 520, 100), (3000, 1500, 7)):
        t = rng.standard_normal((nt, d)).astype(np.float32)
        e = rng.standard_normal((ns, d)).astype(np.float32)
        t[5] = 0
        e[3] = 0
        got = eng.cosine_scores(t, e).cpu().numpy()
        want = scoring_ref.cosine_matrix(t, e)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
        assert not got[5].any() and not got[:, 3].any()
    # more 128-row blocks than resident workgroups: every workgroup takes an equal range of (row block,
    # enrolled block) units (scoring.hip), so row blocks are shared between workgroups; rows early, in the
    # middle, around block 1024 and in the ragged last block
    nt, ns, d = 128 * 1100 + 37, 203, 128
    t = rng.standard_normal((nt, d)).astype(np.float32)
    e = rng.standard_normal((ns, d)).astype(np.float32)
    got = eng.cosine_scores(t, e)
    rows = np.r_[0:130, 128 * 700:128 * 700 + 130, 128 * 1024 - 2:128 * 1024 + 130, nt - 140:nt]
    want = scoring_ref.cosine_matrix(t[rows], e)
    np.testing.assert_allclose(got[torch.from_numpy(rows).to(got.device)].cpu().numpy(), want, rtol=0, atol=1e-5)
    # every row is a unit-vector product: |score| <= 1 and the self-product of a copied row is 1
    assert float(got.abs().max()) <= 1.0 + 1e-5
    e2 = e.copy()
    e2[7] = t[128 * 1050 + 5]
    assert abs(float(eng.cosine_scores(t, e2)[128 * 1050 + 5, 7]) - 1.0) <= 1e-5


def test_evaluation_dropin(eng, golden):
    from speaker_verification_amd import evaluation
    g = golden["scoring"]

    class Fixed(torch.nn.Module):
        def forward(self, utterance, development=False):
            return utterance

    ev = evaluation.Evaluation(Fixed(), {f"id{j:05d}": g["enroll"][j:j + 1] for j in range(6)})
    for i in (0, 5, 41):
        sims, assigned = ev.compute_Similarity(torch.from_numpy(g["test"][i:i + 1]))
        assert sims.dtype == np.float64
        np.testing.assert_allclose(sims, g["sims"][i], rtol=0, atol=1e-5)
        np.testing.assert_array_equal(assigned, g["assigned"][i])
    scores = evaluation.score_matrix(g["test"], g["enroll"]).cpu().numpy().astype(np.float64)
    eer, auc, _, _ = evaluation.get_eer_auc(g["labels"].flatten(), scores.flatten())
    assert eer == pytest.approx(float(g["eer"][0]), abs=1e-9)                 # EER equal to the reference's
    assert auc == pytest.approx(float(g["auc"][0]), abs=1e-9)
    eer2, auc2, _, _ = evaluation.get_eer_auc(g["big_labels"], g["big_scores"])
    assert eer2 == float(g["big_eer"][0]) and auc2 == float(g["big_auc"][0])


def test_enrolment_store_roundtrip(eng, tmp_path):
    """model.create_speaker_models -> {id}.pt files -> evaluation.Evaluation, like the reference's
    enrol-then-evaluate flow (model.py:351-388, evaluation.py:55-65)."""
    from speaker_verification_amd import evaluation
    from speaker_verification_amd.model import create_speaker_models, seeded_model
    model = seeded_model(5, n_labels=8).to(eng.device)
    cubes = np.random.default_rng(6).standard_normal((6, 1, 20, 80, 40)).astype(np.float32)
    ids = ["id10001", "id10002", "id10001", "id10003", "id10002", "id10001"]
    store = create_speaker_models(model, cubes, ids, save_dir=str(tmp_path))
    assert sorted(store) == ["id10001", "id10002", "id10003"]
    with torch.no_grad():
        emb = model(torch.from_numpy(cubes).to(eng.device), development=False).cpu()
    assert torch.equal(store["id10001"], emb[5:6]) and torch.equal(store["id10002"], emb[4:5])   # last one wins (Q17)
    ev = evaluation.Evaluation(model, str(tmp_path))
    assert list(ev.speaker_models) == ["id10001", "id10002", "id10003"]
    sims, assigned = ev.compute_Similarity(torch.from_numpy(cubes[3:4]))
    assert np.argmax(sims) == 2 and sims[2] == pytest.approx(1.0, abs=1e-5) and assigned[2] == 1
    out = evaluation.evaluate(model, cubes, ids, str(tmp_path), plot_path=None)
    assert out["scores"].shape == (6, 3) and 0.0 <= out["eer"] <= 1.0 and out["accuracy"] >= 50.0


def test_device_roc_eer(eng, golden):
    from speaker_verification_amd import evaluation
    g = golden["scoring"]
    eer, auc = evaluation.get_eer_auc_device(g["labels"], g["sims"])
    assert eer == pytest.approx(float(g["eer"][0]), abs=1e-9) and auc == pytest.approx(float(g["auc"][0]), abs=1e-9)
    eer, auc = evaluation.get_eer_auc_device(g["big_labels"], g["big_scores"].astype(np.float32))
    want = scoring_ref.get_eer_auc(g["big_labels"], g["big_scores"].astype(np.float32))
    assert eer == pytest.approx(want[0], abs=1e-9) and auc == pytest.approx(want[1], abs=1e-9)
    rng = np.random.default_rng(10)
    # heavy ties (quantised scores), unbalanced classes, 2e6 pairs
    lab = (rng.random(2_000_000) < 0.03).astype(np.uint8)
    sc = np.round(rng.standard_normal(2_000_000) + 0.8 * lab, 2).astype(np.float32)
    eer, auc = evaluation.get_eer_auc_device(lab, sc)
    want = scoring_ref.get_eer_auc(lab, sc)
    assert eer == pytest.approx(want[0], abs=1e-9) and auc == pytest.approx(want[1], abs=1e-9)
    with pytest.raises(Exception):
        evaluation.get_eer_auc_device(np.ones(10, dtype=np.uint8), np.arange(10, dtype=np.float32))


def test_siamese(eng, golden):
    from speaker_verification_amd.siamese import Siamese
    g = golden["scoring"]
    sia = Siamese(LAMBDA=0.001, M=2.0)
    o1, o2 = torch.from_numpy(g["l2_o1"]).to(eng.device), torch.from_numpy(g["l2_o2"]).to(eng.device)
    np.testing.assert_allclose(sia.l2_dist(o1, o2).cpu().numpy(), g["l2_dist"], rtol=1e-6)
    lin = torch.nn.Linear(4, 3).to(eng.device)
    y = torch.tensor([1, 0, 1, 0, 1, 0, 1, 0, 1], dtype=torch.float32, device=eng.device)
    loss = sia(lin, y, o1.requires_grad_(), o2)
    norms = [float(torch.norm(p.detach())) for p in lin.parameters()]
    want = scoring_ref.contrastive_loss(y.cpu().numpy(), g["l2_o1"], g["l2_o2"], norms, 0.001, 2.0)
    assert float(loss.detach()) == pytest.approx(want, rel=1e-5)
    loss.backward()
    assert o1.grad is not None and torch.isfinite(o1.grad).all()


def test_siamese_forward_against_reference_loss(eng, golden):
    """`Siamese.forward` on ROCm against the REFERENCE's own forward (siamese.py:10-27, run on the CPU by
    tools/make_golden.py with `.cuda()` made the identity): the reference's C3D2 under seed 77 supplies the parameter
    norms, twelve embedding pairs, four (LAMBDA, M) pairs -- rel 1e-5.  Both the autograd path (loss.backward) and the
    inference path (`svk_l2_dist` under no_grad) are held to the same numbers."""
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.siamese import Siamese
    g = golden["scoring"]
    seed, n_labels, n_ch = (int(v) for v in g["sf_model_seed"])
    net = seeded_model(seed, n_labels=n_labels, num_channels=n_ch).to(eng.device)
    norms = np.array([float(torch.norm(p.detach())) for p in net.parameters()])
    np.testing.assert_allclose(norms, g["sf_param_norms"], rtol=5e-6, atol=1e-12)   # same init as the reference's C3D2 (f32 norms: summation order)
    y = torch.from_numpy(g["sf_y"]).to(eng.device)
    o1, o2 = torch.from_numpy(g["sf_o1"]).to(eng.device), torch.from_numpy(g["sf_o2"]).to(eng.device)
    for k, (lam, m) in enumerate(g["sf_cases"]):
        sia = Siamese(LAMBDA=float(lam), M=float(m))
        with torch.no_grad():
            assert float(sia(net, y, o1, o2)) == pytest.approx(float(g["sf_loss"][k]), rel=1e-5)   # svk_l2_dist inside
        a = o1.clone().requires_grad_()
        loss = sia(net, y, a, o2)
        assert float(loss.detach()) == pytest.approx(float(g["sf_loss"][k]), rel=1e-5)
        loss.backward()
        assert torch.isfinite(a.grad).all()
    d = Siamese(0.0, 1.0).l2_dist(o1, o2).cpu().numpy()
    np.testing.assert_allclose(d, g["sf_dist"], rtol=1e-6)
    assert float(d[g["sf_y"] == 1].mean()) == pytest.approx(float(g["sf_same_mean"][0]), rel=1e-6)
    assert float(d[g["sf_y"] == 0].mean()) == pytest.approx(float(g["sf_notsame_mean"][0]), rel=1e-6)


# ---- whole path -------------------------------------------------------------------------------------------
def test_pipeline_end_to_end_and_eer(eng):
    from speaker_verification_amd import evaluation
    from speaker_verification_amd.model import calibrate_batchnorm, perturb_inference_state, seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline, enroll_last_utterance
    n_spk, per = 6, 4
    pcm, spk = synth.corpus(n_spk, per)
    model = seeded_model(11, n_labels=32)
    model.load_state_dict(perturb_inference_state(model.state_dict(), 12))
    pipe = VerificationPipeline(model, use_vad=True, micro_batch=16)
    _, inter = pipe.embed(pcm, return_intermediates=True)
    crops = np.concatenate([d["crop_idx"] for d in inter])
    # crop draws follow the reference's RNG protocol (utils.py:15,372)
    rs = np.random.RandomState(12345)
    nfr = np.concatenate([d["n_frames"].cpu().numpy() for d in inter])
    want_crops = np.stack([rs.randint(int(T) - 80, size=20) for T in nfr])
    np.testing.assert_array_equal(crops, want_crops)
    # BatchNorm statistics calibrated on the data (a well-conditioned embedding, see
    # model.calibrate_batchnorm), then the same crops again through the final weights
    calibrate_batchnorm(pipe.model, torch.cat([d["cube"] for d in inter]))
    pipe.refresh_model()
    emb = pipe.embed(pcm, crop_idx=crops).cpu().numpy()

    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_emb = []
    for i in range(pcm.shape[0]):
        _, _, voiced = vad_ref.vad_energy(pcm[i], 16000, c.VAD_FRAME_MS, c.VAD_PADDING_MS, c.VAD_ENERGY_THRESHOLD)
        # the pipeline reads int16 PCM the way librosa hands it to the reference's lmfe call: / 32768
        feat = ref.lmfe(voiced / 32768.0, 16000, c.FRAME_LEN, c.FRAME_STEP, c.NUM_COEF, c.NUM_FFT)
        assert feat.shape[0] == nfr[i]
        ref_emb.append(model_ref.c3d2_embed(state, model_ref.feature_cube(feat, crops[i])[None]).numpy()[0])
    ref_emb = np.stack(ref_emb)
    scale = np.abs(ref_emb).max()
    # (the bench's parity leg observes 7.6e-6 of the scale on 2 048 clips; 5e-5 leaves room for other weights, no more)
    print("end to end: embedding max |diff| / scale %.2e" % (np.abs(emb - ref_emb).max() / scale))
    np.testing.assert_allclose(emb, ref_emb, rtol=0, atol=5e-5 * scale)

    ids, last = enroll_last_utterance(emb, spk)                                # Q17
    scores = pipe.score(emb, emb[last]).cpu().numpy()
    ref_scores = scoring_ref.cosine_matrix(ref_emb, ref_emb[last])
    np.testing.assert_allclose(scores, scoring_ref.cosine_matrix(emb, emb[last]), rtol=0, atol=1e-5)
    print("end to end: cosine max |diff| %.2e" % np.abs(scores - ref_scores).max())
    np.testing.assert_allclose(scores, ref_scores, rtol=0, atol=2e-5)
    assert scores.std() > 0.05                                                  # well-conditioned scores
    labels = (spk[:, None] == ids[None, :]).astype(np.float64)
    eer_gpu, auc_gpu, _, _ = evaluation.get_eer_auc(labels.flatten(), scores.astype(np.float64).flatten())
    eer_ref, auc_ref, _, _ = scoring_ref.get_eer_auc(labels.flatten(), ref_scores.astype(np.float64).flatten())
    assert eer_gpu == pytest.approx(eer_ref, abs=1e-4)                          # EER parity
    assert auc_gpu == pytest.approx(auc_ref, abs=1e-4)
    # host-fed path (pinned double buffer + copy stream) == resident path, bit for bit -- also when called
    # twice back to back with no synchronisation in between (the buffers are reused across calls)
    pipe_dev = VerificationPipeline(pipe.model, use_vad=True, micro_batch=7, crop_rng="device")
    a = pipe_dev.embed(pcm)
    b = pipe_dev.embed_host(pcm)
    b2 = pipe_dev.embed_host(pcm[::-1].copy())
    b3 = pipe_dev.embed_host(pcm)
    assert torch.equal(a, b) and torch.equal(a, b3)
    assert torch.equal(b2, pipe_dev.embed(pcm[::-1].copy()))
    # device-side crop draw: in range, reproducible, keyed by the global clip index
    nf_dev = eng.to_device(nfr.astype(np.int32))
    d1 = eng.draw_crops(nf_dev, 20, 80, seed=7, first_utt=100).cpu().numpy()
    d2 = eng.draw_crops(nf_dev[4:], 20, 80, seed=7, first_utt=104).cpu().numpy()
    assert (d1 >= 0).all() and (d1 < (nfr - 80)[:, None]).all() and len(np.unique(d1)) > 50
    np.testing.assert_array_equal(d1[4:], d2)
    bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
    short = eng.draw_crops(eng.to_device(np.array([80, 300, 10], dtype=np.int32)), 20, 80, 7, 0, bad).cpu().numpy()
    assert (short[0] == -1).all() and (short[2] == -1).all() and (short[1] >= 0).all() and int(bad.item()) == 2
    z = eng.cube_gather(eng.to_device(np.ones((3, 300, 40), dtype=np.float32)), short).cpu().numpy()
    assert not z[0].any() and not z[2].any() and (z[1] == 1).all()


# ---- round 2 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [8000, 32000, 44100])
def test_nfft1024_other_sampling_rates(sp, eng, golden, fs):
    """fft_length 1024 away from 16 kHz: SpeechPy's bank then ends on bin 256 = nfft/4 (feature.py:77-99),
    one bin past what the fused kernel kept in round 1 (it raised).  Against the reference's own outputs,
    through the fused kernel (5th untangling step) and, forced, through the staged kernels."""
    from speaker_verification_amd import _lib
    from speaker_verification_amd.engine import spec_from_seconds
    g = golden["round2"]
    sig = synth.speaker_clip(9, fs // 1000, fs // 2, fs)
    np.testing.assert_allclose(sp.feature.lmfe(sig, fs, 0.025, 0.01, 40, 1024), g[f"lmfe_1024_fs{fs}"], **FEAT_TOL)
    np.testing.assert_allclose(sp.feature.mfcc(sig, fs, fft_length=1024), g[f"mfcc_1024_fs{fs}"], **FEAT_TOL)
    f, e = sp.feature.mfe((sig / 32768.0).astype(np.float32), fs, fft_length=1024, num_filters=26)
    np.testing.assert_allclose(f, g[f"mfe_1024_fs{fs}_feat"], rtol=2e-4, atol=1e-12)
    np.testing.assert_allclose(e, g[f"mfe_1024_fs{fs}_energy"], rtol=2e-4, atol=1e-12)
    spec = spec_from_seconds(fs, 0.025, 0.01, 1024, 40, 40, _lib.OUT_LMFE)
    eng.plan(spec)                                                      # the fused kernel takes it (no SvkError)
    staged, nf, _ = eng._features_staged(sig[None], spec, None, None, None, None, False)
    np.testing.assert_allclose(staged[0, :int(nf[0])].cpu().numpy(), g[f"lmfe_1024_fs{fs}"], **FEAT_TOL)
    # batched + ragged + fused pre-emphasis at that rate
    clips = np.stack([sig, synth.speaker_clip(3, 2, fs // 2, fs)])
    lens = np.array([sig.size, sig.size - 777], dtype=np.int32)
    feat, nfr, _ = sp.feature.features_batch(clips, fs, "lmfe", 0.025, 0.01, num_filters=40, fft_length=1024,
                                             preemphasis_cof=0.97, lengths=lens)
    for i in range(2):
        want = ref.lmfe(ref.preemphasis(clips[i, :lens[i]], cof=0.97), fs, 0.025, 0.01, 40, 1024)
        assert int(nfr[i]) == want.shape[0]
        np.testing.assert_allclose(feat[i, :want.shape[0]].cpu().numpy(), want, **FEAT_TOL)


def test_pipeline_reads_int16_like_librosa(eng):
    """the reference's model path feeds lmfe the float signal librosa returns (int16 / 32768,
    utils.py:170-173, load_data.py:50-70) with NORMALIZE = False; the pipeline's int16 front end must give
    THOSE log-mel values (2 ln 32768 below raw-int16 ones), with and without the fused pre-emphasis."""
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.pipeline import VerificationPipeline
    pcm, _ = synth.corpus(2, 2)
    for cof in (0.97, None):
        pipe = VerificationPipeline(seeded_model(3, n_labels=4), use_vad=False, normalize=False, preemph_cof=cof)
        feat, nf = pipe.features(eng.to_device(pcm))
        for i in range(pcm.shape[0]):
            sig = pcm[i] / 32768.0
            sig = ref.preemphasis(sig, cof=cof) if cof is not None else sig
            want = ref.lmfe(sig, 16000, c.FRAME_LEN, c.FRAME_STEP, c.NUM_COEF, c.NUM_FFT)
            np.testing.assert_allclose(feat[i, :int(nf[i])].cpu().numpy(), want, **FEAT_TOL)
    raw = VerificationPipeline(seeded_model(3, n_labels=4), use_vad=False, normalize=False, pcm_scale=1.0)
    feat_raw, _ = raw.features(eng.to_device(pcm))
    np.testing.assert_allclose((feat_raw - feat).cpu().numpy()[:, :200], 2 * np.log(32768.0), atol=1e-4)
    # MFCC with c0 := log(frame energy): the energy path carries the scale too
    from speaker_verification_amd import _lib
    from speaker_verification_amd.engine import spec_from_seconds
    spec = spec_from_seconds(16000, 0.020, 0.01, 512, 40, 13, _lib.OUT_MFCC, input_scale=1.0 / 32768.0)
    m, _, en = eng.features(pcm[:1], spec, want_energy=True)
    np.testing.assert_allclose(m[0].cpu().numpy(), ref.mfcc(pcm[0] / 32768.0, 16000), **FEAT_TOL)
    np.testing.assert_allclose(en[0].cpu().numpy(), ref.mfe(pcm[0] / 32768.0, 16000)[1], rtol=1e-4)


def test_vad_rings_longer_than_64_frames(eng, golden, clip_paths):
    """10 ms frames with 1 s of padding = a ring of 100 frames (vad.py:81): keep / segment masks equal the
    reference's own collector (golden) and the packed samples equal the oracle's, bit for bit."""
    from speaker_verification_amd import vad
    g = golden["round2"]
    thr = int(g["vad_threshold"][0])
    clips = {"spk_0_0": synth.speaker_clip(0, 0), "spk_5_0_long": synth.speaker_clip(5, 0, 112000),
             "noise_loud": synth.noise_clip(3, 48000, 3000.0), "spk_3_1": synth.speaker_clip(3, 1, 80000),
             "pattern10": g["vad_pattern10_pcm"]}
    for name, pcm in clips.items():
        for frame_ms, pad_ms in ((10, 1000), (10, 700), (20, 1500)):
            res = eng.vad_energy(pcm[None], thr, frame_ms=frame_ms, padding_ms=pad_ms, want_segments=True)
            want_keep, want_seg = g[f"vad_{name}_{frame_ms}_{pad_ms}_keep"], g[f"vad_{name}_{frame_ms}_{pad_ms}_seg"]
            n = want_keep.size
            assert int(res["n_vad_frames"][0]) == n
            np.testing.assert_array_equal(res["keep"][0, :n].cpu().numpy().astype(bool), want_keep)
            np.testing.assert_array_equal(res["seg"][0, :n].cpu().numpy(), want_seg)
            _, _, voiced = vad_ref.vad_energy(pcm, 16000, frame_ms, pad_ms, thr)
            assert int(res["voiced_len"][0]) == voiced.size
            np.testing.assert_array_equal(res["voiced"][0, :voiced.size].cpu().numpy(), voiced)
    # the drop-in collector with those durations, and the all-frames-at-once decision call
    pcm = clips["pattern10"]
    frames = list(vad.frame_generator(10, pcm.tobytes(), 16000))
    ev = vad.EnergyVad(thr)
    flags = ev.speech_flags(frames, 16000)
    np.testing.assert_array_equal(flags, vad_ref.frame_flags(pcm, 10, 16000, thr))
    assert ev.is_speech(frames[40].bytes, 16000) == bool(flags[40]) and ev.is_speech(frames[5].bytes, 16000) == bool(flags[5])
    segs = list(vad.vad_collector(16000, 10, 1000, ev, frames))
    keep = g["vad_pattern10_10_1000_keep"]
    assert b"".join(segs) == b"".join(f.bytes for i, f in enumerate(frames) if keep[i])

    class Opaque:                                   # any object with is_speech: the host-side protocol loop
        def is_speech(self, b, sr):
            return vad_ref.energy_is_speech(np.frombuffer(b, dtype=np.int16), thr)

    class Batched(Opaque):                          # ... which asks for all decisions at once when it can
        calls = 0

        def speech_flags(self, frs, sr):
            Batched.calls += 1
            return ev.speech_flags(frs, sr)

    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        assert b"".join(vad.vad_collector(16000, 10, 1000, Opaque(), frames)) == b"".join(segs)
        assert b"".join(vad.vad_collector(16000, 10, 1000, Batched(), frames)) == b"".join(segs)
    assert Batched.calls == 1


def test_file_driven_enrol_and_evaluate(eng, golden, tmp_path, monkeypatch, capsys):
    """`create_speaker_models()` and `evaluate()` with NO arguments (model.py:351-388, evaluation.py:90-146):
    checkpoint, id list, id table, WAV tree and `{id}.pt` store under constants.ROOT / DATA_ORIGIN, row by
    row against what the reference's own functions produced on the same tree (golden `eval_*`)."""
    from speaker_verification_amd import constants, evaluation, model as model_mod
    g = golden["round2"]
    root = str(tmp_path)
    data_dir, rel, state = synth.write_verification_tree(root)
    monkeypatch.setattr(constants, "ROOT", root)
    monkeypatch.setattr(constants, "DATA_ORIGIN", data_dir)
    monkeypatch.chdir(tmp_path)                                        # eer_auc.png lands in the CWD, as there
    np.random.seed(int(g["eval_seeds"][0]))
    store = model_mod.create_speaker_models()
    order = [str(s) for s in g["eval_speaker_order"]]
    assert sorted(store) == sorted(order)
    assert sorted(os.listdir(os.path.join(root, "speaker_models"))) == sorted(s + ".pt" for s in order)
    got_enrolled = np.concatenate([store[s].numpy() for s in order])
    scale = np.abs(g["eval_enrolled"]).max()
    np.testing.assert_allclose(got_enrolled, g["eval_enrolled"], rtol=0, atol=5e-5 * scale)      # the libsvk network (dataset_embeddings)
    np.random.seed(int(g["eval_seeds"][1]))
    res = evaluation.evaluate()
    cols = [res["speaker_ids"].index(s) for s in order]                # the reference's os.listdir order
    np.testing.assert_allclose(res["scores"][:, cols], g["eval_scores"], rtol=0, atol=2e-5)
    np.testing.assert_array_equal(res["labels"][:, cols], g["eval_labels"])
    out = capsys.readouterr().out
    assert out.count("correct speaker") == len(rel) and "EER=" in out and "AUC=" in out and "Accuracy:" in out
    assert os.path.exists(tmp_path / "eer_auc.png")
    # EER / AUC / accuracy: the reference's numbers unless two scores of a row sit within the tolerance
    gap = np.sort(g["eval_scores"], axis=1)
    if (gap[:, -1] - gap[:, -2]).min() > 4e-5:
        assert res["accuracy"] == pytest.approx(float(g["eval_accuracy_pct"][0]))
    # EER: the reference's number from the reference's scores through THIS build's function ...
    eer_gold, auc_gold = evaluation.get_eer_auc(g["eval_labels"].flatten(), g["eval_scores"].flatten())[:2]
    assert eer_gold * 100 == pytest.approx(float(g["eval_eer_pct"][0]), abs=1e-6)
    assert auc_gold * 100 == pytest.approx(float(g["eval_auc_pct"][0]), abs=1e-6)
    # ... and from the GPU's scores whenever they rank the 27 pairs as the reference's do (the ROC only sees the order;
    # scores agree to 2e-5, so only a near-tie inside that band could reorder them)
    flat = np.sort(g["eval_scores"].flatten())
    if np.diff(flat).min() > 4e-5:
        np.testing.assert_array_equal(np.argsort(res["scores"][:, cols].flatten(), kind="stable"),
                                      np.argsort(g["eval_scores"].flatten(), kind="stable"))
        assert res["eer"] * 100 == pytest.approx(float(g["eval_eer_pct"][0]), abs=1e-6)
        assert res["auc"] * 100 == pytest.approx(float(g["eval_auc_pct"][0]), abs=1e-6)
    eer_o, auc_o = scoring_ref.k_fold_eer_auc(res["labels"].flatten(), res["scores"].flatten())
    assert res["eer"] == pytest.approx(eer_o, abs=1e-9) and res["auc"] == pytest.approx(auc_o, abs=1e-9)
    # the oracle chain, item by item, on the same tree and seeds
    from oracle import evaluation_ref
    np.random.seed(int(g["eval_seeds"][1]))
    o_scores, o_labels, _, _, _ = evaluation_ref.evaluate(data_dir, rel, state, {s: store[s].numpy() for s in order}, order)
    np.testing.assert_allclose(res["scores"][:, cols], o_scores, rtol=0, atol=2e-5)
    # load_wav keeps the reference's keyword (utils.py:170)
    from speaker_verification_amd import load_data
    sig = load_data.load_wav(filename=os.path.join(data_dir, rel[0]), sample_rate=16000)
    np.testing.assert_array_equal(sig, evaluation_ref.load_wav(os.path.join(data_dir, rel[0])))


def test_file_driven_evaluate_with_the_trained_checkpoint(eng, tmp_path, monkeypatch, capsys):
    """The reference's no-argument `create_speaker_models()` + `evaluate()` (model.py:351-388, evaluation.py:90-146) on a tree
    that carries the committed TRAINED checkpoint, with `constants.NORMALIZE` on (the checkpoint saw CMVN-normalised features):
    10 speakers the network never saw, 4 files each -- an operating point (accuracy, EER) instead of a coin flip, and the
    scores row by row against the oracle's per-utterance chain on the same tree, seeds and weights."""
    from oracle import evaluation_ref
    from speaker_verification_amd import constants, evaluation, model as model_mod
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = str(tmp_path)
    data_dir, rel, state = synth.write_verification_tree(
        root, n_speakers=10, utts_per_speaker=4, n_samples=40000,
        checkpoint=os.path.join(repo, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"))
    monkeypatch.setattr(constants, "ROOT", root)
    monkeypatch.setattr(constants, "DATA_ORIGIN", data_dir)
    monkeypatch.setattr(constants, "NORMALIZE", True)
    monkeypatch.chdir(tmp_path)
    np.random.seed(31)
    store = model_mod.create_speaker_models()
    np.random.seed(32)
    res = evaluation.evaluate()
    capsys.readouterr()
    assert len(store) == 10 and res["scores"].shape == (40, 10)
    assert res["accuracy"] >= 75.0 and res["eer"] < 0.2 and res["auc"] > 0.9, (res["accuracy"], res["eer"], res["auc"])
    order = res["speaker_ids"]
    np.random.seed(31)
    o_store = evaluation_ref.create_speaker_models(data_dir, rel, state, normalize=True)
    np.random.seed(32)
    o_scores, o_labels, o_acc, o_eer, o_auc = evaluation_ref.evaluate(data_dir, rel, state, o_store, order, normalize=True)
    scale = max(float(np.abs(v).max()) for v in o_store.values())
    for sid in order:
        np.testing.assert_allclose(store[sid].numpy(), o_store[sid], rtol=0, atol=5e-5 * scale)
    np.testing.assert_allclose(res["scores"], o_scores, rtol=0, atol=2e-5)
    np.testing.assert_array_equal(res["labels"], o_labels)
    flat = np.sort(o_scores.flatten())
    if np.diff(flat).min() > 4e-5:                       # no near-tie that a 2e-5 difference could reorder
        assert res["eer"] == pytest.approx(o_eer, abs=1e-9) and res["auc"] == pytest.approx(o_auc, abs=1e-9)
        assert res["accuracy"] == pytest.approx(o_acc)


@pytest.mark.parametrize("nfft", [8, 64, 128, 256, 2048, 4096, 8192, 300, 400, 1000, 1023])
def test_spectrum_any_length(sp, nfft):
    """processing.fft_spectrum / power_spectrum for every fft_points (processing.py:142-174): powers of two run the
    LDS Stockham FFT, other lengths the table-driven DFT; frames shorter than nfft are zero-padded, longer cropped (Q6)."""
    rng = np.random.default_rng(nfft)
    for flen in (min(nfft, 200), nfft + 37):
        frames = (rng.standard_normal((37, flen)) * 1000.0)
        want_p = ref.power_spectrum(frames, nfft)
        got_p = sp.processing.power_spectrum(frames, nfft)
        assert got_p.shape == want_p.shape == (37, nfft // 2 + 1)
        np.testing.assert_allclose(got_p, want_p, rtol=2e-4, atol=2e-5 * want_p.max())
        np.testing.assert_allclose(sp.processing.fft_spectrum(frames, nfft), ref.fft_spectrum(frames, nfft),
                                   rtol=2e-4, atol=2e-5 * np.sqrt(want_p.max() * nfft))


def test_mel_stage_wide_banks(eng):
    """svk_mel_features on banks the fused kernel never sees: 200 filters over 1 025 bins (dense random bank), MFE /
    LMFE / MFCC with and without c0 := log E, a frame count that is not a multiple of the tile."""
    from speaker_verification_amd import _lib
    from scipy.fftpack import dct
    rng = np.random.default_rng(8)
    # 300 filters: past the 256 the MFMA form of the kernel takes (its 64 x nf tile must fit LDS) -> the VALU form;
    # 10 filters over 129 bins and 130 frames: partial N tile, partial K chunk, three M tiles of one workgroup in use
    for T, bins, nf in ((130, 129, 10), (77, 1025, 300)):
        power = rng.random((T, bins)) * 50.0
        power[3] = 0.0
        bank = rng.random((nf, bins)) * (rng.random((nf, bins)) < 0.3)
        f, e = eng.mel_features(power, bank, _lib.OUT_LMFE, want_energy=True)
        np.testing.assert_allclose(f.cpu().numpy(), np.log(ref.zero_handling(power @ bank.T)), **FEAT_TOL)
        np.testing.assert_allclose(e.cpu().numpy(), ref.zero_handling(power.sum(axis=1)), rtol=2e-4)
    T, bins, nf = 77, 1025, 200
    power = rng.random((T, bins)) * 50.0
    power[5] = 0.0                                                     # zero frame: energy and mel energies -> eps
    bank = rng.random((nf, bins)) * (rng.random((nf, bins)) < 0.1)
    mel = ref.zero_handling(power @ bank.T)
    energy = ref.zero_handling(power.sum(axis=1))
    f, e = eng.mel_features(power, bank, _lib.OUT_MFE, want_energy=True)
    np.testing.assert_allclose(f.cpu().numpy(), mel, rtol=2e-4)
    np.testing.assert_allclose(e.cpu().numpy(), energy, rtol=2e-4)
    f, _ = eng.mel_features(power, bank, _lib.OUT_LMFE)
    np.testing.assert_allclose(f.cpu().numpy(), np.log(mel), **FEAT_TOL)
    cep = dct(np.log(mel), type=2, axis=-1, norm="ortho")[:, :30]
    f, _ = eng.mel_features(power, bank, _lib.OUT_MFCC, num_ceps=30, dc_elimination=False)
    np.testing.assert_allclose(f.cpu().numpy(), cep, **FEAT_TOL)
    cep[:, 0] = np.log(energy)
    f, _ = eng.mel_features(power, bank, _lib.OUT_MFCC, num_ceps=30, dc_elimination=True)
    np.testing.assert_allclose(f.cpu().numpy(), cep, **FEAT_TOL)


def test_cmvnw_long_clips_and_windows(eng):
    """cmvnw_tile_kernel (prefix sums in LDS; every clip here is at most 3 900 frames, so svk_cmvnw takes nothing else)
    against the oracle's direct window means: clips longer and shorter than the window, ragged batch.  The sliding-sum
    kernel (cmvnw_kernel, longer clips) is covered by tests/test_postprocessing_float64.py."""
    rng = np.random.default_rng(17)
    for T, C, win in ((2500, 40, 301), (90, 13, 301), (1024, 8, 31), (1025, 8, 5)):
        x = rng.standard_normal((T, C)) * 3.0 + 1.0
        for var in (False, True):
            got = eng.cmvnw(x.astype(np.float32), win, var).cpu().numpy()
            np.testing.assert_allclose(got, ref.cmvnw(x.astype(np.float32), win, var), rtol=2e-4, atol=2e-5)
    batch = rng.standard_normal((3, 700, 13)).astype(np.float32)
    nfr = np.array([700, 301, 12], dtype=np.int32)
    got = eng.cmvnw(batch, 301, True, n_frames=nfr).cpu().numpy()
    for u in range(3):
        np.testing.assert_allclose(got[u, :nfr[u]], ref.cmvnw(batch[u, :nfr[u]], 301, True), rtol=2e-4, atol=2e-5)
        np.testing.assert_array_equal(got[u, nfr[u]:], batch[u, nfr[u]:])


def test_rccl_wrappers_single_rank(eng):
    """svk_comm_* (SURVEY 8b's table): RCCL bound at run time; with one rank the all-gather is the identity.
    (N > 1 needs N GPUs: the driver's scaling run covers it through torch.distributed, and the sharding /
    padding logic around the collective runs on two gloo ranks in tests/test_distributed_cpu.py.)"""
    import ctypes as C
    from speaker_verification_amd import _lib
    lib = eng.lib
    info = (C.c_int32 * 2)()
    _lib.check(lib.svk_comm_info(eng.ctx, info), eng.ctx)
    assert info[0] == 0
    with pytest.raises(_lib.SvkError, match="svk_comm_init first"):
        _lib.check(lib.svk_allgather_f32(eng.ctx, None, None, 4), eng.ctx)
    uid = C.create_string_buffer(128)
    _lib.check(lib.svk_comm_unique_id(eng.ctx, uid), eng.ctx)
    assert any(uid.raw)
    _lib.check(lib.svk_comm_init(eng.ctx, uid, 1, 0), eng.ctx)
    try:
        _lib.check(lib.svk_comm_info(eng.ctx, info), eng.ctx)
        assert (info[0], info[1]) == (1, 0)
        with pytest.raises(_lib.SvkError, match="already has a communicator"):
            _lib.check(lib.svk_comm_init(eng.ctx, uid, 1, 0), eng.ctx)
        send = torch.randn(18581, 128, device=eng.device)                    # one rank's shard of 148 642 / 8
        recv = torch.zeros_like(send)
        eng._stream()
        _lib.check(lib.svk_allgather_f32(eng.ctx, eng._ptr(send), eng._ptr(recv), send.numel()), eng.ctx)
        eng.synchronize()
        assert torch.equal(send, recv)
    finally:
        _lib.check(lib.svk_comm_destroy(eng.ctx), eng.ctx)
    _lib.check(lib.svk_comm_info(eng.ctx, info), eng.ctx)
    assert info[0] == 0


def test_siamese_train_step_on_rocm(eng):
    """SURVEY 8f-4 / train_siamese.py:37-175: one contrastive step (embed both cubes of each pair, `Siamese.forward`
    loss = contrastive + LAMBDA * sum of parameter norms, backward, SGD) on the GPU against the SAME step on
    torch-CPU: loss, every gradient and every updated parameter.  (The loss VALUE is pinned to the reference's own
    `Siamese.forward` by `test_siamese_forward_against_reference_loss`; the restated formula used at the end of this
    test is held to the same golden numbers in tests/test_oracle_golden.py.)"""
    import copy
    from speaker_verification_amd.model import seeded_model
    from speaker_verification_amd.train_siamese import make_criterion, siamese_train_step
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(6, 1, 20, 80, 40, generator=g), torch.randn(6, 1, 20, 80, 40, generator=g)
    y = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0, 1.0])
    cpu_model = seeded_model(5, n_labels=4)
    gpu_model = copy.deepcopy(cpu_model).to(eng.device)
    crit = make_criterion(0.001, 2.0)
    opt_c = torch.optim.SGD(cpu_model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4)
    opt_g = torch.optim.SGD(gpu_model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4)
    for step in range(2):
        lc = siamese_train_step(cpu_model, crit, opt_c, a, b, y)
        lg = siamese_train_step(gpu_model, crit, opt_g, a.to(eng.device), b.to(eng.device), y.to(eng.device))
        assert lg == pytest.approx(lc, rel=2e-4 if step == 0 else 1e-2)
        if step > 0:             # the second step starts from weights that already differ by rounding: loss only
            break
        # (a conv bias in front of a training-mode BatchNorm has a mathematically ZERO gradient: both sides hold
        # rounding noise there, so the absolute tolerance is set by the gradient scale of the whole model)
        gscale = max(float(p.grad.abs().max()) for p in cpu_model.parameters())
        for (name, pc), pg in zip(cpu_model.named_parameters(), gpu_model.parameters()):
            scale = max(float(pc.grad.abs().max()), 1e-3 * gscale)
            torch.testing.assert_close(pg.grad.cpu(), pc.grad, rtol=2e-3, atol=2e-3 * scale, msg=lambda m: name + ": " + m)
            # the update is lr * (momentum-filtered) gradient: the gradient tolerance times the learning rate
            torch.testing.assert_close(pg.detach().cpu(), pc.detach(), rtol=1e-4,
                                       atol=1e-6 + 0.01 * 4e-3 * scale * (step + 1), msg=lambda m: name + ": " + m)
    # the loss itself against the restated formula (siamese.py:14-25)
    gpu_model.eval()
    with torch.no_grad():
        o1, o2 = gpu_model(a.to(eng.device), development=False), gpu_model(b.to(eng.device), development=False)
        loss = float(crit(gpu_model, y.to(eng.device), o1, o2))
    norms = [float(torch.norm(p.detach())) for p in gpu_model.parameters()]
    want = scoring_ref.contrastive_loss(y.numpy(), o1.cpu().numpy(), o2.cpu().numpy(), norms, 0.001, 2.0)
    assert loss == pytest.approx(want, rel=1e-4)


def _cpu_layers(state, x, layers, pool=True, slopes=None):
    """conv -> BatchNorm (eval, UNFOLDED) -> PReLU for each (tag, stride) of `layers` on torch-CPU, then MaxPool3d((1,1,2))
    when `pool`: model.py:141-169 layer by layer, the oracle of the libsvk network kernels.  x: (n, C, D, H, W);
    slopes: {tag: replacement PReLU slope tensor}."""
    import torch.nn.functional as F
    with torch.no_grad():
        for tag, stride in layers:
            x = F.conv3d(x, state[f"conv{tag}.weight"], state[f"conv{tag}.bias"], stride=stride)
            x = F.batch_norm(x, state[f"batch_norm{tag}.running_mean"], state[f"batch_norm{tag}.running_var"],
                             state[f"batch_norm{tag}.weight"], state[f"batch_norm{tag}.bias"], training=False, eps=1e-5)
            x = F.prelu(x, (slopes or {}).get(tag, state[f"PReLu{tag}.weight"]))
        if pool:
            x = F.max_pool3d(x, kernel_size=(1, 1, 2), stride=(1, 1, 2))
    return x.numpy()


BLOCK1 = (("1_1", (1, 1, 1)), ("1_2", (1, 2, 1)))
BLOCK2 = (("2_1", (1, 1, 1)), ("2_2", (1, 2, 1)))


def _net(eng, init_seed, perturb_seed):
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    model = seeded_model(init_seed, n_labels=8)
    model.load_state_dict(perturb_inference_state(model.state_dict(), perturb_seed))
    model = model.to(eng.device).eval()
    return model, model.fused_inference(), {k: v.detach().cpu() for k, v in model.state_dict().items()}


def test_c3d2_first_block_kernel(eng):
    """svk_c3d2_stage1 (cube -> conv1_1 -> BN -> PReLU -> conv1_2 -> BN -> PReLU -> pool1 in one MFMA kernel,
    model.py:110-117,141-150; two-piece f16 products on v_mfma_f32_16x16x32_f16, f32 accumulation) against the same layers of the
    CPU oracle's network (torch-CPU f32, unfolded BatchNorm) at the tolerance the f32 kernels are held to, with a too-short clip
    (crop -1 -> zero cube), negative and per-channel slopes."""
    model, emb, state = _net(eng, 41, 42)
    tables = emb.stage1_tables()
    rng = np.random.default_rng(3)
    n, T = 5, 131
    feat = (rng.standard_normal((n, T, 40)) * 2.0 - 6.0).astype(np.float32)
    crops = rng.integers(0, T - 80, size=(n, 20)).astype(np.int32)
    crops[3] = -1
    cubes = np.stack([model_ref.feature_cube(feat[u], np.maximum(crops[u], 0))[0] for u in range(n)])[:, None]
    cubes[3] = 0.0
    want = _cpu_layers(state, torch.from_numpy(cubes), BLOCK1)                            # (n, 16, 16, 36, 18)
    scale = np.abs(want).max()
    got = eng.c3d2_stage1(feat, crops, tables).cpu().numpy()                               # [n][d][h][w][c]
    print("first block: max |diff| / scale %.2e" % (np.abs(got.transpose(0, 4, 1, 2, 3) - want).max() / scale))
    np.testing.assert_allclose(got.transpose(0, 4, 1, 2, 3), want, rtol=1e-4, atol=4e-6 * scale)
    # the cube handed over as feature rows (what C3D2.forward does with a cube): the same numbers, bit for bit
    rows = eng.to_device(cubes).view(n, 1600, 40)
    assert torch.equal(eng.c3d2_stage1(rows, emb.crop_starts(n, eng.device), tables), eng.to_device(got))
    w1frag, b1, s1, w2frag, b2, s2, slope01 = tables
    assert slope01                                        # perturb_inference_state draws slopes in [0.1, 0.4]: the fast PReLU ran above
    same = eng.c3d2_stage1(feat, crops, (w1frag, b1, s1, w2frag, b2, s2, False)).cpu().numpy()
    np.testing.assert_array_equal(same, got)              # general and [0, 1] PReLU forms agree bit for bit
    # negative / per-channel slopes on both layers: PReLU before the max, as the reference orders them
    s1n, s2n = torch.linspace(-0.3, 0.9, 16), torch.linspace(-0.5, 0.4, 16)
    want_n = _cpu_layers(state, torch.from_numpy(cubes), BLOCK1, slopes={"1_1": s1n, "1_2": s2n})
    got_n = eng.c3d2_stage1(feat, crops, (w1frag, b1, s1n.to(eng.device), w2frag, b2, s2n.to(eng.device), False)).cpu().numpy()
    np.testing.assert_allclose(got_n.transpose(0, 4, 1, 2, 3), want_n, rtol=1e-4, atol=4e-6 * np.abs(want_n).max())


def test_c3d2_embedding_on_gpu(eng, golden):
    """The reference's own `C3D2(...)(x, development=False)` / `create_Speaker_Model` outputs (tests/golden/c3d2_embed.npz,
    made by importing /root/reference/model.py) against this build's drop-in calls -- every one of them the seven libsvk
    kernels: `model(x, development=False)` as evaluation.py:68-69 calls it, `create_Speaker_Model` (model.py:188-191),
    `fused_inference()(x)`, `Evaluation.embed`."""
    from speaker_verification_amd import evaluation
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    g = golden["c3d2_embed"]
    model = seeded_model(int(g["init_seed"][0]), int(g["n_labels"][0]), 1)
    model.load_state_dict(perturb_inference_state(model.state_dict(), int(g["perturb_seed"][0])))
    cubes = (np.random.default_rng(int(g["cube_seed"][0])).standard_normal((3, 1, 20, 80, 40)) * 2.0 - 6.0
             ).astype(np.float32)
    model = model.to(eng.device).eval()
    x = torch.from_numpy(cubes).to(eng.device)
    assert model.runs_on_kernels(x)
    plain = model(x, development=False)                   # grad mode on, as the reference calls it: still the kernels
    assert plain.grad_fn is None
    scale = np.abs(g["embed"]).max()
    print("golden embeddings: max |diff| / scale %.2e" % (np.abs(plain.cpu().numpy() - g["embed"]).max() / scale))
    np.testing.assert_allclose(plain.cpu().numpy(), g["embed"], rtol=0, atol=1e-5 * scale)
    assert torch.equal(model.fused_inference()(x), plain)
    sm = model.create_Speaker_Model(x[1:2])
    np.testing.assert_allclose(sm.detach().cpu().numpy(), g["speaker_model"], rtol=0, atol=1e-5 * scale)
    ev = evaluation.Evaluation(model, {"a": g["embed"][0:1], "b": g["embed"][1:2], "c": g["embed"][2:3]})
    assert torch.equal(ev.embed(cubes), plain)
    sims, assigned = ev.compute_Similarity(x[2:3])
    assert np.argmax(sims) == 2 and sims[2] == pytest.approx(1.0, abs=1e-5) and assigned[2] == 1
    # the softmax head on top of the kernels' embedding (development=True, model.py:170-172)
    probs = model(x)
    with torch.no_grad():
        want = torch.softmax(model.FC6(model.PReLu5(plain)), dim=1)
    torch.testing.assert_close(probs, want, rtol=1e-6, atol=1e-7)


def test_trained_checkpoint_embeddings_against_the_reference(eng, golden):
    """The committed trained checkpoint: PCM -> pre-emphasis -> log-mel -> CMVN -> cube -> C3D2 on the GPU against what the
    REFERENCE's own speechpy + FeatureCube + load_checkpoint + forward produced for the same clips and crops
    (tests/golden/round4.npz), through the production route (no cube in HBM), through `model(cube)` the way
    evaluation.py:113-121 calls it, and the cosines evaluation.py:77 computes from them."""
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    g = golden["round4"]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = torch.load(os.path.join(repo, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu",
                    weights_only=True)
    model = C3D2(100, 1).load_checkpoint(ck)                              # the reference's loading call (model.py:177-186)
    assert next(model.parameters()).is_cuda
    pcm = np.stack([synth.speaker_clip(int(s), int(u)) for s, u in g["clip_ids"]])
    pipe = VerificationPipeline(model, use_vad=False, normalize=True, preemph_cof=0.98, micro_batch=3)
    scale = float(np.abs(g["embed"]).max())
    emb = pipe.embed(pcm, crop_idx=g["crop_idx"])
    print("trained checkpoint, PCM -> embedding vs the reference: max |diff| / scale %.2e"
          % (np.abs(emb.cpu().numpy() - g["embed"]).max() / scale))
    np.testing.assert_allclose(emb.cpu().numpy(), g["embed"], rtol=0, atol=5e-5 * scale)
    _, inter = pipe.embed(pcm, crop_idx=g["crop_idx"], return_intermediates=True)
    cubes = torch.cat([d["cube"] for d in inter])
    np.testing.assert_allclose([float(c_.abs().sum()) for c_ in cubes], g["cube_abssum"], rtol=1e-5)
    via_model = model(cubes, development=False)
    np.testing.assert_allclose(via_model.cpu().numpy(), g["embed"], rtol=0, atol=5e-5 * scale)
    np.testing.assert_allclose(model(cubes).detach().cpu().numpy()[:, :8], g["softmax_top"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(model.create_Speaker_Model(cubes[3:4]).detach().cpu().numpy(), g["speaker_model"], rtol=0, atol=5e-5 * scale)
    np.testing.assert_allclose(pipe.score(emb, emb).cpu().numpy(), g["cosine"], rtol=0, atol=1e-5)


def test_reference_call_surface_runs_the_libsvk_network(eng):
    """Which code runs a forward (model.C3D2.forward): the libsvk kernels for inference calls on the device, the torch
    layers wherever autograd or another input layout needs them; and the inference snapshot follows the weights."""
    from speaker_verification_amd.model import C3D2, FusedEmbedder, seeded_model
    model, emb, state = _net(eng, 21, 22)
    x = torch.randn((2, 1, 20, 80, 40), device=eng.device) * 2 - 6
    want = torch.from_numpy(model_ref.c3d2_embed(state, x.cpu().numpy()).numpy())
    scale = float(want.abs().max())
    got = model(x, development=False)
    assert float((got.cpu() - want).abs().max()) <= 1e-5 * scale
    # not an inference call: training mode, a gradient asked of the input, a host tensor, the opt-out switch
    assert not model.runs_on_kernels(x.cpu()) and not model.runs_on_kernels(x.clone().requires_grad_(True))
    with torch.no_grad():
        assert model.runs_on_kernels(x.clone().requires_grad_(True))
    model.train()
    assert not model.runs_on_kernels(x)
    model.eval()
    model.inference_kernels = False
    assert not model.runs_on_kernels(x)
    del model.inference_kernels
    assert model.runs_on_kernels(x)
    assert not C3D2(4, 3).to(eng.device).eval().runs_on_kernels(torch.zeros((1, 3, 20, 80, 40), device=eng.device))
    # a gradient through the torch layers still works on the device (training / fine-tuning)
    xg = x.clone().requires_grad_(True)
    model(xg, development=False).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    # the snapshot follows the weights: same object while nothing changed, rebuilt after an in-place update or a load
    assert model.fused_inference() is model.fused_inference()
    first = model.fused_inference()
    with torch.no_grad():
        model.conv3_1.bias.add_(0.5)
    assert model.fused_inference() is not first
    changed = model(x, development=False)
    assert float((changed - got).abs().max()) > 1e-3 * scale
    state2 = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want2 = torch.from_numpy(model_ref.c3d2_embed(state2, x.cpu().numpy()).numpy())
    assert float((changed.cpu() - want2).abs().max()) <= 1e-5 * float(want2.abs().max())
    model.load_state_dict({k: v for k, v in state.items()})
    assert torch.equal(model(x, development=False), got)
    # a model that is not C3D2-shaped has no libsvk form: loud, not a silent framework fallback
    other = C3D2(4, 1)
    other.conv1_1 = torch.nn.Conv3d(1, 16, kernel_size=(3, 1, 3))
    with pytest.raises(ValueError, match="C3D2's layers"):
        FusedEmbedder(other.to(eng.device).eval())
    with pytest.raises(ValueError):
        emb(torch.zeros((2, 1, 20, 80, 39), device=eng.device))
    # more cubes than one launch sequence takes: chunked inside, same rows
    many = torch.randn((70, 1, 20, 80, 40), device=eng.device)
    assert torch.equal(emb(many, batch=32), emb(many))


def test_network_is_indifferent_to_a_checkpoints_channel_scales(eng):
    """model.py:141-169 is the same function when a checkpoint carries channel c of a layer a > 0 times larger (BatchNorm's gamma,
    beta) and the next layer's weights on it a times smaller; the half pairs the kernels multiply are not (floor 2^-25, ceiling
    65 504).  A network regauged by a = 10^-3 .. 10^3 per channel on every layer -- activations up to ~10^5 and weights down to
    ~10^-5 as the checkpoint states them -- gives the ORIGINAL network's embeddings (torch-CPU f32, unfolded BatchNorm) at the
    end-to-end bar, through C3D2.forward on the device; and its first block's output is the original's in the units `act_scale`
    names.  (FusedEmbedder fixes every channel's power of two before it splits weights: tests/test_host_logic.py has the exact,
    CPU-side statement for powers of two.)"""
    from speaker_verification_amd.model import _LAYERS
    from test_host_logic import _regauged
    model, emb, state = _net(eng, 61, 62)
    gen = torch.Generator().manual_seed(9)
    alphas = [torch.pow(10.0, 6.0 * torch.rand((t[2],), generator=gen) - 3.0) for t in _LAYERS]
    other = _regauged(model, alphas).eval()
    rng = np.random.default_rng(4)
    cubes = torch.from_numpy((rng.standard_normal((6, 1, 20, 80, 40)) * 2.0 - 1.0).astype(np.float32))
    with torch.no_grad():
        want = model.cpu().torch_layers(cubes).numpy()                          # the original network on torch-CPU
        model.to(eng.device)
        assert other.runs_on_kernels(cubes.to(eng.device))
        got = other(cubes.to(eng.device), development=False).cpu().numpy()      # the regauged one through the kernels
        base = model(cubes.to(eng.device), development=False).cpu().numpy()
    scale = np.abs(want).max()
    print("regauged network: max |diff| / scale %.2e (original through the kernels: %.2e)"
          % (np.abs(got - want).max() / scale, np.abs(base - want).max() / scale))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=5e-5 * scale)
    np.testing.assert_allclose(got, base, rtol=1e-4, atol=2e-5 * scale)
    e2 = other.fused_inference()
    rows = cubes.to(eng.device).view(6, 1600, 40)
    y1 = eng.c3d2_stage1(rows, emb.crop_starts(6, eng.device), emb.stage1_tables())
    y2 = eng.c3d2_stage1(rows, e2.crop_starts(6, eng.device), e2.stage1_tables()) / e2.act_scale[1].to(eng.device)
    # (y1 itself is in the original's units only if its own channel scales are one, which perturb_inference_state's BatchNorm gives)
    assert all(bool((s == 1).all()) for s in emb.act_scale)
    ref = y1 * alphas[1].to(eng.device)
    np.testing.assert_allclose(y2.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=4e-6 * float(ref.abs().max()))
    with pytest.raises(ValueError, match="65 504"):
        model(cubes.to(eng.device) * 1e5, development=False)                    # outside the half pairs' domain: refused, not wrong


def test_c3d2_second_block_kernels(eng):
    """svk_c3d2_stage2 (conv2_1 -> BN -> PReLU -> conv2_2 -> BN -> PReLU -> pool2, model.py:119-124,151-158, both direct-form
    kernels on two-piece f16 products) against the same layers on torch-CPU with unfolded BatchNorm, on a random activation in stage 1's
    output layout."""
    model, emb, state = _net(eng, 51, 52)
    tables = emb.stage2_tables()
    rng = np.random.default_rng(4)
    act1 = rng.standard_normal((3, 16, 36, 18, 16)).astype(np.float32)         # [n][d][h][w][c]
    want = _cpu_layers(state, torch.from_numpy(act1.transpose(0, 4, 1, 2, 3).copy()), BLOCK2)    # (n, 32, 12, 15, 7)
    scale = np.abs(want).max()
    assert tables[6]                                       # slopes in [0.1, 0.4]: the two-instruction PReLU runs
    got = eng.c3d2_stage2(eng.to_device(act1), tables).cpu().numpy()                              # [n][12][15][7][32]
    print("second block: max |diff| / scale %.2e" % (np.abs(got.transpose(0, 4, 1, 2, 3) - want).max() / scale))
    np.testing.assert_allclose(got.transpose(0, 4, 1, 2, 3), want, rtol=1e-4, atol=4e-6 * scale)
    got_g = eng.c3d2_stage2(eng.to_device(act1), tables[:6] + (False,)).cpu().numpy()
    np.testing.assert_array_equal(got_g, got)              # general and [0, 1] PReLU forms agree bit for bit
    s1n, s2n = torch.linspace(-0.3, 0.9, 32), torch.linspace(-0.5, 0.4, 32)
    want_n = _cpu_layers(state, torch.from_numpy(act1.transpose(0, 4, 1, 2, 3).copy()), BLOCK2, slopes={"2_1": s1n, "2_2": s2n})
    t_n = (tables[0], tables[1], s1n.to(eng.device), tables[3], tables[4], s2n.to(eng.device), False)
    got_n = eng.c3d2_stage2(eng.to_device(act1), t_n).cpu().numpy()
    np.testing.assert_allclose(got_n.transpose(0, 4, 1, 2, 3), want_n, rtol=1e-4, atol=4e-6 * np.abs(want_n).max())


def _conv31_unchunk(y):
    """svk_c3d2_conv31's chunked, column-major output [n][10 d][8 chunks][5 w][15 h][8] -> (n, 64, 10, 15, 5)."""
    n = y.shape[0]
    return np.ascontiguousarray(y.transpose(0, 2, 5, 1, 4, 3)).reshape(n, 64, 10, 15, 5)


def test_c3d2_conv31_kernel(eng):
    """svk_c3d2_conv31 (conv3_1 -> BN -> PReLU, model.py:126-128,159-161, a direct-form kernel on two-piece f16
    products) against the same layer on torch-CPU with unfolded BatchNorm; per-channel and negative slopes."""
    model, emb, state = _net(eng, 61, 62)
    tables = emb.conv31_tables()
    assert tables is not None and tables[3]
    rng = np.random.default_rng(5)
    act = rng.standard_normal((3, 12, 15, 7, 32)).astype(np.float32)            # [n][d][h][w][c]
    x = torch.from_numpy(act.transpose(0, 4, 1, 2, 3).copy())
    want = _cpu_layers(state, x, (("3_1", (1, 1, 1)),), pool=False)             # (n, 64, 10, 15, 5)
    scale = np.abs(want).max()
    got = eng.c3d2_conv31(eng.to_device(act), tables).cpu().numpy()             # [n][10][8][5][15][8]
    print("conv3_1 kernel, max |diff| / scale: %.2e" % (np.abs(_conv31_unchunk(got) - want).max() / scale))
    np.testing.assert_allclose(_conv31_unchunk(got), want, rtol=1e-4, atol=4e-6 * scale)
    same = eng.c3d2_conv31(eng.to_device(act), tables[:3] + (False,)).cpu().numpy()
    np.testing.assert_array_equal(same, got)                                     # general and [0, 1] PReLU forms agree
    sn = torch.linspace(-0.5, 0.4, 64)
    got_n = eng.c3d2_conv31(eng.to_device(act), (tables[0], tables[1], sn.to(eng.device), False)).cpu().numpy()
    want_n = _cpu_layers(state, x, (("3_1", (1, 1, 1)),), pool=False, slopes={"3_1": sn})
    np.testing.assert_allclose(_conv31_unchunk(got_n), want_n, rtol=1e-4, atol=4e-6 * scale)
    with pytest.raises(ValueError):
        eng.c3d2_conv31(torch.zeros((2, 10, 15, 5, 64), device=eng.device), tables)
    assert eng.lib.svk_c3d2_conv31(eng.ctx, None, 1, None, None, None, 0, None) == -1


def _to_chunked(x):
    """(n, C, D, H, W) -> the chunked layout of csrc/c3d2_tail.hip: [n][D][C / 8][H * W][8]."""
    n, C, D, H, W = x.shape
    return np.ascontiguousarray(x.reshape(n, C // 8, 8, D, H * W).transpose(0, 3, 1, 4, 2))


def _from_chunked(y, H, W):
    """[n][D][C / 8][H * W][8] -> (n, C, D, H, W)."""
    n, D, Cg, P, _ = y.shape
    return np.ascontiguousarray(y.transpose(0, 2, 4, 1, 3)).reshape(n, Cg * 8, D, H, W)


def test_c3d2_tail_kernels(eng):
    """svk_c3d2_conv41, svk_c3d2_conv42, svk_c3d2_fc5 (model.py:132-139,165-170: conv4_1 -> BN -> PReLU -> conv4_2 -> BN ->
    PReLU -> flatten -> FC5 as GEMMs over the batch; conv4_1 direct-form on two-piece f16 products, conv4_2 Winograd F(2,3) along
    depth with host-transformed weights) each against
    the same layer on torch-CPU with unfolded BatchNorm: batches of 1, 3 (one partial group of 16 cubes), 37 (2 full + 1
    partial), 70 (several items per workgroup for FC5's 64-cube groups) and 520 cubes; the 2 100-cube case of conv4_2
    (several items per workgroup); negative / per-channel slopes."""
    import torch.nn.functional as F
    model, emb, state = _net(eng, 91, 92)
    t41, t42, tfc = emb.conv41_tables(), emb.conv42_tables(), emb.fc5_tables()
    assert t41 is not None and t42 is not None and tfc is not None and t41[3] and t42[3]
    rng = np.random.default_rng(8)

    def layer(tag, x, slope=None):
        return _cpu_layers(state, torch.from_numpy(x), ((tag, (1, 1, 1)),), pool=False, slopes=None if slope is None else {tag: slope})

    for n in (1, 3, 37, 70, 520):
        # conv4_1: (n, 64, 8, 9, 5) -> (n, 128, 6, 9, 3)
        x = rng.standard_normal((n, 64, 8, 9, 5)).astype(np.float32)
        want = layer("4_1", x)
        got = _from_chunked(eng.c3d2_conv41(eng.to_device(_to_chunked(x)), t41).cpu().numpy(), 9, 3)
        err41 = np.abs(got - want).max() / np.abs(want).max()
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=4e-6 * np.abs(want).max())
        # conv4_2: (n, 128, 6, 9, 3) -> (n, 128, 4, 3, 3)
        x2 = rng.standard_normal((n, 128, 6, 9, 3)).astype(np.float32)
        want2 = layer("4_2", x2)
        got2c = eng.c3d2_conv42(eng.to_device(_to_chunked(x2)), t42)
        got2 = _from_chunked(got2c.cpu().numpy(), 3, 3)
        err42 = np.abs(got2 - want2).max() / np.abs(want2).max()
        np.testing.assert_allclose(got2, want2, rtol=1e-4, atol=4e-6 * np.abs(want2).max())
        # FC5 on conv4_2's chunked output: model.py:168 flattens NCDHW
        with torch.no_grad():
            want3 = F.linear(torch.from_numpy(got2).reshape(n, 4608), state["FC5.weight"], state["FC5.bias"]).numpy()
        got3 = eng.c3d2_fc5(got2c, tfc).cpu().numpy()
        errfc = np.abs(got3 - want3).max() / np.abs(want3).max()
        np.testing.assert_allclose(got3, want3, rtol=1e-4, atol=4e-6 * np.abs(want3).max())
        assert torch.equal(eng.c3d2_fc5(got2c, tfc), eng.c3d2_fc5(got2c, tfc))                     # fixed summation order
        print("tail kernels, %d cubes: max |diff| / scale conv4_1 %.2e, conv4_2 %.2e, FC5 %.2e" % (n, err41, err42, errfc))
    # several items per workgroup for conv4_2 (2 items per group of 16 cubes; 256 workgroups): 2 100 cubes, sampled rows
    x2 = rng.standard_normal((2100, 128, 6, 9, 3)).astype(np.float32)
    got2 = eng.c3d2_conv42(eng.to_device(_to_chunked(x2)), t42)
    assert torch.equal(got2, eng.c3d2_conv42(eng.to_device(_to_chunked(x2)), t42))
    pick = [0, 15, 16, 1000, 2047, 2048, 2099]
    want2 = layer("4_2", x2[pick])
    np.testing.assert_allclose(_from_chunked(got2[pick].cpu().numpy(), 3, 3), want2, rtol=1e-4, atol=4e-6 * np.abs(want2).max())
    del got2, x2
    # general PReLU (negative and per-channel slopes) and the [0, 1] form agree where both apply
    x = rng.standard_normal((5, 64, 8, 9, 5)).astype(np.float32)
    xc = eng.to_device(_to_chunked(x))
    np.testing.assert_array_equal(eng.c3d2_conv41(xc, t41[:3] + (False,)).cpu().numpy(), eng.c3d2_conv41(xc, t41).cpu().numpy())
    sn = torch.linspace(-0.5, 0.4, 128)
    got_n = _from_chunked(eng.c3d2_conv41(xc, (t41[0], t41[1], sn.to(eng.device), False)).cpu().numpy(), 9, 3)
    want_n = layer("4_1", x, sn)
    np.testing.assert_allclose(got_n, want_n, rtol=1e-4, atol=4e-6 * np.abs(want_n).max())
    # error paths: wrong layouts are refused by the host layer, NULL buffers by the library
    with pytest.raises(ValueError):
        eng.c3d2_conv41(torch.zeros((21, 10, 15, 5, 64), device=eng.device), t41)
    # ... and so are weight blocks of another layer's shape or dtype (the kernel would read them out of bounds) and short bias / slope rows
    with pytest.raises(ValueError, match="weight blocks"):
        eng.c3d2_conv41(xc, (t42[0],) + t41[1:])
    with pytest.raises(ValueError, match="weight blocks"):
        eng.c3d2_conv41(xc, (t41[0].float(),) + t41[1:])
    with pytest.raises(ValueError, match="weight blocks"):
        eng.c3d2_conv42(eng.c3d2_conv41(xc, t41), (t41[0],) + t42[1:])
    with pytest.raises(ValueError, match="bias / slope"):
        eng.c3d2_conv41(xc, (t41[0], t41[1][:64], t41[2], True))
    assert eng.lib.svk_c3d2_conv41(eng.ctx, None, 1, None, None, None, 0, None) == -1
    assert eng.lib.svk_c3d2_conv42(eng.ctx, None, 1, None, None, None, 0, None) == -1
    assert eng.lib.svk_c3d2_fc5(eng.ctx, None, 1, None, None, None, None) == -1
    assert eng.lib.svk_c3d2_conv42(eng.ctx, None, 0, None, None, None, 0, None) == 0


def test_c3d2_conv32_in_the_last_blocks_shape(eng, monkeypatch):
    """svk_c3d2_conv32t (conv3_2 -> BN -> PReLU, model.py:129-131,162-164; a per-(cube, column) kernel on the f16 matrix pipe,
    two waves per N tile splitting K, work items from a device-wide counter one ahead) against
    the same layer on torch-CPU with unfolded BatchNorm: batches of 1, 3, 37 and 700 cubes (3 500 items on 256 workgroups); the
    column-major chunked output of conv3_1 it stages from; both item assignments."""
    model, emb, state = _net(eng, 95, 96)
    t32t, t31 = emb.conv32t_tables(), emb.conv31_tables()
    assert t32t is not None and t32t[3]
    rng = np.random.default_rng(12)

    def layer(x, slope=None):
        return _cpu_layers(state, torch.from_numpy(x), (("3_2", (1, 1, 1)),), pool=False, slopes=None if slope is None else {"3_2": slope})

    def to_in(x):      # (n, 64, 10, 15, 5) -> [n][10 d][8 chunks][5 w][15 h][8]
        n = x.shape[0]
        return np.ascontiguousarray(x.reshape(n, 8, 8, 10, 15, 5).transpose(0, 3, 1, 5, 4, 2))

    for n in (1, 3, 37, 700):
        x = rng.standard_normal((n, 64, 10, 15, 5)).astype(np.float32)
        np.testing.assert_array_equal(_conv31_unchunk(to_in(x)), x)                   # the two layout helpers are inverses
        got_c = eng.c3d2_conv32t(eng.to_device(to_in(x)), t32t)                      # [n][8][8][45][8]
        pick = list(range(n)) if n <= 37 else [0, 15, 16, 333, 687, 688, 699]
        want = layer(x[pick])
        got = _from_chunked(got_c[pick].cpu().numpy(), 9, 5)
        print("conv3_2 (last block's shape), %d cubes: max |diff| / scale %.2e" % (n, np.abs(got - want).max() / np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=4e-6 * np.abs(want).max())
        assert torch.equal(got_c, eng.c3d2_conv32t(eng.to_device(to_in(x)), t32t))
    monkeypatch.setenv("SVK_C3D2_STATIC_ITEMS", "1")                                   # fixed-stride items: the same results
    assert torch.equal(got_c, eng.c3d2_conv32t(eng.to_device(to_in(x)), t32t))
    monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS")
    sn = torch.linspace(-0.5, 0.4, 64)
    got_n = _from_chunked(eng.c3d2_conv32t(eng.to_device(to_in(x[:5])), (t32t[0], t32t[1], sn.to(eng.device), False)).cpu().numpy(), 9, 5)
    want_n = layer(x[:5], sn)
    np.testing.assert_allclose(got_n, want_n, rtol=1e-4, atol=4e-6 * np.abs(want_n).max())
    # conv3_1 -> conv3_2 chained through the chunked layout, against the two layers on torch-CPU
    a31 = rng.standard_normal((23, 12, 15, 7, 32)).astype(np.float32)
    chain = eng.c3d2_conv32t(eng.c3d2_conv31(eng.to_device(a31), t31), t32t).cpu().numpy()
    want_c = _cpu_layers(state, torch.from_numpy(a31.transpose(0, 4, 1, 2, 3).copy()), (("3_1", (1, 1, 1)), ("3_2", (1, 1, 1))), pool=False)
    np.testing.assert_allclose(_from_chunked(chain, 9, 5), want_c, rtol=1e-4, atol=6e-6 * np.abs(want_c).max())
    with pytest.raises(ValueError):
        eng.c3d2_conv32t(torch.zeros((2, 12, 15, 7, 32), device=eng.device), t32t)
    assert eng.lib.svk_c3d2_conv32t(eng.ctx, None, 1, None, None, None, 0, None) == -1


def test_network_kernels_many_items_per_workgroup(eng):
    """The network kernels are persistent (a workgroup loops over work items, the first block prefetching the next item's
    patch inside the current one's matrix work): the small-batch tests above give every workgroup at most one item, so
    here each gets several -- batches of 64 / 256 / 200 cubes, sampled cubes against the torch-CPU layers with unfolded
    BatchNorm; bitwise repeatable; the same results whichever workgroup takes an item."""
    model, emb, state = _net(eng, 71, 72)
    g = torch.Generator(device=eng.device)
    g.manual_seed(5)
    # first block: 64 cubes = 2 304 items over 256 workgroups
    n, T = 64, 150
    feat = torch.randn((n, T, 40), device=eng.device, generator=g) * 2 - 6
    crops = torch.randint(0, T - 80, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
    crops[7] = -1
    t1 = emb.stage1_tables()
    got1 = eng.c3d2_stage1(feat, crops, t1)
    assert torch.equal(got1, eng.c3d2_stage1(feat, crops, t1))
    # four cubes of the 64 (first, the zero cube's neighbour, middle, last: items that are a workgroup's 1st .. 9th)
    pick = [0, 8, 31, 63]
    fh, ch = feat.cpu().numpy(), crops.cpu().numpy()
    cubes = np.stack([model_ref.feature_cube(fh[u], np.maximum(ch[u], 0))[0] for u in pick])[:, None]
    want1 = _cpu_layers(state, torch.from_numpy(cubes), BLOCK1)                                     # (4, 16, 16, 36, 18)
    g4 = got1[pick].permute(0, 4, 1, 2, 3).cpu().numpy()
    print("first block, 64 cubes vs torch-CPU: max |diff| / scale %.2e" % (np.abs(g4 - want1).max() / np.abs(want1).max()))
    np.testing.assert_allclose(g4, want1, rtol=1e-4, atol=4e-6 * np.abs(want1).max())
    zero = _cpu_layers(state, torch.zeros((1, 1, 20, 80, 40)), BLOCK1)                               # the zero cube (crop -1)
    np.testing.assert_allclose(got1[7:8].permute(0, 4, 1, 2, 3).cpu().numpy(), zero, rtol=1e-4, atol=4e-6 * np.abs(want1).max())
    # second block: 256 cubes = 2 304 / 5 376 items over 512 workgroups
    act1 = torch.randn((256, 16, 36, 18, 16), device=eng.device, generator=g)
    t2 = emb.stage2_tables()
    w2 = eng.c3d2_stage2(act1, t2)
    assert torch.equal(w2, eng.c3d2_stage2(act1, t2))
    # work items drawn from the device-wide counter (default) or at a fixed stride: the same results, bit for bit
    t31 = emb.conv31_tables()
    a2s = torch.randn((200, 12, 15, 7, 32), device=eng.device, generator=g)
    got31 = eng.c3d2_conv31(a2s, t31)
    os.environ["SVK_C3D2_STATIC_ITEMS"] = "1"
    try:
        fixed2, fixed31 = eng.c3d2_stage2(act1, t2), eng.c3d2_conv31(a2s, t31)
    finally:
        del os.environ["SVK_C3D2_STATIC_ITEMS"]
    assert torch.equal(fixed2, w2) and torch.equal(fixed31, got31)
    pick = [0, 100, 201, 255]
    want2 = _cpu_layers(state, act1[pick].permute(0, 4, 1, 2, 3).cpu().contiguous(), BLOCK2)
    g4 = w2[pick].permute(0, 4, 1, 2, 3).cpu().numpy()
    print("second block, 256 cubes vs torch-CPU: max |diff| / scale %.2e" % (np.abs(g4 - want2).max() / np.abs(want2).max()))
    np.testing.assert_allclose(g4, want2, rtol=1e-4, atol=4e-6 * np.abs(want2).max())
    del act1, w2
    # conv3_1: 200 cubes = 1 000 items over 768 workgroups
    pick = [0, 77, 150, 199]
    want31 = _cpu_layers(state, a2s[pick].permute(0, 4, 1, 2, 3).cpu().contiguous(), (("3_1", (1, 1, 1)),), pool=False)
    np.testing.assert_allclose(_conv31_unchunk(got31[pick].cpu().numpy()), want31, rtol=1e-4, atol=4e-6 * np.abs(want31).max())
    # the whole chain on 300 cubes (19 groups of 16, the last partial) against the torch-CPU network, sampled
    cubes300 = torch.randn((300, 1, 20, 80, 40), device=eng.device, generator=g) * 2 - 6
    e300 = emb(cubes300)
    pick = [0, 15, 16, 143, 288, 299]
    want_e = model_ref.c3d2_embed(state, cubes300[pick].cpu().numpy()).numpy()
    np.testing.assert_allclose(e300[pick].cpu().numpy(), want_e, rtol=0, atol=1e-5 * np.abs(want_e).max())


def _bench_line(args, timeout=900):
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    proc = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + list(args), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert proc.returncode == 0, proc.stderr.decode()[-2000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_two_ranks_share_one_gpu(tmp_path):
    """The N > 1 path on the device: `bench.py --gpus 2 --backend gloo` starts two rank processes on this one GPU
    (RCCL refuses two ranks on a device, so the all-gather goes through gloo / host memory; everything else is the
    code the 8-GPU run executes): contiguous shards, padded gather, every rank scores, rank 0 reports.  The sharded
    run must report two ranks and give the SAME scores-derived numbers as the one-rank run, and --dump-outputs must
    hand back the same arrays from both."""
    common = ["--corpus", "5001", "--micro-batch", "1024", "--steps", "1", "--warmup", "1", "--full", "--no-extras"]
    two = _bench_line(["--gpus", "2", "--backend", "gloo", "--dump-outputs", str(tmp_path / "two")] + common)
    one = _bench_line(["--dump-outputs", str(tmp_path / "one")] + common)
    for name, shape in (("embeddings", (5001, 128)), ("scores", (4874, 40))):
        got_one, got_two = np.load(tmp_path / "one" / (name + ".npy")), np.load(tmp_path / "two" / (name + ".npy"))
        assert got_one.shape == shape and got_one.dtype == np.float32 and np.isfinite(got_one).all(), name
        assert np.array_equal(got_one, got_two), name
    assert two["ranks_seen"] == 2 and two["n_gpus"] == 2 and two["backend"] == "gloo" and two["scaling"] == "strong"
    assert two["config"]["corpus_clips"] == one["config"]["corpus_clips"] == 5001
    assert two["config"]["clips_per_rank"] == 2501 and one["config"]["clips_per_rank"] == 5001
    assert two["allgather_us"] > 0 and one["allgather_us"] is None
    assert len(two["per_rank_ms"]) == 2 and two["slowest_rank"] in (0, 1) and two["fastest_rank"] in (0, 1)
    # every clip's embedding depends on the clip alone (crops keyed by the global index, deterministic kernels): the
    # sharded run scores the SAME embeddings, so the EER is the same number, not a close one
    assert two["eer"]["eer"] == one["eer"]["eer"] and two["eer"]["auc"] == one["eer"]["auc"]
    assert two["eer"]["pairs"] == one["eer"]["pairs"] == 4874 * 40
    assert two["eer"]["eer"] == pytest.approx(two["eer"]["eer_device"], abs=1e-9)
    # the committed checkpoint gives an operating point, not a coin flip
    assert one["eer"]["eer"] < 0.1 and one["eer"]["auc"] > 0.95 and one["weights"]["weights"].endswith("c3d2_synth.pt")
    # the line's contract (task prompt / DESIGN section 6)
    for rec in (one, two):
        assert rec["metric"].startswith("utterances/sec") and rec["unit"] == "utterances/s" and rec["higher_is_better"] is True
        assert rec["steps"] == 1 and rec["warmup"] == 1 and rec["vs_baseline"] is None and rec["dtype"].startswith("f32")
        assert rec["value"] == pytest.approx(5001 / (rec["ms_per_step"] * 1e-3), rel=1e-6)
        assert "synthetic" in rec["data"] and "5001-clip corpus" in rec["config"]["workload"]
        roof = rec["roofline"]
        assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == pytest.approx(16 * 157.3) and "f16" in roof["pipe"]
        # frac = issued MFMA work / time / peak: a utilisation, never above 1; algorithmic_frac (SURVEY 8(d)'s direct-form
        # multiply-adds) may pass it -- and 1 -- where the depth transform issues 2/3 of the products
        assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"]) and 0.05 < roof["frac"] < 1.0
        assert roof["algorithmic_frac"] > roof["frac"] and roof["mfma_per_cube"] == pytest.approx(36 * (200 + 36 * 41), rel=1e-3)
        assert "c3d2_stage1h_kernel" in roof["kernel"] and roof["avg_launch_ms"] > 0
        # the counters behind frac are tied to the kernel sources they were collected from
        assert set(roof["this_run"]) == {"csrc_sha", "libsvk_sha"} and roof["stale"] in (True, False, None)
        if roof["stale"] is False:
            assert roof["counters_from"]["csrc_sha"] == roof["this_run"]["csrc_sha"]
        net = rec["roofline_network"]
        assert set(net) >= {"stage1", "stage2", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "fc5"}
        for name, row in net.items():
            if not name.startswith("_"):
                # (no lower bound worth the name: two processes time-slice ONE device here, and a short kernel whose events straddle a
                # switch to the other process reads a hundred times its duration -- 0.0077 seen for conv3_2)
                assert 0.0 < row["frac"] < 1.0 and row["mfma_per_cube"] == pytest.approx(row["mfma_per_cube_by_construction"], rel=1e-3), name
                # MFMA + the vector instructions that cannot overlap it: still a share of the SIMDs' FP32 issue slots
                assert row["fp32_lanes_busy"] is None or row["frac"] < row["fp32_lanes_busy"] < 1.0, name
        # issued per utterance: conv1_1 .. conv4_1: 60 336 + 40 068 + 5 400 + 12 600 + 4 752 f16 MFMAs of 16 384 FLOP; conv4_2, FC5: 8 640 f32 MFMAs of 2 048
        assert rec["roofline_e2e"]["frac"] < 1.0 and rec["roofline_e2e"]["issued_gflop_per_utt"] == pytest.approx(2.035483, rel=1e-3)
        assert rec["roofline_frontend"]["bound"] == "hbm" and rec["roofline_e2e"]["bound"] == "mfma"


def test_bench_plain_run_is_the_headline(tmp_path):
    """Without --full the bench times the same steps and hands back the same arrays, but its line carries the headline and
    the configuration only: no EER, no roofline rows, none of the side benches or the CPU-oracle leg."""
    common = ["--corpus", "5001", "--micro-batch", "1024", "--steps", "1", "--warmup", "1"]
    plain = _bench_line(["--dump-outputs", str(tmp_path / "plain")] + common)
    full = _bench_line(["--dump-outputs", str(tmp_path / "full"), "--full", "--no-extras"] + common)
    for name in ("embeddings", "scores"):
        assert np.array_equal(np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))), name
    assert plain["metric"] == full["metric"] and plain["unit"] == full["unit"] and plain["dtype"] == full["dtype"]
    assert plain["higher_is_better"] is True and plain["value"] == pytest.approx(5001 / (plain["ms_per_step"] * 1e-3), rel=1e-6)
    assert plain["config"] == full["config"] and plain["steps"] == 1 and plain["warmup"] == 1
    moved = {"eer", "roofline", "roofline_frontend", "roofline_stage2", "roofline_network", "roofline_e2e", "scaling_efficiency_vs",
             "rccl_expectation_us", "parity", "cpu_baseline"}
    assert not moved & set(plain) and moved - {"parity", "cpu_baseline"} <= set(full)
    assert set(plain) == set(full) - moved


def test_bench_four_ranks_uneven_shards_on_one_gpu():
    """BASELINE config 5's shape in small: 20 003 clips over FOUR ranks (shards of 5 001, 5 001, 5 001, 5 000: the last one
    short, the gather padded) on this one GPU through gloo -- the same embeddings, hence the same EER / AUC to the last
    digit, as one rank over the whole corpus."""
    common = ["--corpus", "20003", "--micro-batch", "2048", "--steps", "1", "--warmup", "0", "--full", "--no-extras"]
    four = _bench_line(["--gpus", "4", "--backend", "gloo"] + common, timeout=1200)
    one = _bench_line(common)
    assert four["ranks_seen"] == 4 and four["n_gpus"] == 4 and four["config"]["clips_per_rank"] == 5001
    assert len(four["per_rank_ms"]) == 4 and four["allgather_bytes_per_rank"] == 5001 * 128 * 4
    assert four["eer"]["eer"] == one["eer"]["eer"] and four["eer"]["auc"] == one["eer"]["auc"]
    assert four["eer"]["short_clips"] == one["eer"]["short_clips"]
    assert four["value"] == pytest.approx(20003 / (four["ms_per_step"] * 1e-3), rel=1e-6)


def test_bench_under_torch_distributed_run():
    """The launch form the driver uses for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr
    127.0.0.1 --master-port P bench.py --gpus 2 ...` -- this process is then ONE rank (RANK / LOCAL_RANK / WORLD_SIZE from the
    environment, no self-launch); here with `--backend gloo` so that both ranks can share this one GPU.  One JSON line from
    rank 0, the same numbers as the self-launched run."""
    import json
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    common = ["--corpus", "5001", "--micro-batch", "1024", "--steps", "1", "--warmup", "0", "--full", "--no-extras"]
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                           "127.0.0.1", "--master-port", str(port), os.path.join(repo, "bench.py"), "--gpus", "2", "--backend", "gloo"]
                          + common, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert proc.returncode == 0, proc.stderr.decode()[-2000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, proc.stdout.decode()[-2000:]
    rec = json.loads(lines[0])
    assert rec["ranks_seen"] == 2 and rec["n_gpus"] == 2 and rec["config"]["clips_per_rank"] == 2501
    one = _bench_line(common)
    assert rec["eer"]["eer"] == one["eer"]["eer"] and rec["eer"]["auc"] == one["eer"]["auc"]


def test_bench_parity_leg_at_the_trained_operating_point():
    """bench.py's CPU-oracle leg (cpu_baseline + parity) on the first 492 clips (four speakers) of a 5 001-clip corpus with
    the committed trained checkpoint: the production path's embeddings against the oracle's from the same PCM, and the EER
    on both sides -- equal, at an operating point where the ROC is steep (not the diagonal of a random-init network)."""
    rec = _bench_line(["--corpus", "5001", "--micro-batch", "1024", "--steps", "1", "--warmup", "0", "--full", "--parity-only",
                       "--cpu-sample", "492"], timeout=1200)
    par, base = rec["parity"], rec["cpu_baseline"]
    assert par["sample_clips"] == 492 and par["embed_max_abs_diff"] <= 5e-5 * par["embed_scale"]
    assert par["score_max_abs_diff"] <= 2e-5
    assert par["eer_equal"] and par["eer_gpu"] == par["eer_cpu_ref"] and par["eer_gpu"] < 0.2
    assert par["full_matrix_score_max_abs_diff"] <= 1e-5 and rec["eer"]["eer"] == pytest.approx(par["full_matrix_eer_cpu_ref"], abs=1e-9)
    assert rec["eer"]["eer"] < 0.1
    # the baseline's harness: chain and pair-by-pair scoring timed separately, every worker warmed before the clock starts
    assert base["kind"] == "port" and base["unit"] == "utterances/s" and base["value"] > 0 and base["cores"] >= 1
    for row in base["chain_by_workers"].values():
        assert row["chain_utt_per_s"] >= row["utt_per_s"] > 0 and row["scoring_s"] >= 0 and row["warm_s"] > 0
    assert "host_fed" not in rec and "ragged" not in rec                    # --parity-only: none of the side benches


def test_network_block_error_paths(eng):
    """The libsvk network blocks refuse what they were not built for, loudly (no silent fallback inside the library)."""
    from speaker_verification_amd import _lib
    model, emb, state = _net(eng, 5, 6)
    tables = emb.stage1_tables()
    feat = torch.zeros((2, 100, 39), device=eng.device)                      # 39 coefficients: not the 20 x 80 x 40 cube
    with pytest.raises(_lib.SvkError, match="20 x 80 x 40"):
        eng.c3d2_stage1(feat, torch.zeros((2, 20), dtype=torch.int32, device=eng.device), tables)
    feat = torch.zeros((2, 100, 40), device=eng.device)
    with pytest.raises(_lib.SvkError, match="20 x 80 x 40"):
        eng.c3d2_stage1(feat, torch.zeros((2, 19), dtype=torch.int32, device=eng.device), tables)
    assert eng.lib.svk_c3d2_stage1(eng.ctx, None, 1, 100, 40, None, 20, 80, None, None, None, None, None, None, 0, None) == -1
    assert eng.lib.svk_c3d2_stage2(eng.ctx, None, 1, None, None, None, None, None, None, 0, None, None) == -1
    # flag bits other than bit 1 (slopes in [0, 1]) named kernel forms that no longer exist: refused
    for bad_flags in (1, 4, 8, 16):
        assert eng.lib.svk_c3d2_stage1(eng.ctx, None, 1, 100, 40, None, 20, 80, None, None, None, None, None, None, bad_flags, None) == -1
        assert eng.lib.svk_c3d2_stage2(eng.ctx, None, 1, None, None, None, None, None, None, bad_flags, None, None) == -1
        assert eng.lib.svk_c3d2_conv31(eng.ctx, None, 1, None, None, None, bad_flags, None) == -1
    assert eng.lib.svk_c3d2_stage1_lds_bytes() <= eng.lds_per_cu
    # empty batch: nothing launched, nothing touched
    assert eng.lib.svk_c3d2_stage1(eng.ctx, None, 0, 100, 40, None, 20, 80, None, None, None, None, None, None, 0, None) == 0
    with pytest.raises(ValueError):
        eng.c3d2_stage2(torch.zeros((2, 16, 18, 18, 32), device=eng.device), emb.stage2_tables())
    # all-(-1) crops (every clip too short): an all-bias activation, finite, identical for every cube
    y = eng.c3d2_stage1(torch.randn((3, 90, 40), device=eng.device), torch.full((3, 20), -1, dtype=torch.int32,
                                                                              device=eng.device), tables)
    assert bool(torch.isfinite(y).all()) and torch.equal(y[0], y[1]) and torch.equal(y[1], y[2])
    # crop starts the C-ABI cannot trust: INT32_MAX (start + row would wrap negative), INT32_MAX - 79, max_frames, INT32_MIN
    # -- all read as "no frames" (zero rows), never out of bounds
    featr = torch.randn((3, 90, 40), device=eng.device)
    for wild in (2**31 - 1, 2**31 - 80, 90, -2**31):
        bad = torch.full((3, 20), -1, dtype=torch.int32, device=eng.device)
        bad[1] = wild
        yb = eng.c3d2_stage1(featr, bad, tables)
        torch.cuda.synchronize()
        assert torch.equal(yb[1], yb[0]), wild
    # crops that run off the END of the clip (start + 80 > max_frames): the rows past it read as zeros -- bit for bit what the
    # same crops give on the features padded with zero rows, where every patch piece takes the kernel's fast path (LDS-DMA);
    # starts 50 / 60 cut a 32-row piece in the middle, 89 leaves one row
    part = torch.randint(0, 11, (3, 20), device=eng.device, dtype=torch.int32, generator=torch.Generator(device=eng.device).manual_seed(5))
    part[1, ::3] = 50
    part[1, 1] = 60
    part[2, 5] = 89
    part[0, 19] = 11
    featp = torch.zeros((3, 170, 40), device=eng.device)
    featp[:, :90] = featr
    assert torch.equal(eng.c3d2_stage1(featr, part, tables), eng.c3d2_stage1(featp, part, tables))
