"""The three-channel C3D2 (constants.DERIVATIVE = True: static, delta and delta-delta features, utils.FeatureCube3C) on the
libsvk kernels: the first block `svk_c3d2_stage1_c3`, its tables, the model / FusedEmbedder routing and the batched
`evaluation.dataset_embeddings`.  Reference outputs: tests/golden/c3d2_3c.npz (tools/make_golden_c3d2_3c.py)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import model_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3d2_3c.npz")
BLOCK1 = (("1_1", (1, 1, 1)), ("1_2", (1, 2, 1)))


@pytest.fixture(scope="module")
def g3():
    return np.load(GOLDEN, allow_pickle=False)


def _golden_model(g):
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    model = seeded_model(int(g["init_seed"][0]), int(g["n_labels"][0]), 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), int(g["perturb_seed"][0])))
    return model.eval()


def _golden_cubes(g):
    return (np.random.default_rng(int(g["cube_seed"][0])).standard_normal((3, 3, 20, 80, 40)) * 2.0 - 6.0).astype(np.float32)


def _cpu_block1(state, x):
    """conv1_1 -> BN (eval, unfolded) -> PReLU -> conv1_2 -> BN -> PReLU -> pool1 on torch-CPU f32 (model.py:141-150)."""
    import torch.nn.functional as F
    with torch.no_grad():
        for tag, stride in BLOCK1:
            x = F.conv3d(x, state[f"conv{tag}.weight"], state[f"conv{tag}.bias"], stride=stride)
            x = F.batch_norm(x, state[f"batch_norm{tag}.running_mean"], state[f"batch_norm{tag}.running_var"],
                             state[f"batch_norm{tag}.weight"], state[f"batch_norm{tag}.bias"], training=False, eps=1e-5)
            x = F.prelu(x, state[f"PReLu{tag}.weight"])
        return F.max_pool3d(x, kernel_size=(1, 1, 2), stride=(1, 1, 2)).numpy()


def _cubes_from_rows(feat3, crops):
    """[n, 3, T, 40] rows + [n, 20] starts -> (n, 3, 20, 80, 40); a crop whose 80 rows are not all inside the clip is zero
    rows past the clip's end (a start outside [0, T) is all zero), as svk_c3d2_stage1 documents."""
    n, _, T, C = feat3.shape
    out = np.zeros((n, 3, 20, 80, C), dtype=np.float32)
    for u in range(n):
        for k, s in enumerate(crops[u]):
            if 0 <= s < T:
                rows = feat3[u, :, s:s + 80]
                out[u, :, k, :rows.shape[1]] = rows
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_three_channel_tables_on_cpu(g3):
    """FusedEmbedder builds a three-channel model's tables on the host: conv1_1's [3][2][64][8] blocks are the BN-folded,
    scale-fixed weights split into H + L (to 2^-22 of each weight, 2^-25 absolute), with each channel's 16th tap a zero pad.
    (Before the three-channel first block this raised ValueError.)"""
    from speaker_verification_amd.model import FusedEmbedder
    emb = FusedEmbedder(_golden_model(g3))
    assert emb.num_channels == 3
    w1blk = emb.stage1_tables()[0]
    assert tuple(w1blk.shape) == (3, 2, 64, 8) and w1blk.dtype == torch.float16
    w1 = emb.stages[0][0].double()                                   # [16 co][3 ch][3][1][5], folded and scale-fixed
    blk = w1blk.double()
    lane = np.arange(64)
    co, kk = lane & 15, lane >> 4
    taps = np.zeros((3, 16, 48), dtype=np.float64)                   # the 45 taps padded to 48 (16 per channel)
    for ch in range(3):
        for ln in range(64):
            for e in range(8):
                t = 8 * (kk[ln] & 1) + e
                h, lo = float(blk[ch, 0, ln, e]), float(blk[ch, 1, ln, e])
                if kk[ln] < 2:
                    taps[ch, co[ln], 16 * ch + t] = h + lo
                else:                                                # the l half of the fragment: H again, no L
                    assert h == float(blk[ch, 0, ln - 32, e]) and lo == 0.0
    want = np.zeros((16, 48))
    for ch in range(3):
        want[:, 16 * ch:16 * ch + 15] = w1[:, ch].reshape(16, 15).numpy()
    got = taps.sum(0)
    assert not got[:, 15::16].any()                                  # the pads
    # 2^-22 of the weight; an L piece below the smallest normal half is rounded to a multiple of 2^-24 (the 2^-25 floor)
    np.testing.assert_allclose(got, want, rtol=2.0 ** -22, atol=2.0 ** -25)
    # conv1_2's blocks are the one-channel layout
    assert tuple(emb.stage1_tables()[3].shape) == (14, 2, 64, 8)


def test_three_channel_state_and_oracle(g3):
    """The seeded, perturbed three-channel model is the reference's (state sums), and the CPU oracle embeds the golden cubes
    as the reference did: the oracle is pinned for three channels."""
    model = _golden_model(g3)
    state = model.state_dict()
    names = [str(k) for k in g3["state_names"]]
    assert sorted(state.keys()) == names
    np.testing.assert_allclose([float(state[k].double().abs().sum()) for k in names], g3["state_abs_sums"], rtol=1e-12)
    got = model_ref.c3d2_embed({k: v.detach() for k, v in state.items()}, torch.from_numpy(_golden_cubes(g3))).numpy()
    scale = np.abs(g3["embed"]).max()
    np.testing.assert_allclose(got, g3["embed"], rtol=0, atol=1e-6 * scale)


def test_three_channel_routing_on_cpu():
    """Host tensors and training mode stay on the torch layers; other channel counts never reach the kernels."""
    from speaker_verification_amd.model import C3D2
    m = C3D2(8, 3).eval()
    m.three_channel_kernels = True
    assert not m.runs_on_kernels(torch.zeros((1, 3, 20, 80, 40)))        # host tensor
    with pytest.raises(ValueError):
        from speaker_verification_amd.model import FusedEmbedder
        FusedEmbedder(C3D2(8, 2))


# ---- GPU ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.mark.gpu
def test_three_channel_reference_parity(eng, g3):
    """model(cube3, development=False) with `three_channel_kernels` runs the kernels and matches the reference's embeddings;
    softmax rows and create_Speaker_Model follow."""
    model = _golden_model(g3).to(eng.device)
    model.three_channel_kernels = True
    x = torch.from_numpy(_golden_cubes(g3)).to(eng.device)
    assert model.runs_on_kernels(x)
    with torch.no_grad():
        emb = model(x, development=False)
        probs = model(x)
    scale = np.abs(g3["embed"]).max()
    print("three-channel golden embeddings: max |diff| / scale %.2e" % (np.abs(emb.cpu().numpy() - g3["embed"]).max() / scale))
    np.testing.assert_allclose(emb.cpu().numpy(), g3["embed"], rtol=0, atol=5e-5 * scale)
    with torch.no_grad():
        want = torch.softmax(model.FC6(model.PReLu5(emb)), dim=1)
    torch.testing.assert_close(probs, want, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(probs.cpu().numpy(), g3["softmax"], rtol=1e-3, atol=1e-7)
    sm = model.create_Speaker_Model(x[1:2])
    assert torch.equal(sm, emb[1:2])
    np.testing.assert_allclose(sm.detach().cpu().numpy(), g3["speaker_model"], rtol=0, atol=5e-5 * scale)


def _three_channel_feats(eng, n, seconds_min=1.2):
    """Real CMVN'd static / delta / delta-delta log-mel features of synthetic clips: [n, 3, T, 40] (ragged rows zero)."""
    from speaker_verification_amd import constants as c, synth
    from speaker_verification_amd.speechpy import feature, processing
    feats = []
    for k in range(n):
        clip = synth.speaker_clip(k % 3 + 1, k, int(16000 * (seconds_min + 0.31 * k)))
        f = feature.lmfe(clip / 32768.0, 16000, c.FRAME_LEN, c.FRAME_STEP, c.NUM_COEF, c.NUM_FFT)
        f3 = np.asarray(feature.extract_derivative_feature(f), dtype=np.float64)
        for ch in range(3):
            f3[:, :, ch] = processing.cmvn(f3[:, :, ch], variance_normalization=True)
        feats.append(f3.transpose(2, 0, 1))
    T = max(f.shape[1] for f in feats)
    out = np.zeros((n, 3, T, 40), dtype=np.float32)
    for k, f in enumerate(feats):
        out[k, :, :f.shape[1]] = f
    return out, [f.shape[1] for f in feats]


@pytest.mark.gpu
def test_three_channel_first_block_against_f32(eng, g3):
    """svk_c3d2_stage1_c3 against torch-CPU f32 of conv1_1 -> conv1_2 -> pool1 with unfolded BatchNorm at the per-layer bar of
    the one-channel kernel: the golden N(-6, 2) cubes, and real CMVN'd static / delta / delta-delta features (small delta
    values: the half pairs' 2^-25 floor in play), with crop starts outside the clip (zero rows)."""
    model = _golden_model(g3).to(eng.device)
    emb = model.fused_inference()
    tables = emb.stage1_tables()
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    # (a) the golden cubes, as feature rows with crop starts 0, 80, ...
    cubes = _golden_cubes(g3)
    rows = eng.to_device(cubes).view(3, 3, 1600, 40)
    got = eng.c3d2_stage1(rows, emb.crop_starts(3, eng.device), tables).cpu().numpy()
    want = _cpu_block1(state, torch.from_numpy(cubes))
    scale = np.abs(want).max()
    print("three-channel first block (N(-6, 2) cubes): max |diff| / scale %.2e" % (np.abs(got.transpose(0, 4, 1, 2, 3) - want).max() / scale))
    np.testing.assert_allclose(got.transpose(0, 4, 1, 2, 3), want, rtol=1e-4, atol=4e-6 * scale)
    # (b) real features; T not a multiple of 80; starts past the end and negative
    feat3, frames = _three_channel_feats(eng, 5)
    assert any(t % 80 for t in frames)
    rng = np.random.default_rng(5)
    crops = np.stack([rng.integers(0, t - 80, size=20) for t in frames]).astype(np.int32)
    crops[1, 3] = -1
    crops[2, 7] = feat3.shape[2] + 5
    crops[3, 0] = -(2 ** 31)
    crops[4, 19] = frames[4] - 40                           # half inside the clip: the rest are the zero padding rows
    cubes = _cubes_from_rows(feat3, crops)
    want = _cpu_block1(state, torch.from_numpy(cubes))
    got = eng.c3d2_stage1(feat3, crops, tables).cpu().numpy()
    scale = np.abs(want).max()
    print("three-channel first block (CMVN'd features): max |diff| / scale %.2e" % (np.abs(got.transpose(0, 4, 1, 2, 3) - want).max() / scale))
    np.testing.assert_allclose(got.transpose(0, 4, 1, 2, 3), want, rtol=1e-4, atol=4e-6 * scale)


@pytest.mark.gpu
def test_three_channel_layouts_and_bad_arguments(eng, g3):
    """The per-call cube route and the feature-row route with explicit starts give identical embeddings; bad arguments are
    error codes, not faults."""
    model = _golden_model(g3).to(eng.device)
    emb = model.fused_inference()
    cubes = _golden_cubes(g3)
    x = torch.from_numpy(cubes).to(eng.device)
    via_cube = emb(x)
    starts = np.tile((np.arange(20) * 80).astype(np.int32), (3, 1))
    via_rows = emb.embed_features(x.view(3, 3, 1600, 40), starts)
    assert torch.equal(via_cube, via_rows)
    with pytest.raises(ValueError):
        emb(torch.zeros((1, 1, 20, 80, 40), device=eng.device))          # a one-channel cube for a three-channel model
    with pytest.raises(ValueError):
        emb.embed_features(x.view(3, 4800, 40), starts)                    # rows without the channel axis
    bad = x.clone()
    bad[0, 2, 0, 0, 0] = float("inf")
    with pytest.raises(ValueError):
        emb(bad)
    lib, ctx = eng.lib, eng.ctx
    assert lib.svk_c3d2_stage1_c3(ctx, None, 1, 100, 40, None, 20, 80, None, None, None, None, None, None, 0, None) == -1
    assert lib.svk_c3d2_stage1_c3(ctx, None, 1, 100, 40, None, 20, 80, None, None, None, None, None, None, 4, None) == -1
    assert lib.svk_c3d2_stage1_c3(ctx, None, 1, 100, 13, None, 20, 80, None, None, None, None, None, None, 0, None) == -2
    assert lib.svk_c3d2_stage1_c3(ctx, None, -1, 100, 40, None, 20, 80, None, None, None, None, None, None, 0, None) == -1
    assert lib.svk_c3d2_stage1_c3(ctx, None, 0, 100, 40, None, 20, 80, None, None, None, None, None, None, 0, None) == 0
    assert lib.svk_c3d2_stage1_c3_lds_bytes() == lib.svk_c3d2_stage1_lds_bytes() <= eng.lds_per_cu
    with pytest.raises(ValueError):
        eng.c3d2_stage1(torch.zeros((2, 3, 100, 40), device=eng.device), np.zeros((1, 20), np.int32), emb.stage1_tables())
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_three_channel_large_launch_matches_batches_of_one(eng, g3):
    """2 100 cubes in one launch are bit-identical to the same cubes embedded one at a time, and deterministic."""
    model = _golden_model(g3).to(eng.device)
    emb = model.fused_inference()
    n, T = 2100, 97
    gen = torch.Generator(device=eng.device).manual_seed(7)
    feat = torch.randn((n, 3, T, 40), device=eng.device, generator=gen) * 2.0 - 1.0
    crops = torch.randint(0, T - 80, (n, 20), device=eng.device, generator=gen, dtype=torch.int32)
    big = emb.embed_features(feat, crops)
    assert torch.equal(big, emb.embed_features(feat, crops))
    one = torch.cat([emb.embed_features(feat[i:i + 1], crops[i:i + 1]) for i in range(n)])
    assert torch.equal(big, one)
    assert bool(torch.isfinite(big).all())


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True])
def test_three_channel_dataset_embeddings(eng, g3, tmp_path, monkeypatch, normalize):
    """evaluation.dataset_embeddings with DERIVATIVE = True (batched: ragged front end, two derivative launches, CMVN per
    channel, svk_c3d2_stage1_c3) against the per-item chain CMVN -> FeatureCube3C -> the torch layers under the same NumPy
    seed: the same crop draws, the same embeddings, the same RNG state after."""
    from speaker_verification_amd import constants as c, evaluation, load_data, synth, utils, vad
    monkeypatch.setattr(c, "DERIVATIVE", True)
    monkeypatch.setattr(c, "NORMALIZE", normalize)
    names = []
    for k in range(7):
        rel = "id1000%d/u%d.wav" % (k % 3, k)
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        vad.write_wave(str(tmp_path / rel), synth.speaker_clip(k % 3 + 1, k, 16000 + 5077 * k).tobytes(), 16000)
        names.append(rel)
    listing = tmp_path / "ids.txt"
    listing.write_text("\n".join(names) + "\n")
    labels = {"id10000": 0, "id10001": 1, "id10002": 2}
    model = _golden_model(g3).to(eng.device)
    ds = load_data.AudioDataset(str(listing), str(tmp_path), labels)
    np.random.seed(2718)
    got = evaluation.dataset_embeddings(ds, model, batch=3).cpu().numpy()
    after_batched = np.random.get_state()
    per_item = load_data.AudioDataset(str(listing), str(tmp_path), labels, transform=utils.Compose(
        [utils.CMVN(), utils.FeatureCube3C((80, 40, 20, 3)), utils.ToTensor()]))
    model.inference_kernels = False
    np.random.seed(2718)
    cubes = np.stack([per_item[i][0] for i in range(len(per_item))])
    with torch.no_grad():
        want = model(torch.from_numpy(cubes).to(eng.device), development=False).cpu().numpy()
    after_items = np.random.get_state()
    assert after_batched[0] == after_items[0] and np.array_equal(after_batched[1], after_items[1]) and after_batched[2:] == after_items[2:]
    scale = np.abs(want).max()
    print("dataset_embeddings (DERIVATIVE, NORMALIZE=%s): max |diff| / scale %.2e" % (normalize, np.abs(got - want).max() / scale))
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-5 * scale)


@pytest.mark.gpu
def test_three_channel_transforms_against_the_reference(eng, g3, monkeypatch):
    """utils.CMVN (DERIVATIVE and NORMALIZE on) + FeatureCube3C give the reference's cube under its seed."""
    from speaker_verification_amd import constants as c, utils
    monkeypatch.setattr(c, "DERIVATIVE", True)
    monkeypatch.setattr(c, "NORMALIZE", True)
    feat = np.random.default_rng(int(g3["cmvn_feat_seed"][0])).standard_normal((120, 40)) * 3.0 + 1.0
    stacked = utils.CMVN()({"feature": feat, "label": 5})["feature"]
    assert stacked.shape == (120, 40, 3)
    np.testing.assert_allclose(stacked, g3["cmvn_out"], rtol=1e-3, atol=1e-4)
    np.random.seed(int(g3["cube_np_seed"][0]))
    cube = utils.FeatureCube3C((80, 40, 20, 3))({"feature": g3["cmvn_out"], "label": 5})["feature"]
    np.testing.assert_array_equal(cube, g3["cube_out"])
    np.random.seed(int(g3["cube_np_seed"][0]))
    np.testing.assert_array_equal(np.random.randint(120 - 80, size=20), g3["cube_idx"])


@pytest.mark.gpu
def test_three_channel_forward_routing(eng, g3):
    """forward's routing: a three-channel model stays on the torch layers by default (as before this kernel existed) and runs
    svk_c3d2_stage1_c3 once `three_channel_kernels` is set, on the instance or the class; a cube whose channel count is not the
    model's, another channel count, a host tensor, training mode and `inference_kernels = False` stay on the torch layers."""
    from speaker_verification_amd.model import C3D2
    model = _golden_model(g3).to(eng.device)
    x = torch.from_numpy(_golden_cubes(g3)).to(eng.device)
    assert not model.runs_on_kernels(x)
    with torch.no_grad():
        torch_rows = model(x, development=False)
    model.three_channel_kernels = True
    assert model.runs_on_kernels(x)
    with torch.no_grad():
        kernel_rows = model(x, development=False)
    assert torch.equal(kernel_rows, model.fused_inference()(x))
    scale = float(torch_rows.abs().max())
    assert float((kernel_rows - torch_rows).abs().max()) <= 5e-5 * scale
    assert not model.runs_on_kernels(x.cpu())
    assert not model.runs_on_kernels(torch.zeros((1, 1, 20, 80, 40), device=eng.device))
    model.train()
    assert not model.runs_on_kernels(x)
    model.eval()
    model.inference_kernels = False
    assert not model.runs_on_kernels(x)
    del model.inference_kernels, model.three_channel_kernels
    assert not model.runs_on_kernels(x)
    C3D2.three_channel_kernels = True
    try:
        assert model.runs_on_kernels(x)
        assert not C3D2(4, 2).to(eng.device).eval().runs_on_kernels(torch.zeros((1, 2, 20, 80, 40), device=eng.device))
        assert C3D2(4, 1).to(eng.device).eval().runs_on_kernels(torch.zeros((1, 1, 20, 80, 40), device=eng.device))
    finally:
        C3D2.three_channel_kernels = False
