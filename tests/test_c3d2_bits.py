"""The bits of the seven C3D2 network kernels, pinned for refactors: the SHA-256 of every kernel's output bytes on one seeded
input against tests/golden/c3d2_bits.json.

The golden pins ONE compiler and ONE architecture (hipcc of the ROCm release the digests were recorded with, gfx950): a change
that leaves the source's arithmetic and its order alone leaves these digests alone, and a deliberate change of the arithmetic
order (another accumulation order, another split, another PReLU form) or a compiler that contracts or reorders differently must
re-record the file -- run this module once on the commit BEFORE such a change with SVK_C3D2_BITS_RECORD=1 to see that it
reproduces the committed file, and once after it to write the new one.  What the numbers should be is the business of
tests/test_c3d2_float64.py; this file only says they are still the same.

Input: 600 cubes, the smallest round number at which every persistent kernel gives some workgroup a third item on a 256-CU
card (conv4_1: one item per cube, one workgroup per CU, its ticket drawn two grids ahead), so every kernel's whole item pipeline
runs.  On a card with another CU count the items fall to other workgroups; the outputs, and the digests compared, are the same.
Feature rows [600, 120, 40] (and [600, 3, 120, 40] for the three-channel first block) with crop starts in [0, 40]; two cubes
carry one start each outside the clip (-5, and max_frames - 10): zero rows by the C-ABI, and the only way into
patch_piece_issue's lane-by-lane branch, which no pipeline input reaches.  The shipped checkpoint's tables (its conv1_1 weight
times 1, 1/2, -1/4 as the three channels' -- exact scalings) run the chain stage1 -> stage2 -> conv3_1 -> conv3_2 -> conv4_1 ->
conv4_2 -> FC5 with the slope flag set and clear, work items from the device-wide counters and at a fixed stride
(SVK_C3D2_STATIC_ITEMS): four runs, one digest per kernel and flag, the same for both item assignments."""
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3d2_bits.json")
RECORD = bool(os.environ.get("SVK_C3D2_BITS_RECORD"))
N, T = 600, 120
CHAIN = ("stage2", "conv31", "conv32t", "conv41", "conv42", "fc5")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def tables(eng):
    """kernel -> the shipped checkpoint's operand tables, + "stage1_c3"."""
    import copy
    from speaker_verification_amd import model as M
    fe = copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()
    out = {k: getattr(fe, k + "_tables")() for k in R.KERNELS}
    (w1, b1, s1, *_), st2 = fe.stages[0], fe.stages[1]
    out["stage1_c3"] = M._stage1_tables((torch.cat([w1, 0.5 * w1, -0.25 * w1], 1), b1, s1), st2)
    for k, t in out.items():
        assert k == "fc5" or t[-1] is True, "%s: the shipped slopes lie in [0, 1], so either PReLU form may run" % k
    return out


@pytest.fixture(scope="module")
def inputs(eng):
    rng = np.random.default_rng(20261017)
    feat3 = (rng.standard_normal((N, 3, T, 40)) * 2.0 - 6.0).astype(np.float32)
    crops = rng.integers(0, 41, (N, 20)).astype(np.int32)
    crops[17, 3] = -5
    crops[401, 11] = T - 10
    feat3, crops = torch.from_numpy(feat3).to(eng.device), torch.from_numpy(crops).to(eng.device)
    return feat3[:, 0].contiguous(), feat3, crops


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _digests(eng, tables, inputs, slope01):
    feat, feat3, crops = inputs

    def tab(k):
        return tables[k] if k == "fc5" else tuple(tables[k][:-1]) + (slope01,)

    out = {"stage1_c3": _sha(eng.c3d2_stage1(feat3, crops, tab("stage1_c3")))}
    y = eng.c3d2_stage1(feat, crops, tab("stage1"))
    out["stage1"] = _sha(y)
    for k in CHAIN:
        y = getattr(eng, "c3d2_" + k)(y, tab(k))
        out[k] = _sha(y)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flag,static", [("slope01", False), ("slope01", True), ("any", False), ("any", True)],
                         ids=["slope01-queued", "slope01-static", "any-queued", "any-static"])
def test_output_bits_are_the_recorded_ones(eng, tables, inputs, monkeypatch, flag, static):
    """Every kernel's output bytes hash to the recorded digest: slope flag set (`slope01`) and clear (`any`), items from the
    device-wide counters (`queued`) and at a fixed stride (`static`) -- the static run is held to the queued run's digest."""
    if static:
        monkeypatch.setenv("SVK_C3D2_STATIC_ITEMS", "1")
    else:
        monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)
    got = _digests(eng, tables, inputs, flag == "slope01")
    if RECORD and not static:
        gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        gold.setdefault("digests", {})[flag] = got
        gold["input"] = "%d cubes, feature rows [%d, 40] / [3, %d, 40], crop starts in [0, 40] and -5, %d" % (N, T, T, T - 10)
        gold["hip_runtime"] = torch.version.hip
        gold["arch"] = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
        with open(GOLDEN, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")
    want = json.load(open(GOLDEN))["digests"][flag]
    assert set(want) == set(got) == set(R.KERNELS) | {"stage1_c3"}
    wrong = sorted(k for k in got if got[k] != want[k])
    assert not wrong, "%s, %s items: other bits than recorded from %s" % (flag, "static" if static else "queued", wrong)
