#!/usr/bin/env python3
"""Generate tests/golden/c3d2_3c.npz -- the three-channel model (constants.DERIVATIVE = True) -- by IMPORTING THE REFERENCE,
with the import recipe of tools/make_golden.py (whose helpers it uses; that file is left as it is).

Run from the repo root:  python tools/make_golden_c3d2_3c.py
Stored: seeds, the reference's C3D2(1211, 3) state sums, its embeddings / softmax rows / speaker model for the N(-6, 2) cubes
of c3d2_embed.npz (three channels here), and the reference's CMVN (DERIVATIVE and NORMALIZE on) + FeatureCube3C output for a
fixed feature matrix and NumPy seed, with the crop starts.  Nothing of the reference's code is copied.
"""
import io
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference and the repo)
from speaker_verification_amd.model import perturb_inference_state  # noqa: E402


def main():
    _, _, ref_utils, _, ref_model = mg._import_reference_app_modules()
    # utils.py:6 imports the package only; its CMVN reaches speechpy.feature / .processing as attributes
    import importlib
    for sub in ("feature", "processing"):
        importlib.import_module("speech_feature_extraction.speechpy." + sub)
    g = {"versions": mg.versions()}
    sink = io.StringIO()
    real_stdout, sys.stdout = sys.stdout, sink                      # C3D2.__init__ prints
    try:
        torch.manual_seed(2024)
        net = ref_model.C3D2(1211, 3)
    finally:
        sys.stdout = real_stdout
    state = perturb_inference_state(net.state_dict(), seed=99)
    net.load_state_dict(state)
    net.eval()
    g["init_seed"], g["perturb_seed"], g["n_labels"] = np.array([2024]), np.array([99]), np.array([1211])
    names = sorted(state.keys())
    g["state_names"] = np.array(names)
    g["state_abs_sums"] = np.array([float(state[k].double().abs().sum()) for k in names])
    cube_rng = np.random.default_rng(31)
    cubes = (cube_rng.standard_normal((3, 3, 20, 80, 40)) * 2.0 - 6.0).astype(np.float32)
    g["cube_seed"] = np.array([31])
    with torch.no_grad():
        g["embed"] = net(torch.from_numpy(cubes), development=False).numpy()
        g["softmax"] = net(torch.from_numpy(cubes), development=True).numpy()
        g["speaker_model"] = net.create_Speaker_Model(torch.from_numpy(cubes[1:2])).numpy()

    # CMVN (utils.py:382-397, DERIVATIVE and NORMALIZE on) -> FeatureCube3C (utils.py:325-348) with the global NumPy RNG
    feat = np.random.default_rng(33).standard_normal((120, 40)) * 3.0 + 1.0
    saved = ref_utils.c.DERIVATIVE, ref_utils.c.NORMALIZE
    ref_utils.c.DERIVATIVE, ref_utils.c.NORMALIZE = True, True
    try:
        sample = ref_utils.CMVN()({"feature": feat.copy(), "label": 5})
    finally:
        ref_utils.c.DERIVATIVE, ref_utils.c.NORMALIZE = saved
    g["cmvn_feat_seed"] = np.array([33])
    g["cmvn_out"] = np.asarray(sample["feature"])                       # (120, 40, 3)
    np.random.seed(778)
    out = ref_utils.FeatureCube3C((80, 40, 20, 3))(sample)
    g["cube_np_seed"] = np.array([778])
    g["cube_out"] = out["feature"]                                      # (3, 20, 80, 40)
    np.random.seed(778)
    g["cube_idx"] = np.random.randint(120 - 80, size=20)
    np.savez_compressed(os.path.join(mg.OUT, "c3d2_3c.npz"), **g)
    print("c3d2_3c.npz", sum(v.nbytes for v in g.values()) // 1024, "KiB raw")


if __name__ == "__main__":
    main()
