"""The C-ABI library builds, loads and exports exactly what include/svk.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    so = os.path.join(REPO, "speaker_verification_amd", "libsvk.so")
    if not os.path.exists(so):
        entry.build()
    from speaker_verification_amd import _lib
    return _lib.load()


def _header_code():
    """include/svk.h without its comments"""
    text = open(os.path.join(REPO, "include", "svk.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_and_binding_agree(lib):
    """The one header <-> binding table <-> library walk: every entry point is declared once in include/svk.h, bound in
    _lib.SIGNATURES with the declaration's parameter count, exported by the built library and typed on the loaded one."""
    from speaker_verification_amd import _lib
    assert os.listdir(os.path.join(REPO, "include")) == ["svk.h"]          # one header: a second one is a second boundary
    code = _header_code()
    declared = sorted(set(re.findall(r"\b(svk_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_lib.SIGNATURES) and len(declared) == 97
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        decls = re.findall(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert len(decls) == 1, name                                        # exactly one declaration `name ( ... ) ;`
        params = decls[0].strip()
        assert (0 if params in ("", "void") else len(params.split(","))) == len(argtypes), name
        assert getattr(raw, name) is not None                               # dlsym succeeds on a raw handle
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert re.search(r"#define\s+SVK_KNN_CLUSTER_MUTUAL\s+%d\b" % _lib.KNN_CLUSTER_MUTUAL, code)


def test_version_and_pure_host_entry_points(lib):
    from speaker_verification_amd._lib import FrontendCfg
    from speaker_verification_amd import _lib as binding
    header = open(os.path.join(REPO, "include", "svk.h")).read()
    assert lib.svk_version() == binding.VERSION == int(re.search(r"#define SVK_VERSION (\d+)", header).group(1))
    cfg = FrontendCfg(320, 160, 512, 40, 13, 2, 1, 0, 1, 0.98)
    assert lib.svk_frontend_num_frames(ctypes.byref(cfg), 48000) == 298       # Q3
    assert lib.svk_frontend_num_frames(ctypes.byref(cfg), 319) == 0
    assert lib.svk_frontend_num_cols(ctypes.byref(cfg)) == 13
    cfg.out_kind = 1
    assert lib.svk_frontend_num_cols(ctypes.byref(cfg)) == 40
    cfg_b = FrontendCfg(400, 160, 1024, 40, 40, 1, 1, 0, 1, 0.0)
    assert lib.svk_frontend_num_frames(ctypes.byref(cfg_b), 48000) == 297


def test_error_codes_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    handle = ctypes.c_void_p()
    assert lib.svk_create(0, ctypes.byref(handle)) == -4          # SVK_ERR_NO_DEVICE, no abort
    assert lib.svk_sync(None) == -1
    assert lib.svk_last_error(None) == b"null context"


def test_product_fails_loudly_without_gpu():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speaker_verification_amd.speechpy import feature
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature.mfcc(np.zeros(16000, dtype=np.int16), 16000)


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package may reference it."""
    pkg = os.path.join(REPO, "speaker_verification_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


def test_host_sanitizer_build(tmp_path):
    """`make asan`: the HOST side of every translation unit under AddressSanitizer + UBSan (the
    device code is compiled as usual -- there is no GPU sanitizer on this pool).  A child interpreter with the
    ASan runtime preloaded loads that build through the normal binding and walks the entry points that need no
    GPU: version, the pure host helpers, every NULL / bad-argument early return, the no-device path."""
    import subprocess
    import sys
    csrc = os.path.join(REPO, "speaker_verification_amd", "csrc")
    so = os.path.join(REPO, "speaker_verification_amd", "libsvk_asan.so")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))] + \
           [os.path.join(REPO, "include", "svk.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asan"], check=True, stdout=subprocess.DEVNULL)
    runtime = subprocess.run(["/opt/rocm/bin/hipcc", "--print-file-name=libclang_rt.asan-x86_64.so"],
                             stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    assert os.path.exists(runtime)
    script = r'''
import ctypes, sys
sys.path.insert(0, %r)
from speaker_verification_amd import _lib
_lib.LIB_PATH = %r
lib = _lib.load()
assert lib.svk_version() == _lib.VERSION
cfg = _lib.FrontendCfg(320, 160, 512, 40, 13, 2, 1, 0, 1, 0.98, 1.0)
assert lib.svk_frontend_num_frames(ctypes.byref(cfg), 48000) == 298
assert lib.svk_frontend_num_frames(None, 48000) == 0 and lib.svk_frontend_num_cols(None) == 0
assert lib.svk_frontend_num_cols(ctypes.byref(cfg)) == 13
h = ctypes.c_void_p()
rc = lib.svk_create(0, ctypes.byref(h))
assert rc in (0, -4), rc                       # -4 = SVK_ERR_NO_DEVICE here; 0 on a GPU box
assert lib.svk_create(0, None) == -1
for fn, args in (("svk_sync", (None,)), ("svk_set_stream", (None, None)), ("svk_malloc", (None, 16, None)),
                 ("svk_memset", (None, None, 0, 4)), ("svk_device_info", (None, None)),
                 ("svk_comm_unique_id", (None, None)), ("svk_comm_init", (None, None, 1, 0)),
                 ("svk_allgather_f32", (None, None, None, 4)), ("svk_comm_destroy", (None,)),
                 ("svk_comm_info", (None, None)), ("svk_cmvn", (None, None, 1, 1, 1, None, 0)),
                 ("svk_cosine_scores", (None, None, None, 1, 1, 1, None)), ("svk_l2_dist", (None, None, None, 1, 1, None)),
                 ("svk_spectrum", (None, None, 1, 1, 512, 1, None)), ("svk_preemphasis", (None, None, 0, 1, 1, 0.5, None)),
                 ("svk_frontend_plan_create", (None, None, None, None)),
                 ("svk_roc_eer", (None, None, None, 1, None, 0, None))):
    assert getattr(lib, fn)(*args) == -1, fn   # SVK_ERR_BAD_ARG, no crash, nothing for ASan / UBSan to report
assert lib.svk_last_error(None) == b"null context"
assert lib.svk_roc_workspace_bytes(1000) > 0
lib.svk_destroy(None); lib.svk_frontend_plan_destroy(None)
if rc == 0:
    lib.svk_destroy(h)
print("asan walk ok")
''' % (REPO, so)
    env = dict(os.environ, LD_PRELOAD=runtime, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=600)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    assert b"asan walk ok" in proc.stdout
    assert b"runtime error" not in proc.stderr and b"AddressSanitizer" not in proc.stderr
