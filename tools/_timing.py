"""What the time_*.py tools share: the HIP-event timer, the call-by-call alternation, the SVK_TOOL_LIB loader, the head of the
result line and the entry that files one timing in it.  A tool builds its operands, times them and prints the one JSON line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec (6.3 TB/s is the measured copy rate)
_res = {}


def one(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(torch, fns, reps, warmup):
    """{name: sorted times in ms}: the functions take turns, call by call, so that clocks and cache state drift for all alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(one(torch, fn))
    return {name: sorted(v) for name, v in times.items()}


def timed(torch, fn, reps, warmup=3):
    """The median of one function's times, in ms."""
    return alternated(torch, {"fn": fn}, reps, warmup)["fn"][reps // 2]


def load_lib():
    """(the _lib module, the loaded library); SVK_TOOL_LIB=path/to/libsvk.so times another build of the library in the same
    process layout: entry points that build lacks are left unbound (hasattr(lib, name) tells)."""
    from speaker_verification_amd import _lib
    if os.environ.get("SVK_TOOL_LIB"):
        _lib.LIB_PATH = os.environ["SVK_TOOL_LIB"]
        lib = _lib.C.CDLL(_lib.LIB_PATH)
        _lib.VERSION = lib.svk_version()
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(lib, k)}
    return _lib, _lib.load()


def header(_lib, lib, sha=True, **fields):
    """Starts the result line: the library's path (relative to the repository; the file name alone for a library outside
    it), version and (sha) source digest, then the tool's own fields -- among them
    the empty dicts (ms, spread_ms, bytes, tb_s, flop, tf_s, ...) that `put` is to fill."""
    _res.clear()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.abspath(_lib.LIB_PATH)           # inside the repository: relative to it, so that a filed line names no machine
    _res.update(lib=os.path.relpath(path, repo) if path.startswith(repo + os.sep) else os.path.basename(path),
                version=int(lib.svk_version()))
    if sha:
        _res["csrc_sha"] = _lib.provenance()["csrc_sha"]
    _res.update(fields)
    return _res


def put(name, times, nbytes=None, flop=None):
    """Files a timing under `name` in the dicts the header declared: the median of sorted `times` (or the one median a tool
    took with `timed`), its spread, and the TB/s / TF/s that nbytes / flop amount to.  Returns the median."""
    med = times[len(times) // 2] if isinstance(times, list) else times
    _res["ms"][name] = round(med, 4)
    if "spread_ms" in _res:
        _res["spread_ms"][name] = [round(times[0], 4), round(times[-1], 4)]
    if nbytes:
        if "bytes" in _res:
            _res["bytes"][name] = int(nbytes)
        _res["tb_s"][name] = round(nbytes / (med * 1e-3) / 1e12, 3)
    if flop:
        if "flop" in _res:
            _res["flop"][name] = int(flop)
        _res["tf_s"][name] = round(flop / (med * 1e-3) / 1e12, 2)
    return med
