"""Guard memory for the memory contract of include/svk.h (Conventions): a call writes only the elements it documents as
outputs, what its workspaces and outputs hold on entry changes no result, and bytes beyond an input's documented extent change
no result.  tests/test_memory_contract_*.py hold every entry point of the library that touches device memory to it.

An `Arena` is ONE allocation laid out  guard | payload | guard.  Each guard is GUARD = 64 KiB -- a condition, not a
measurement: more than any single tile row or vector tail of the kernels can overrun, so that a stray store lands in memory the
test owns.  Nothing is ever placed at the end of an allocation, and nothing here provokes a fault.  The payload starts a chosen
number of bytes after a 256-byte boundary: 0 for the vector paths, the smallest alignment svk.h allows (the element size) for
the scalar paths, 16 where the ABI asks for 16.  Guards and payload are filled with byte patterns per ENVIRONMENT:

    A   guards 0xA5, payload 0x00   a value read from beyond an input, or from an unwritten output or workspace, is 0
    B   guards 0xFF, payload 0xFF   ... is NaN as f32 / f64 and -1 as an integer
    C   guards 0x3C, payload 0x5A   ... is a finite number of another magnitude on each side

An input fills its payload exactly, so its last element lies flush against the trailing guard; the padding between strided rows
keeps the payload pattern.  `Arena.check()` asserts every guard byte and reports the first changed offset and the count.
`Contract` runs one call of the library on arenas: it collects them, places them by the alignment rule, and after the call
checks every guard and that every input is byte-identical.  Everything works on CPU tensors too (the helper's own tests)."""
import ctypes as C

import numpy as np
import torch

GUARD = 64 * 1024
ENVIRONMENTS = {"A": (0xA5, 0x00), "B": (0xFF, 0xFF), "C": (0x3C, 0x5A)}   # name -> (guard byte, payload byte)
ENV_NAMES = tuple(ENVIRONMENTS)
COUNTER_PRESET = 7                       # counters "the caller zeroes" start here: the call may only ADD to them

_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def pattern(byte, size):
    """The unsigned integer of `size` bytes that all hold `byte`."""
    return int.from_bytes(bytes([byte]) * size, "little")


def bits(t):
    """A tensor's elements as a NumPy array of unsigned integers of the same width: what byte-for-byte comparisons use (a NaN
    equals itself, -0.0 differs from +0.0)."""
    t = t.detach().contiguous().cpu()
    return t.reshape(-1).view(torch.uint8).numpy().view(_UINT[t.element_size()]).reshape(tuple(t.shape))


class Arena:
    """guard | payload | guard in one allocation.  `shape` elements of `dtype`; a 2-D shape may have its rows `stride` elements
    apart (stride >= shape[1]): the payload then ends with the last row's last element."""

    def __init__(self, dtype, shape, env, offset=0, device="cpu", stride=None, name="buffer"):
        self.name, self.env, self.dtype, self.offset = name, env, dtype, int(offset)
        self.guard_byte, self.payload_byte = ENVIRONMENTS[env]
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.size = itemsize(dtype)
        if self.offset % self.size:
            raise ValueError("offset %d misaligns %s" % (offset, dtype))
        numel = int(np.prod(self.shape, dtype=np.int64))
        self.stride = None
        if stride is not None and len(self.shape) == 2 and numel:
            if stride < self.shape[1]:
                raise ValueError("stride below the row length")
            self.stride = int(stride)
            numel = (self.shape[0] - 1) * self.stride + self.shape[1]
        self.numel, self.nbytes = numel, numel * self.size
        total = GUARD + 256 + self.offset + self.nbytes + GUARD
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        self.lead = (-(self.buf.data_ptr() + GUARD)) % 256 + GUARD + self.offset     # the leading guard's length
        self.buf.fill_(self.guard_byte)
        self.payload = self.buf[self.lead:self.lead + self.nbytes]
        self.payload.fill_(self.payload_byte)
        self.data_ptr = self.buf.data_ptr() + self.lead
        assert (self.data_ptr - self.offset) % 256 == 0 and total - self.lead - self.nbytes >= GUARD
        self.saved = None

    # ---- the payload ----------------------------------------------------------------------------------------------------
    @property
    def ptr(self):
        return C.c_void_p(self.data_ptr)

    @property
    def tensor(self):
        """The payload as a tensor of the arena's dtype and shape (a view: strided rows where a stride was given)."""
        flat = self.payload.view(self.dtype)
        if self.stride is not None:
            return torch.as_strided(flat, self.shape, (self.stride, 1))
        return flat.view(self.shape)

    def put(self, src):
        """Copy `src` (same shape) into the payload and remember the bytes: `unchanged()` compares with them."""
        if self.numel:
            self.tensor.copy_(torch.as_tensor(src).to(self.dtype).reshape(self.shape))
        self.saved = self.payload.cpu().clone()
        return self

    def unchanged(self):
        assert self.saved is not None
        assert torch.equal(self.payload.cpu(), self.saved), "%s (environment %s): the call changed an input" % (self.name, self.env)

    def bits(self):
        """The elements as unsigned integers (a copy on the host), shaped like `tensor`."""
        return bits(self.tensor)

    def prefill(self):
        """The unsigned integer an element holds while nobody has written it."""
        return pattern(self.payload_byte, self.size)

    def padding_kept(self):
        """The bytes between strided rows still hold the payload pattern."""
        if self.stride is None or self.stride == self.shape[1]:
            return
        flat = bits(self.payload.view(self.dtype)).copy()
        rows = np.lib.stride_tricks.as_strided(flat, self.shape, (self.stride * flat.itemsize, flat.itemsize))
        rows[...] = self.prefill()
        bad = np.flatnonzero(flat != self.prefill())
        assert bad.size == 0, "%s (environment %s): %d padding elements between rows changed, the first at element %d" % (
            self.name, self.env, bad.size, bad[0])

    # ---- the guards -----------------------------------------------------------------------------------------------------
    def changed_guard_bytes(self):
        """-> (count, first): changed guard bytes and the first one's offset from the payload's start (negative: in front of
        it; >= nbytes: behind it), or (0, None)."""
        count, first = 0, None
        for start, region in ((0, self.buf[:self.lead]), (self.lead + self.nbytes, self.buf[self.lead + self.nbytes:])):
            bad = region != self.guard_byte
            n = int(bad.sum())
            if n:
                count += n
                if first is None:
                    first = start + int(torch.nonzero(bad)[0]) - self.lead
        return count, first

    def check(self):
        count, first = self.changed_guard_bytes()
        if count:
            where = "%d bytes in front of it" % -first if first < 0 else "%d bytes past its end" % (first - self.nbytes)
            raise AssertionError("%s (environment %s, %d payload bytes, %d bytes off a 256-byte boundary): %d guard bytes "
                                 "changed, the first at payload offset %d (%s)"
                                 % (self.name, self.env, self.nbytes, self.offset, count, first, where))


class Contract:
    """One call of the library in one environment.  scalar=False places every buffer on a 256-byte boundary (the vector paths),
    scalar=True one element past it (workspaces and whatever `off=` names: that many bytes).  `call` checks the status and
    synchronises; `verify` checks P1: every guard of every buffer, and every input byte for byte."""

    def __init__(self, eng, env, scalar=False):
        self.eng, self.env, self.scalar, self.arenas = eng, env, scalar, []
        self.device = eng.device if eng is not None else "cpu"

    def _arena(self, name, dtype, shape, off, stride):
        if off is None:
            off = itemsize(dtype)
        a = Arena(dtype, shape, self.env, off if self.scalar else 0, self.device, stride, name)
        self.arenas.append(a)
        return a

    def input(self, name, t, off=None, stride=None):
        """`t` (a tensor or array, copied) as an input flush against its trailing guard; None stays None (a NULL pointer)."""
        if t is None:
            return None
        t = torch.as_tensor(t)
        return self._arena(name, t.dtype, t.shape, off, stride).put(t)

    def input_where(self, name, t, live, off=None):
        """An input of which the header lets the call read only the elements where `live` (a bool tensor of t's shape) is
        set: those are copied, every other element holds the payload pattern (0, NaN / -1, a finite other number)."""
        t, live = torch.as_tensor(t), torch.as_tensor(live).to(self.device)
        a = self._arena(name, t.dtype, t.shape, off, None)
        a.tensor[live] = t.to(self.device)[live]
        a.saved = a.payload.cpu().clone()
        return a

    def output(self, name, dtype, shape, off=None, stride=None, prefill=None):
        a = self._arena(name, dtype, shape, off, stride)
        if prefill is not None:
            a.tensor.copy_(torch.as_tensor(prefill).to(dtype).reshape(a.shape))
        return a

    def workspace(self, nbytes):
        """P3: exactly the bytes the library asks for, the guard straight behind them (16-byte aligned: the ABI's demand)."""
        return self._arena("workspace", torch.uint8, (int(nbytes),), 16, None)

    def counter(self, name="counter"):
        """P4: an int32 counter the caller zeroes, preset to COUNTER_PRESET."""
        return self.output(name, torch.int32, (1,), prefill=torch.tensor([COUNTER_PRESET], dtype=torch.int32))

    def call(self, fn, *args):
        args = [a.ptr if isinstance(a, Arena) else a for a in args]
        self.eng._stream()
        rc = fn(self.eng.ctx, *args)
        torch.cuda.synchronize()
        if rc != 0:
            raw = self.eng.lib.svk_last_error(self.eng.ctx)
            raise AssertionError("%s returned %d: %s" % (fn.__name__, rc, raw.decode("utf-8", "replace") if raw else ""))
        self.verify()

    def verify(self):
        for a in self.arenas:
            a.check()
            if a.saved is not None:
                a.unchanged()
            else:
                a.padding_kept()


PLACED = ("vector", "scalar")             # what the cases are parametrised over: Contract(scalar=placed == "scalar")


def randn(seed, *shape):
    """Seeded N(0, 1) float32 on the host: the cases' inputs, the same on every run."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def counter_is(counter, added, what):
    """P4: the counter went from COUNTER_PRESET to COUNTER_PRESET + added."""
    now = int(counter.tensor.cpu()[0])
    assert now == COUNTER_PRESET + added, "%s: the counter went from %d to %d, %d were to be added" % (what, COUNTER_PRESET, now, added)


def same_bits(got, want, what):
    """Byte-for-byte equality of two arrays of `bits`, with the first difference in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s against %s" % (what, got.shape, want.shape)
    diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert diff.size == 0, "%s: %d of %d elements differ, the first at flat index %d (0x%x against 0x%x)" % (
        what, diff.size, got.size, diff[0], int(got.reshape(-1)[diff[0]]), int(want.reshape(-1)[diff[0]]))


def keeps_prefill(arena, region, what):
    """`region` (a slice of arena.bits()) still holds the payload pattern: the header calls it untouched."""
    region = np.asarray(region)
    bad = np.flatnonzero(region.reshape(-1) != arena.prefill())
    assert bad.size == 0, "%s (environment %s): %d of %d untouched elements were written, the first at flat index %d" % (
        what, arena.env, bad.size, region.size, bad[0])


# Every svk_* entry point defined in the library's sources (every *.hip of csrc/) is either exercised by a case (CASES: entry ->
# the test module that holds it) or exempt with a reason.  tests/test_memory_contract_helper.py walks _lib.SIGNATURES, the
# sources and the directory listing against the three, so that a later entry point or source file cannot be left out silently.
CONTRACT_SOURCES = ("scoring.hip", "search.hip", "plda.hip", "backend.hip", "pool.hip", "snorm.hip", "calibration.hip", "roc.hip",
                    "head.hip", "cluster.hip", "spectral.hip", "frontend.hip", "stages.hip", "vad.hip", "ingest.hip", "c3d2.hip",
                    "c3d2_tail.hip", "context.hip", "comm.hip", "knn_cluster.hip")
CASES = {
    "svk_frontend_run": "test_memory_contract_frontend",
    "svk_preemphasis": "test_memory_contract_stages",
    "svk_stack_frames": "test_memory_contract_stages",
    "svk_spectrum": "test_memory_contract_stages",
    "svk_mel_features": "test_memory_contract_stages",
    "svk_cmvn": "test_memory_contract_stages",
    "svk_cmvn_stats": "test_memory_contract_stages",
    "svk_delta_cmvn_stats": "test_memory_contract_stages",
    "svk_cmvnw": "test_memory_contract_stages",
    "svk_derivative": "test_memory_contract_stages",
    "svk_log_power": "test_memory_contract_stages",
    "svk_delta_planes": "test_memory_contract_stages",
    "svk_cube_gather": "test_memory_contract_stages",
    "svk_cube_gather_cmvn": "test_memory_contract_stages",
    "svk_cube_gather_delta": "test_memory_contract_stages",
    "svk_cube_draw_crops": "test_memory_contract_stages",
    "svk_vad_energy": "test_memory_contract_ingest",
    "svk_vad_adaptive": "test_memory_contract_vad_adaptive",
    "svk_ingest_resample": "test_memory_contract_ingest",
    "svk_c3d2_stage1": "test_memory_contract_network",
    "svk_c3d2_stage1_c3": "test_memory_contract_network",
    "svk_c3d2_stage1_multi": "test_memory_contract_network",
    "svk_c3d2_stage1_c3_multi": "test_memory_contract_network",
    "svk_c3d2_stage2": "test_memory_contract_network",
    "svk_c3d2_conv31": "test_memory_contract_network",
    "svk_c3d2_conv32t": "test_memory_contract_network",
    "svk_c3d2_conv41": "test_memory_contract_network",
    "svk_c3d2_conv42": "test_memory_contract_network",
    "svk_c3d2_fc5": "test_memory_contract_network",
    "svk_cosine_scores": "test_memory_contract_scoring",
    "svk_l2_dist": "test_memory_contract_scoring",
    "svk_pair_scores": "test_memory_contract_scoring",
    "svk_plda_pair_scores": "test_memory_contract_scoring",
    "svk_plda_scores": "test_memory_contract_scoring",
    "svk_cosine_topk": "test_memory_contract_scoring",
    "svk_cosine_topk_norm": "test_memory_contract_search_norm",
    "svk_class_scatter": "test_memory_contract_backend",
    "svk_embedding_project": "test_memory_contract_backend",
    "svk_embedding_pool": "test_memory_contract_backend",
    "svk_c3d2_head": "test_memory_contract_backend",
    "svk_roc_eer": "test_memory_contract_evaluation",
    "svk_roc_k": "test_memory_contract_evaluation",
    "svk_roc_dcf": "test_memory_contract_evaluation",
    "svk_decision_counts": "test_memory_contract_evaluation",
    "svk_top1": "test_memory_contract_evaluation",
    "svk_rocch": "test_memory_contract_rocch",
    "svk_pav_apply": "test_memory_contract_rocch",
    "svk_calibration_stats": "test_memory_contract_evaluation",
    "svk_calibration_apply": "test_memory_contract_evaluation",
    "svk_cohort_moments": "test_memory_contract_evaluation",
    "svk_score_norm": "test_memory_contract_evaluation",
    "svk_score_norm_pairs": "test_memory_contract_evaluation",
    "svk_window_crops": "test_memory_contract_diarization",
    "svk_segment_affinity": "test_memory_contract_diarization",
    "svk_ahc": "test_memory_contract_diarization",
    "svk_spectral_embed": "test_memory_contract_diarization",
    "svk_knn_cluster": "test_memory_contract_cluster",
}
_SIZE_ONLY = "host arithmetic on its arguments: touches no device memory (the cases pass its value as the workspace's exact length)"
_HOST_ONLY = "reads or writes host memory only: no device memory the caller owns"
_HANDLE = "makes, frees or configures what the library owns (the handle, a plan, the stream): no device memory the caller owns"
_RCCL = "RCCL, one process per GPU: not reachable from a single-process test"
_RUNTIME = "a thin wrapper of one HIP runtime call (hipMalloc, hipFree, hipMemcpy, hipMemset): no kernel of the library runs"
EXEMPT = {
    "svk_version": _HOST_ONLY,
    "svk_last_error": _HOST_ONLY,
    "svk_device_info": _HOST_ONLY,
    "svk_create": _HANDLE,
    "svk_destroy": _HANDLE,
    "svk_set_stream": _HANDLE,
    "svk_sync": _HANDLE,
    "svk_frontend_plan_create": _HANDLE,
    "svk_frontend_plan_destroy": _HANDLE,
    "svk_frontend_num_frames": _SIZE_ONLY,
    "svk_frontend_num_cols": _SIZE_ONLY,
    "svk_c3d2_stage1_lds_bytes": _SIZE_ONLY,
    "svk_c3d2_stage1_c3_lds_bytes": _SIZE_ONLY,
    "svk_c3d2_fc5_workspace_floats": _SIZE_ONLY,
    "svk_malloc": _RUNTIME,
    "svk_free": _RUNTIME,
    "svk_memcpy_h2d": _RUNTIME,
    "svk_memcpy_d2h": _RUNTIME,
    "svk_memset": _RUNTIME,
    "svk_comm_unique_id": _RCCL,
    "svk_comm_init": _RCCL,
    "svk_allgather_f32": _RCCL,
    "svk_comm_destroy": _RCCL,
    "svk_comm_info": _RCCL,
    "svk_plda_scores_workspace_bytes": _SIZE_ONLY,
    "svk_cosine_topk_workspace_bytes": _SIZE_ONLY,
    "svk_class_scatter_workspace_bytes": _SIZE_ONLY,
    "svk_roc_workspace_bytes": _SIZE_ONLY,
    "svk_roc_k_workspace_bytes": _SIZE_ONLY,
    "svk_roc_dcf_workspace_bytes": _SIZE_ONLY,
    "svk_calibration_stats_workspace_bytes": _SIZE_ONLY,
    "svk_ahc_workspace_bytes": _SIZE_ONLY,
    "svk_spectral_workspace_bytes": _SIZE_ONLY,
    "svk_rocch_workspace_bytes": _SIZE_ONLY,
    "svk_rocch_level_counts_offset": "host arithmetic on its argument (an offset into svk_rocch's workspace, for diagnostics): touches no device memory",
    "svk_rocch_max_vertices": "host arithmetic on its argument: touches no device memory (the cases pass its value as the planes' capacity)",
    "svk_cosine_topk_norm_workspace_bytes": _SIZE_ONLY,
    "svk_knn_cluster_workspace_bytes": _SIZE_ONLY,
    "svk_ahc_limits": "writes two constants to a host array: no device memory",
    "svk_spectral_limits": "writes three constants to a host array: no device memory",
}
