"""The memory contract of include/svk.h (Conventions) for the network entries of c3d2.hip and c3d2_tail.hip: svk_c3d2_stage1,
_c3, _multi, _c3_multi, svk_c3d2_stage2, conv31, conv32t, conv41, conv42 and fc5, called directly on guarded arenas
(tests/memory_contract.py) in the environments A, B and C.  `vector` places every buffer on a 256-byte boundary, `scalar` at
the smallest alignment the ABI allows: 16 bytes for activations, weight tables and workspaces, 8 for the first block's
d_feat, the element size for crop starts, biases and slopes.  The tables come from the committed synthetic checkpoint through
FusedEmbedder (tests/c3d2_f64_ref.py); every table is an input flush against its guard; activations are chained, each layer fed
the Engine's output of the one before, so that values stay in the half-pair domain.  Every comparison is on bytes, against the
Engine wrapper's result on ordinary tensors.  The outputs are documented as dense: no element may still hold the prefill in
all three environments."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import c3d2_f64_ref as R          # noqa: E402  (tests/ is on sys.path)
import memory_contract as M       # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
T_ROWS = 100                      # feature rows per clip: 20 is the last start whose 80 rows lie inside
MOST = 33                         # cubes the cases need at most: two M tiles of 16 cubes and one cube more


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def fe(eng):
    return copy.deepcopy(R.trained_model()).to(eng.device).eval().fused_inference()


@pytest.fixture(scope="module")
def fe3(eng):
    from speaker_verification_amd.model import perturb_inference_state, seeded_model
    model = seeded_model(7, 8, 3)
    model.load_state_dict(perturb_inference_state(model.state_dict(), 11))
    return model.eval().to(eng.device).fused_inference()


def _flag_values(tables, layers):
    """Both flag values.  2 is the caller's assertion that every PReLU slope lies in [0, 1]: the tables of the models used
    here must allow it, or the cases would silently run one value only."""
    assert len(tables) > 3 * layers and tables[3 * layers], "these tables do not allow flags = 2 (a PReLU slope outside [0, 1])"
    return (0, 2)


def _with_flags(tables, layers, flags):
    return tuple(tables[:3 * layers]) + ((True,) if flags else ())


def _dense(outs, what):
    """outs: {environment: (arena, bits)}.  No element holds its environment's prefill in all three."""
    still = None
    for arena, got in outs.values():
        same = got == arena.prefill()
        still = same if still is None else still & same
    assert not still.any(), "%s: %d elements were written in no environment" % (what, int(still.sum()))


# ---- the first block ---------------------------------------------------------------------------------------------------------
# crop starts: 0 and 20 (the last full crop), -1, 21, 60 and 99 (running off the clip: the lane-by-lane path) and T; the crops
# that run off are the LAST clip's (toward the trailing guard); the middle clip leaves rows at both ends unnamed
FIRST = [0, 20, -1, 13, 20, T_ROWS, 7, 19, 1, 20, 3, 11, 17, 2, 9, 20, 0, 15, 6, 20]
MIDDLE = [4, 15, 5, 13, 8, 4, 7, 9, 14, 10, 6, 11, 12, 4, 9, 15, 5, 15, 6, 10]
LAST = [2, 20, 5, 21, 20, 2, 7, 19, 60, 20, 3, 11, 99, 2, 9, 20, -1, 15, T_ROWS, 20]


def _starts(n, K):
    """[n][20] (K None) or [n][K][20] int32 and the rows of each clip some crop names [n][T]."""
    clips = {1: [LAST], 3: [FIRST, MIDDLE, LAST]}[n]
    named = torch.zeros((n, T_ROWS), dtype=torch.bool)
    for u, starts in enumerate(clips):
        for s in starts:
            if 0 <= s < T_ROWS:
                named[u, s:min(s + 80, T_ROWS)] = True
    assert not named[-1, :2].any() and named[-1, -1] and (n == 1 or not named[1, -4:].any())
    if K is None:
        return torch.tensor(clips, dtype=I32), named
    return torch.tensor([[list(np.roll(starts, 7 * k)) for k in range(K)] for starts in clips], dtype=I32), named


def _stage1_direct(eng, env, placed, three, feat, live, idx, tables, flags, K):
    n = feat.shape[0]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    df, di = c.input_where("d_feat", feat, live, off=8), c.input("d_crop_idx", idx)
    args = []
    for j in range(2):
        args += [c.input("d_w%dblk" % (j + 1), tables[3 * j], off=16), c.input("d_bias%d" % (j + 1), tables[3 * j + 1]),
                 c.input("d_slope%d" % (j + 1), tables[3 * j + 2])]
    out = c.output("d_out", F32, (n * (K or 1), 16, 36, 18, 16), off=16)
    name = "svk_c3d2_stage1" + ("_c3" if three else "") + ("_multi" if K else "")
    extra = (K,) if K else ()
    if name == "svk_c3d2_stage1":
        c.call(eng.lib.svk_c3d2_stage1, df, n, T_ROWS, 40, di, 20, 80, *args, flags, out)
    elif name == "svk_c3d2_stage1_c3":
        c.call(eng.lib.svk_c3d2_stage1_c3, df, n, T_ROWS, 40, di, 20, 80, *args, flags, out)
    elif name == "svk_c3d2_stage1_multi":
        c.call(eng.lib.svk_c3d2_stage1_multi, df, n, T_ROWS, 40, di, 20, 80, *args, flags, out, *extra)
    else:
        c.call(eng.lib.svk_c3d2_stage1_c3_multi, df, n, T_ROWS, 40, di, 20, 80, *args, flags, out, *extra)
    return name, out


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("static_items", (False, True), ids=("tickets", "static-items"))
@pytest.mark.parametrize("K", (None, 1, 3), ids=("parent", "multi-1", "multi-3"))
@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("three", (False, True), ids=("one-channel", "three-channel"))
def test_first_block(eng, fe, fe3, monkeypatch, three, n, K, static_items, placed):
    """Feature rows no crop names hold the pattern; a crop that runs off its clip reads zeros for the rows beyond it, also where
    those rows would be the next clip's or the trailing guard."""
    tables = (fe3 if three else fe).stage1_tables()
    idx, named = _starts(n, K)
    feat = M.randn(n + 3 * three, *((n, 3, T_ROWS, 40) if three else (n, T_ROWS, 40))) * 2
    live = (named[:, None, :, None] if three else named[:, :, None]).expand(feat.shape)
    for flags in _flag_values(tables, 2):
        use = _with_flags(tables, 2, flags)
        want = M.bits(eng.c3d2_stage1(feat, idx, use))
        if K == 1:
            M.same_bits(want, M.bits(eng.c3d2_stage1(feat, idx[:, 0], use)), "K = 1 against the parent entry")
        _static_items(monkeypatch, static_items)
        outs = {}
        for env in M.ENV_NAMES:
            name, out = _stage1_direct(eng, env, placed, three, feat, live, idx, tables, flags, K)
            outs[env] = (out, out.bits())
            M.same_bits(outs[env][1], want, "%s n %d flags %d, %s, environment %s" % (name, n, flags, placed, env))
        _dense(outs, name)
        monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)


# ---- the chained activations -------------------------------------------------------------------------------------------------
LAYER = {       # entry -> (Engine method, tables, layers, input shape, output shape)
    "svk_c3d2_stage2": ("c3d2_stage2", "stage2_tables", 2, (16, 36, 18, 16), (12, 15, 7, 32)),
    "svk_c3d2_conv31": ("c3d2_conv31", "conv31_tables", 1, (12, 15, 7, 32), (10, 8, 5, 15, 8)),
    "svk_c3d2_conv32t": ("c3d2_conv32t", "conv32t_tables", 1, (10, 8, 5, 15, 8), (8, 8, 45, 8)),
    "svk_c3d2_conv41": ("c3d2_conv41", "conv41_tables", 1, (8, 8, 45, 8), (6, 16, 27, 8)),
    "svk_c3d2_conv42": ("c3d2_conv42", "conv42_tables", 1, (6, 16, 27, 8), (4, 16, 9, 8)),
}
ORDER = tuple(LAYER) + ("svk_c3d2_fc5",)


def _ticket_cubes(eng):
    """Cubes per entry of the handle-state test.  A persistent kernel takes its first items from blockIdx -- one item in the
    second block, two in conv3_2 and conv4_1, three in the first block, each a whole grid apart -- and only the items behind
    them from tickets (ticket + 1, 2 or 3 grids).  With one workgroup per CU a counter therefore matters only to a launch of
    more than num_cu items in the second block (7 per cube), 2 num_cu in conv3_2 (5 per cube) and 3 num_cu in the first block
    (36 per cube): the counts below.  With the handful of cubes of the other cases a counter that is never zeroed changes
    nothing (tried: the mutant passed).
    NOT observable here: conv3_1's grid holds several workgroups per CU (as many as the occupancy calculator allows), so it
    uses a ticket only above that many times num_cu / 5 cubes, and conv4_1 (one item per cube) only above 2 num_cu cubes --
    hundreds of cubes, beyond what a test of this suite may allocate.  The two run below all the same (their results must
    not depend on the handle's history), but a counter of theirs left non-zero would pass."""
    return {"svk_c3d2_stage1": 3 * eng.num_cu // 36 + 2, "svk_c3d2_stage2": eng.num_cu // 7 + 2,
            "svk_c3d2_conv32t": 2 * eng.num_cu // 5 + 2, "svk_c3d2_conv31": 5, "svk_c3d2_conv41": 5}


OBSERVED = ("svk_c3d2_stage1", "svk_c3d2_stage2", "svk_c3d2_conv32t")      # entries whose counter the handle-state test can see


@pytest.fixture(scope="module")
def acts(eng, fe):
    """entry -> its input for max(MOST, the second block's cubes in the handle-state test): the Engine's output of the layer
    before, from random feature rows."""
    most = max(MOST, _ticket_cubes(eng)["svk_c3d2_stage2"])
    feat = M.randn(5, most, T_ROWS, 40) * 2
    idx = torch.tensor([MIDDLE] * most, dtype=I32)
    x, out = eng.c3d2_stage1(feat, idx, fe.stage1_tables()), {}
    for entry in ORDER[:-1]:
        out[entry] = x
        x = getattr(eng, LAYER[entry][0])(x, getattr(fe, LAYER[entry][1])())
    out["svk_c3d2_fc5"] = x
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    return out


def _layer_direct(eng, env, placed, entry, x, tables, flags, act2=None):
    """One call of a conv entry on arenas -> (d_out arena, the d_act2 arena or None)."""
    layers, out_shape = LAYER[entry][2], LAYER[entry][4]
    n = x.shape[0]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    args = [c.input("d_in", x, off=16)]
    for j in range(layers):
        args += [c.input("weight blocks %d" % j, tables[3 * j], off=16), c.input("bias %d" % j, tables[3 * j + 1]),
                 c.input("slope %d" % j, tables[3 * j + 2])]
    scratch = None
    if entry == "svk_c3d2_stage2":
        scratch = c.output("d_act2", F32, (n, 14, 36, 14, 32), off=16) if act2 else None
    out = c.output("d_out", F32, (n,) + out_shape, off=16)
    if entry == "svk_c3d2_stage2":
        c.call(eng.lib.svk_c3d2_stage2, args[0], n, *args[1:], flags, scratch, out)
    elif entry == "svk_c3d2_conv31":
        c.call(eng.lib.svk_c3d2_conv31, args[0], n, *args[1:], flags, out)
    elif entry == "svk_c3d2_conv32t":
        c.call(eng.lib.svk_c3d2_conv32t, args[0], n, *args[1:], flags, out)
    elif entry == "svk_c3d2_conv41":
        c.call(eng.lib.svk_c3d2_conv41, args[0], n, *args[1:], flags, out)
    else:
        c.call(eng.lib.svk_c3d2_conv42, args[0], n, *args[1:], flags, out)
    return out, scratch


def _hold_layer(eng, fe, acts, entry, n, placed, act2=None, act2_untouched=False):
    method, tables_of, layers = LAYER[entry][:3]
    tables = getattr(fe, tables_of)()
    x = acts[entry][:n].contiguous()
    for flags in _flag_values(tables, layers):
        want = M.bits(getattr(eng, method)(x, _with_flags(tables, layers, flags)))
        outs = {}
        for env in M.ENV_NAMES:
            out, scratch = _layer_direct(eng, env, placed, entry, x, tables, flags, act2)
            outs[env] = (out, out.bits())
            what = "%s n %d flags %d, %s, environment %s" % (entry, n, flags, placed, env)
            M.same_bits(outs[env][1], want, what)
            if act2_untouched:
                M.keeps_prefill(scratch, scratch.bits(), what + ": d_act2")
        _dense(outs, entry)


def _static_items(monkeypatch, on):
    """SVK_C3D2_STATIC_ITEMS set or REMOVED: a value from outside the test must not turn the ticket variant into the static one."""
    if on:
        monkeypatch.setenv("SVK_C3D2_STATIC_ITEMS", "1")
    else:
        monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("act2", ("NULL", "given"))
@pytest.mark.parametrize("static_items", (False, True), ids=("tickets", "static-items"))
@pytest.mark.parametrize("n", (1, 2, 5))
def test_stage2(eng, fe, acts, monkeypatch, n, static_items, act2, placed):
    """The one-kernel path never reads or writes d_act2: NULL is accepted, and a buffer keeps its prefill completely."""
    monkeypatch.delenv("SVK_C3D2_STAGE2_TWO_KERNELS", raising=False)
    _static_items(monkeypatch, static_items)
    _hold_layer(eng, fe, acts, "svk_c3d2_stage2", n, placed, act2 == "given", act2 == "given")


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n", (1, 2, 5))
def test_stage2_two_kernels(eng, fe, acts, monkeypatch, n, placed):
    """Under SVK_C3D2_STAGE2_TWO_KERNELS d_act2 is a workspace: guarded, and what it holds on entry changes nothing."""
    monkeypatch.setenv("SVK_C3D2_STAGE2_TWO_KERNELS", "1")
    _static_items(monkeypatch, False)
    _hold_layer(eng, fe, acts, "svk_c3d2_stage2", n, placed, True)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("static_items", (False, True), ids=("tickets", "static-items"))
@pytest.mark.parametrize("n", (1, 2, 5))
@pytest.mark.parametrize("entry", ("svk_c3d2_conv31", "svk_c3d2_conv32t", "svk_c3d2_conv41"))
def test_conv3_and_conv41(eng, fe, acts, monkeypatch, entry, n, static_items, placed):
    _static_items(monkeypatch, static_items)
    _hold_layer(eng, fe, acts, entry, n, placed)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_conv42(eng, fe, acts, n, placed):
    """An M tile is one position of 16 cubes: the rows of a ragged tile are clamped to the last cube, not read past it."""
    _hold_layer(eng, fe, acts, "svk_c3d2_conv42", n, placed)


def _fc5_direct(eng, env, placed, x, tables):
    n = x.shape[0]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    dx, dw, db = c.input("d_in", x, off=16), c.input("d_wfrag", tables[0], off=16), c.input("d_bias", tables[1], off=16)
    work = c.workspace(4 * eng.lib.svk_c3d2_fc5_workspace_floats(n))
    out = c.output("d_out", F32, (n, 128), off=16)
    c.call(eng.lib.svk_c3d2_fc5, dx, n, dw, db, work, out)
    return out


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_fc5(eng, fe, acts, n, placed):
    """d_work is exactly svk_c3d2_fc5_workspace_floats(n) floats, the guard straight behind them."""
    assert eng.lib.svk_c3d2_fc5_workspace_floats(n) == 4 * n * 128
    x = acts["svk_c3d2_fc5"][:n].contiguous()
    want = M.bits(eng.c3d2_fc5(x, fe.fc5_tables()))
    outs = {}
    for env in M.ENV_NAMES:
        out = _fc5_direct(eng, env, placed, x, fe.fc5_tables())
        outs[env] = (out, out.bits())
        M.same_bits(outs[env][1], want, "svk_c3d2_fc5 n %d, %s, environment %s" % (n, placed, env))
    _dense(outs, "svk_c3d2_fc5")


# ---- the handle's state ------------------------------------------------------------------------------------------------------
def _ticket_entries(handle, fe, acts, env):
    """Every entry that draws tickets from a counter in the handle's scratch (SVK_SLOT_STAGE1, STAGE2, CONV31, CONV32, CONV41),
    each run TWICE in a row on `handle` with _ticket_cubes' cubes -> {entry: (first bits, second bits)}."""
    cubes = _ticket_cubes(handle)
    n = cubes["svk_c3d2_stage1"]
    feat, idx = M.randn(3, n, T_ROWS, 40) * 2, torch.tensor([MIDDLE] * n, dtype=I32)
    live = torch.ones(feat.shape, dtype=torch.bool)
    got = {}
    for _ in range(2):
        _, out = _stage1_direct(handle, env, "vector", False, feat, live, idx, fe.stage1_tables(), 0, None)
        got.setdefault("svk_c3d2_stage1", []).append(out.bits())
    for entry in ("svk_c3d2_stage2", "svk_c3d2_conv31", "svk_c3d2_conv32t", "svk_c3d2_conv41"):
        x, n = acts[entry], cubes[entry]
        x = torch.cat([x] * -(-n // x.shape[0]))[:n].contiguous()       # cubes are independent: repeated where more are needed
        for _ in range(2):
            out, _ = _layer_direct(handle, env, "vector", entry, x, getattr(fe, LAYER[entry][1])(), 0)
            got.setdefault(entry, []).append(out.bits())
    return got


def test_ticket_counters_start_from_zero_at_every_call(eng, fe, acts, monkeypatch):
    """The work-item counters live in the handle's fixed scratch, which cannot be guarded: what can go wrong is a call that
    does not zero its counter, or another entry that disturbs it.  On a fresh handle: every ticket-drawing entry twice in a
    row, then again after the tail entries, svk_top1 and svk_c3d2_head (neighbouring scratch slots) have run -- the same bytes
    each time, equal to the long-lived handle's.  Only the counters of OBSERVED can show here, and only with the cube counts of
    _ticket_cubes (the one test of this module with more than a handful of cubes); conv3_1's and conv4_1's cannot."""
    from speaker_verification_amd.engine import Engine
    monkeypatch.delenv("SVK_C3D2_STATIC_ITEMS", raising=False)
    monkeypatch.delenv("SVK_C3D2_STAGE2_TWO_KERNELS", raising=False)
    want = _ticket_entries(eng, fe, acts, "A")
    fresh = Engine(eng.device_index)
    first = _ticket_entries(fresh, fe, acts, "B")
    y = fresh.c3d2_conv42(acts["svk_c3d2_conv42"][:17].contiguous(), fe.conv42_tables())
    emb = fresh.c3d2_fc5(y, fe.fc5_tables())
    fresh.top1(M.randn(3, 300, 65), torch.arange(300, dtype=I32) % 65)
    w6, b6 = (M.randn(65, 65, 128) * 0.2).to(eng.device), M.randn(66, 65).to(eng.device)
    fresh.c3d2_head(emb, (w6, b6, 0.25), probs=True, k=5, true_idx=torch.arange(17, dtype=I32) % 65)
    again = _ticket_entries(fresh, fe, acts, "C")
    wrong = []                        # every entry is judged, so that one failure does not hide another entry's
    for entry in want:
        runs = (("on the long-lived handle, the second call in a row", want[entry][1]),
                ("on a fresh handle, the first call", first[entry][0]), ("on a fresh handle, the second call in a row", first[entry][1]),
                ("after other entries used the handle", again[entry][0]), ("after them, the second call in a row", again[entry][1]))
        for when, got in runs:
            n_diff = int((got != want[entry][0]).sum())
            if n_diff:
                wrong.append("%s %s: %d of %d elements differ" % (entry, when, n_diff, got.size))
    assert not wrong, "results depend on the handle's history:\n  " + "\n  ".join(wrong)
