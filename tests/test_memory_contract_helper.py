"""tests/memory_contract.py proves itself on CPU tensors, and the coverage walk: every svk_* entry point defined in a source
file of the library (every *.hip of csrc/) has a case in tests/test_memory_contract_*.py or a stated exemption."""
import math
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "speaker_verification_amd", "csrc")


@pytest.mark.parametrize("env", M.ENV_NAMES)
@pytest.mark.parametrize("offset", (0, 4, 8, 16))
def test_untouched_arena_passes(env, offset):
    a = M.Arena(torch.float32, (3, 5), env, offset)
    assert (a.data_ptr - offset) % 256 == 0 and a.nbytes == 60
    assert a.lead >= M.GUARD and a.buf.numel() - a.lead - a.nbytes >= M.GUARD
    a.check()
    a.tensor.fill_(1.0)               # the whole payload may be written
    a.check()
    assert a.changed_guard_bytes() == (0, None)


@pytest.mark.parametrize("env", M.ENV_NAMES)
@pytest.mark.parametrize("where", (-1, 0, M.GUARD - 1, -M.GUARD))
def test_one_byte_on_either_side_is_caught(env, where):
    """One byte straight in front of the payload, straight behind it, and at the far end of either guard."""
    a = M.Arena(torch.float64, (7,), env, 8)
    at = a.nbytes + where if where >= 0 else where            # offset from the payload's start
    a.buf[a.lead + at] = a.guard_byte ^ 0x01
    assert a.changed_guard_bytes() == (1, at)
    with pytest.raises(AssertionError, match=r"1 guard bytes changed, the first at payload offset %d " % at):
        a.check()


def test_first_offset_and_count():
    a = M.Arena(torch.int32, (4,), "A", 4)
    a.buf[a.lead + a.nbytes + 3:a.lead + a.nbytes + 19] = 0          # a 16-byte store three bytes past the end
    a.buf[a.lead - 2] = 0
    assert a.changed_guard_bytes() == (17, -2)


def test_environments_give_the_intended_values():
    def t(env, dt):                   # two payload elements
        return M.Arena(dt, (2,), env).tensor.clone()

    def g(env, dt):                   # the first guard bytes as that type
        return M.Arena(dt, (2,), env).buf[:8].clone().view(dt)
    # A: zeros in the payload, a small finite number in the guards
    assert all(float(v) == 0.0 for dt in (torch.float32, torch.float64) for v in t("A", dt))
    assert all(int(v) == 0 for dt in (torch.int32, torch.int64, torch.uint8) for v in t("A", dt))
    assert all(math.isfinite(float(v)) and float(v) != 0.0 for dt in (torch.float32, torch.float64) for v in g("A", dt))
    # B: NaN as a float, -1 as an integer, on both sides
    for view in (t, g):
        assert all(math.isnan(float(v)) for dt in (torch.float32, torch.float64) for v in view("B", dt))
        assert all(int(v) == -1 for dt in (torch.int32, torch.int64) for v in view("B", dt))
    assert all(int(v) == 255 for v in t("B", torch.uint8))
    # C: finite, non-zero, and different on the two sides
    for dt in (torch.float32, torch.float64):
        p, q = float(t("C", dt)[0]), float(g("C", dt)[0])
        assert math.isfinite(p) and math.isfinite(q) and p != 0.0 and q != 0.0 and p != q
    assert int(t("C", torch.int32)[0]) == 0x5A5A5A5A and int(g("C", torch.int32)[0]) == 0x3C3C3C3C
    assert M.pattern(0x5A, 8) == 0x5A5A5A5A5A5A5A5A and M.Arena(torch.float64, (1,), "C").prefill() == 0x5A5A5A5A5A5A5A5A


def test_input_lies_flush_against_its_trailing_guard():
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    a = M.Arena(torch.float32, (3, 4), "B", 4, stride=7).put(src)
    assert a.numel == 2 * 7 + 4 and torch.equal(a.tensor, src)
    flat = a.payload.view(torch.float32)
    assert float(flat[-1]) == 11.0 and int(a.buf[a.lead + a.nbytes]) == 0xFF        # last element, then guard
    assert all(math.isnan(float(v)) for v in flat[4:7])                               # stride padding: the payload pattern
    a.unchanged()
    a.padding_kept()
    a.check()
    flat[5] = 0.0
    with pytest.raises(AssertionError, match="1 padding elements"):
        a.padding_kept()
    with pytest.raises(AssertionError, match="changed an input"):
        a.unchanged()


def test_contract_collects_and_verifies_on_the_host():
    c = M.Contract(None, "C", scalar=True)
    x = c.input("x", np.arange(5, dtype=np.float64))
    out = c.output("out", torch.float32, (5,))
    work = c.workspace(48)
    cnt = c.counter()
    assert c.input("absent", None) is None
    assert x.offset == 8 and out.offset == 4 and work.offset == 16 and work.nbytes == 48 and cnt.offset == 4
    assert int(cnt.tensor[0]) == M.COUNTER_PRESET
    M.counter_is(cnt, 0, "untouched")
    cnt.tensor.add_(2)
    M.counter_is(cnt, 2, "two added")
    with pytest.raises(AssertionError, match="went from 7 to 9, 1 were to be added"):
        M.counter_is(cnt, 1, "one expected")
    assert M.Contract(None, "C").input("x", np.zeros(3, np.float32)).offset == 0
    out.tensor.copy_(x.tensor)
    c.verify()
    M.same_bits(out.bits(), M.bits(torch.arange(5, dtype=torch.float32)), "out")
    M.keeps_prefill(work, work.bits(), "workspace")
    work.buf[work.lead + 48] = 0      # the byte straight behind the workspace
    with pytest.raises(AssertionError, match="workspace .*first at payload offset 48 "):
        c.verify()


def test_bits_tell_zeros_and_nans_apart():
    a = torch.tensor([0.0, -0.0, float("nan")])
    with pytest.raises(AssertionError, match="1 of 3 elements differ, the first at flat index 1"):
        M.same_bits(M.bits(a), M.bits(torch.tensor([0.0, 0.0, float("nan")])), "zeros")
    M.same_bits(M.bits(a), M.bits(a.clone()), "same")


# ---- the coverage walk -----------------------------------------------------------------------------------------------------
def _defined_entries():
    """Every name of _lib.SIGNATURES that one of the contract's source files DEFINES: `name ( parameters ) {` -- whatever its
    return type and however the line is broken (a call ends in `;` or sits inside an expression, not in front of a body)."""
    from speaker_verification_amd import _lib
    found = {}
    for src in M.CONTRACT_SOURCES:
        with open(os.path.join(CSRC, src)) as fh:
            text = fh.read()
        for fn in _lib.SIGNATURES:
            if re.search(r"\b%s\s*\([^;{}()]*\)\s*\{" % re.escape(fn), text):
                found[fn] = src
    return found


def test_every_entry_point_has_a_case_or_an_exemption():
    listing = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(M.CONTRACT_SOURCES) == listing and len(set(M.CONTRACT_SOURCES)) == len(M.CONTRACT_SOURCES), \
        "CONTRACT_SOURCES is not the library's source files: %s" % sorted(set(listing) ^ set(M.CONTRACT_SOURCES))
    from speaker_verification_amd import _lib
    defined = _defined_entries()
    assert len(defined) == len(_lib.SIGNATURES) == 97 and set(M.CONTRACT_SOURCES) == set(defined.values()), \
        "the walk no longer finds the entry points: %s" % sorted(set(_lib.SIGNATURES) - set(defined))
    missing = sorted(fn for fn in defined if fn not in M.CASES and fn not in M.EXEMPT)
    assert not missing, "entry points without a memory-contract case or an exemption: %s" % missing
    assert not set(M.CASES) & set(M.EXEMPT)
    stale = sorted(fn for fn in list(M.CASES) + list(M.EXEMPT) if fn not in defined)
    assert not stale, "listed but not defined in %s: %s" % (M.CONTRACT_SOURCES, stale)
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in M.EXEMPT.values())


def test_cases_name_modules_that_mention_their_entry():
    """A tripwire, not a proof: the module CASES names for an entry exists, is gpu-marked and spells `lib.<entry>` somewhere
    (a renamed file or a dropped case shows; a commented-out call would not)."""
    for fn, module in M.CASES.items():
        with open(os.path.join(REPO, "tests", module + ".py")) as fh:
            text = fh.read()
        assert re.search(r"lib\.%s\b" % fn, text), "%s does not call %s" % (module, fn)
        assert "pytest.mark.gpu" in text
