"""The host side of the score normalisation: the two statements of the selection rule in tests/snorm_f64_ref.py agree on
tie-heavy rows, `ScoreNorm`'s argument errors, the three new entries in the binding and the header, and `search` refusing a
score normalisation.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_f64_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("svk_cohort_moments", "svk_score_norm", "svk_score_norm_pairs")


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300, 1211])
def test_the_two_selection_rules_agree_on_tie_heavy_rows(n):
    rng = np.random.default_rng(100 + n)
    for trial in range(20):
        row = ref.tie_heavy_row(rng, n, levels=int(rng.integers(1, 6)))
        if trial % 4 == 1:                                # zeros of both signs among the ties, and non-finite columns
            row = np.where(rng.random(n) < 0.3, np.float32(-0.0), row)
            row = np.where(rng.random(n) < 0.1, np.float32(np.nan), row).astype(np.float32)
        for top_k in {0, 1, 2, 5, 300, max(n - 1, 1), n, n + 5}:
            m, vstar, sel = ref.select_threshold(row, top_k)
            m2, vstar2, sel2 = ref.select_sorted(row, top_k)
            assert m == m2 == ref.used_count(int(np.isfinite(row).sum()), top_k)
            if m == 0:
                assert np.isnan(vstar) and np.isnan(vstar2)
                continue
            assert vstar.tobytes() == vstar2.tobytes() and not (vstar == 0 and np.signbit(vstar))
            assert np.sort(sel).tobytes() == sel2.tobytes()          # the same multiset, -0.0 as +0.0 in both
            assert sel.size == m and sel.min() == vstar


def test_the_additions_follow_the_team_size():
    assert ref.team_size(2048) == 64 and ref.team_size(2049) == 256
    assert ref.additions(1) == 1 + 6 + 1 and ref.additions(1211) == 19 + 6 + 1 and ref.additions(2048) == 32 + 6 + 1
    assert ref.additions(2049) == 9 + 6 + 4 + 1
    assert ref.additions(ref.ROW_LDS_MAX + 1) == 65 + 6 + 4 + 1


def test_score_norm_argument_errors():
    from speaker_verification_amd.score_norm import ScoreNorm
    with pytest.raises(ValueError, match="mode"):
        ScoreNorm(mode="as")
    with pytest.raises(ValueError, match="top_k"):
        ScoreNorm(top_k=-1)
    with pytest.raises(ValueError, match="top_k"):
        ScoreNorm(top_k=2.5)
    sn = ScoreNorm(top_k=0, mode="z")
    assert (sn.top_k, sn.mode) == (0, "z") and ScoreNorm().top_k == 300 and ScoreNorm().mode == "s"
    rows = np.zeros((2, 4), dtype=np.float32)
    with pytest.raises(RuntimeError, match="not fitted"):
        sn.moments(rows, "test")
    with pytest.raises(ValueError, match="side"):
        sn.moments(rows, "cohort")
    with pytest.raises(RuntimeError, match="not fitted"):
        sn.normalize(rows, None, None)
    with pytest.raises(RuntimeError, match="not fitted"):
        sn.check_scorer(None, None)


def test_binding_and_header_declare_the_three_entries():
    from speaker_verification_amd import _lib
    header = open(os.path.join(REPO, "include", "svk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES
        decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert decl is not None, name + " is not declared in svk.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    assert int(re.search(r"#define SVK_VERSION (\d+)", header).group(1)) == _lib.VERSION == 114
    makefile = open(os.path.join(REPO, "speaker_verification_amd", "csrc", "Makefile")).read()
    assert "snorm.hip" in re.search(r"^SRCS\s*=(.*)$", makefile, flags=re.M).group(1).split()


def test_search_refuses_a_score_normalisation():
    from speaker_verification_amd.pipeline import VerificationPipeline
    pipe = VerificationPipeline.__new__(VerificationPipeline)
    pipe.plda = pipe.calibration = None
    pipe.score_norm = object()
    with pytest.raises(ValueError, match="normalised"):
        pipe.search(np.zeros((2, 4), np.float32), np.zeros((3, 4), np.float32))
