"""The host side of the speaker search: `evaluation.topk_hits` against a direct loop, and the declaration of svk_cosine_topk in
the header and the binding (no GPU)."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hits_by_loop(indices, true_columns):
    n, k = indices.shape
    hits = np.zeros(k, dtype=np.int64)
    for row in range(n):
        for r in range(k):
            if true_columns[row] >= 0 and true_columns[row] in list(indices[row, :r + 1]):
                hits[r] += 1
    return hits


@pytest.mark.parametrize("n,k,cols", [(200, 5, 12), (50, 1, 3), (7, 32, 40), (0, 4, 9), (64, 8, 4)])
def test_topk_hits(n, k, cols):
    from speaker_verification_amd.evaluation import topk_hits
    rng = np.random.default_rng(n + k)
    indices = np.full((n, k), -1, dtype=np.int64)
    for row in range(n):                                           # distinct columns, best first, -1 past the candidates
        m = min(k, cols, int(rng.integers(0, k + 1)))
        indices[row, :m] = rng.permutation(cols)[:m]
    true = rng.integers(-1, cols, n)                               # -1: the speaker is not enrolled
    got = topk_hits(indices, true)
    assert got.dtype == np.int64 and got.shape == (k,)
    np.testing.assert_array_equal(got, hits_by_loop(indices, true))
    assert np.all(np.diff(got) >= 0)


def test_topk_hits_never_counts_minus_one():
    from speaker_verification_amd.evaluation import topk_hits
    indices = np.array([[-1, -1, -1], [2, -1, -1], [0, 1, 2]], dtype=np.int64)
    np.testing.assert_array_equal(topk_hits(indices, np.array([-1, -1, -1])), [0, 0, 0])
    np.testing.assert_array_equal(topk_hits(indices, np.array([0, 2, 2])), [1, 1, 2])
    np.testing.assert_array_equal(topk_hits(indices[:, :1], np.array([0, 2, 0])), [2])
    with pytest.raises(ValueError):
        topk_hits(indices, np.array([0, 1]))


def test_header_and_binding_declare_the_search():
    from speaker_verification_amd import _lib
    header = open(os.path.join(REPO, "include", "svk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"size_t\s+svk_cosine_topk_workspace_bytes\s*\(\s*int32_t n_query, int32_t n_gallery, int32_t dim, int32_t k\)", code)
    decl = re.search(r"int\s+svk_cosine_topk\s*\((.*?)\)\s*;", code, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 14
    assert len(_lib.SIGNATURES["svk_cosine_topk"][1]) == 14 and len(_lib.SIGNATURES["svk_cosine_topk_workspace_bytes"][1]) == 4
    assert int(re.search(r"#define SVK_VERSION (\d+)", header).group(1)) == _lib.VERSION == 114
