"""Host side of pooled embeddings (no GPU): the new C-ABI entries are declared, bound and exported and refuse a NULL context;
`speaker_segments`, the chunk size in clips and the reference-RNG draw of K cubes per clip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svk_c3d2_stage1_multi", "svk_c3d2_stage1_c3_multi", "svk_embedding_pool")


def test_new_symbols_declared_bound_and_exported():
    from speaker_verification_amd import _lib
    header = open(os.path.join(REPO, "include", "svk.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(svk_ctx\* ctx," % name, header), name + " is not declared in svk.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # the two first-block entries: their parent's arguments plus one int32
    for name in NEW[:2]:
        parent = _lib.SIGNATURES[name[:-len("_multi")]]
        assert _lib.SIGNATURES[name] == (parent[0], parent[1] + [C.c_int32])
    assert "#define SVK_VERSION 114 " in header and _lib.VERSION == 114 == lib.svk_version()


def test_null_context_is_bad_arg():
    from speaker_verification_amd import _lib
    lib = _lib.load()
    stage1 = [None, None, 1, 200, 40, None, 20, 80, None, None, None, None, None, None, 0, None, 1]
    assert lib.svk_c3d2_stage1_multi(*stage1) == _lib.SVK_ERR_BAD_ARG
    assert lib.svk_c3d2_stage1_c3_multi(*stage1) == _lib.SVK_ERR_BAD_ARG
    assert lib.svk_embedding_pool(None, None, 4, 128, 1, 4, None, None, 0, None, None) == _lib.SVK_ERR_BAD_ARG


def test_speaker_segments_stable_and_complete():
    from speaker_verification_amd.pipeline import speaker_segments
    rng = np.random.default_rng(5)
    ids = rng.permutation(np.repeat(np.array(["id10003", "id10001", "id10007", "id10002"]), [5, 1, 9, 3]))
    uniq, start, index = speaker_segments(ids)
    assert list(uniq) == sorted(set(ids)) and start.dtype == np.int64 and index.dtype == np.int64
    assert start[0] == 0 and start[-1] == len(ids) and int(np.diff(start).sum()) == len(ids)
    assert sorted(index.tolist()) == list(range(len(ids)))
    for s, sid in enumerate(uniq):
        rows = index[start[s]:start[s + 1]]
        assert (ids[rows] == sid).all() and len(rows) == (ids == sid).sum()
        assert (np.diff(rows) > 0).all()            # stable: a speaker's utterances in the order they were listed
    uniq, start, index = speaker_segments(np.array([], dtype=np.int64))
    assert len(uniq) == 0 and start.tolist() == [0] and len(index) == 0


def test_clips_per_chunk():
    from speaker_verification_amd.pipeline import VerificationPipeline, clips_per_chunk
    assert clips_per_chunk(8, 3) == 2 and clips_per_chunk(8, 1) == 8 and clips_per_chunk(1024, 4) == 256
    assert clips_per_chunk(2, 5) == 1 and clips_per_chunk(8, 9) == 1           # K > micro_batch: one clip per chunk
    # the pipeline's chunks use it (no engine needed for the arithmetic)
    pipe = VerificationPipeline.__new__(VerificationPipeline)
    pipe.micro_batch, pipe.cubes_per_clip, pipe.crop_rng = 8, 3, "device"
    assert pipe.chunks(5) == [(0, 2), (2, 4), (3, 5)]                            # two clips per chunk, the last one shifted
    pipe.cubes_per_clip = 1
    assert pipe.chunks(5) == [(0, 5)]


def test_reference_rng_draw_is_clip_major():
    """crop_rng="reference", K = 2: randint(T - 80, size=20) twice per clip, in clip order -- draw[u, 0] then draw[u, 1]."""
    from speaker_verification_amd.pipeline import VerificationPipeline
    frames = [297, 181, 250]
    pipe = VerificationPipeline.__new__(VerificationPipeline)
    pipe.cubes_per_clip, pipe.rng = 2, np.random.RandomState(7)
    got = pipe.draw_crops(frames)
    rng = np.random.RandomState(7)
    want = np.stack([np.stack([rng.randint(T - 80, size=20) for _ in range(2)]) for T in frames])
    assert got.shape == (3, 2, 20) and got.dtype == np.int32 and np.array_equal(got, want)
    # K = 1 keeps today's [n, 20] draw and consumes the RandomState as before
    pipe.cubes_per_clip, pipe.rng = 1, np.random.RandomState(7)
    rng = np.random.RandomState(7)
    one = pipe.draw_crops(frames)
    assert one.shape == (3, 20) and np.array_equal(one, np.stack([rng.randint(T - 80, size=20) for T in frames]))
    with pytest.raises(ValueError, match="80"):
        pipe.draw_crops([80])
