"""The synthetic corpus of the clustering pipeline tests: 40 speakers x 25 utterances, dim 128, every row its speaker's random
unit centre + 0.05 N(0, I), in shuffled order.  tests/test_knn_cluster_host.py establishes its separation in float64 (seeds
0 - 2); tests/test_cluster_pipeline.py clusters it on the device."""
import numpy as np

SPEAKERS, UTTERANCES, DIM, NOISE = 40, 25, 128, 0.05
# For this distribution the largest cross-speaker cosine of 1 000 rows lies around 0.36 - 0.45, draw by draw.  The tests want a
# margin on both sides of the threshold 0.5 (same speaker >= 0.58, others <= 0.38), so the stream is keyed (seed, STREAM) and
# STREAM is the first key at which the seeds 0 - 2 all keep that margin; the host test asserts it, nothing assumes it.
STREAM = 28


def corpus(seed):
    """-> (emb float32 [1000, 128], speaker int64 [1000])."""
    rng = np.random.default_rng([seed, STREAM])
    centres = rng.standard_normal((SPEAKERS, DIM))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    speaker = rng.permutation(np.repeat(np.arange(SPEAKERS), UTTERANCES))
    emb = centres[speaker] + NOISE * rng.standard_normal((speaker.size, DIM))
    return emb.astype(np.float32), speaker.astype(np.int64)


def topk_f64(cos, k):
    """The k-NN lists of a float64 cosine matrix whose diagonal is NaN (no self match): higher first, the lower index among
    equals -> (score float32 [n, k], index int64 [n, k])."""
    n = cos.shape[0]
    score, index = np.empty((n, k), dtype=np.float32), np.empty((n, k), dtype=np.int64)
    for i in range(n):
        cand = np.flatnonzero(~np.isnan(cos[i]))
        best = cand[np.lexsort((cand, -cos[i, cand]))[:k]]
        score[i], index[i] = cos[i, best], best
    return score, index
