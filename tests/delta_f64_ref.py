"""Reference arithmetic for the three-channel input kernels (svk_delta_cmvn_stats, svk_delta_planes, svk_cube_gather_delta):
the planes in NumPy float32 exactly as the kernels form them, then statistics and normalisation in float64.  Used by
tests/test_delta_planes.py and tests/test_three_channel_pipeline.py.

THE PLANES.  For delta = 2 a delta value is (x[c + 1] + 2 x[c + 2]) * f32(1 / 10) with the column index clamped to the last
column: 1 * x and 2 * x are exact, so the sum is rounded once whether or not the device fuses the multiply into the add, and the
product with the f32 scale is rounded once: NumPy float32 gives the device's bits.  (For other windows k * x is not exact and a
fused multiply-add may round differently: there the kernels are compared with svk_derivative only.)  Delta-delta is the same
expression on the FLOAT32 delta values.

THE STATISTICS.  mean and 1 / (std + 2^-30) per column in float64 (two passes, population std), over the clip's rows of each
plane; the normalised value is float32(((double)v - mean) * inv), rounded once.
"""
import numpy as np

EPS = 2.0 ** -30


def inv_scale32(delta):
    return np.float32(1.0 / sum(2.0 * k * k for k in range(1, delta + 1)))


def derivative32(x32, delta=2):
    """[..., C] float32 -> the reference's 'derivative' (Q11) in float32: sum_k k * x[min(c + k, C - 1)] in order, one rounding
    per operation, times the float32 scale."""
    x32 = np.asarray(x32, dtype=np.float32)
    C = x32.shape[-1]
    cols = np.arange(C)
    acc = np.zeros_like(x32)
    for k in range(1, delta + 1):
        acc = acc + np.float32(k) * x32[..., np.minimum(cols + k, C - 1)]
    return (acc * inv_scale32(delta)).astype(np.float32)


def planes32(x32, delta=2):
    """[..., T, C] static float32 -> [3, ..., T, C]: static, delta, delta of the float32 delta."""
    x32 = np.asarray(x32, dtype=np.float32)
    d1 = derivative32(x32, delta)
    return np.stack([x32, d1, derivative32(d1, delta)])


def delta_f64_ref(x32, delta=2, variance=True):
    """One clip [T, C] (T >= 1) -> dict(planes [3, T, C] f32, mean [3, C], inv [3, C] (float64), want [3, T, C] f32 = the
    normalised planes, floor [3, C] = T 2^-50 max|v| inv: what statistics summed in another order may move a float64 value
    by before it is rounded (tests/postproc_f64_ref.py's cmvn floor))."""
    p = planes32(x32, delta)
    v = p.astype(np.float64)
    T = v.shape[1]
    mean = v.mean(1)
    inv = 1.0 / (v.std(1) + EPS) if variance else np.ones_like(mean)
    want = ((v - mean[:, None]) * inv[:, None]).astype(np.float32)
    return {"planes": p, "mean": mean, "inv": inv, "want": want, "floor": T * 2.0 ** -50 * np.abs(v).max(1) * inv}
