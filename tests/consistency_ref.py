"""float64 numpy restatement of sucre_view_consistency on explicit match lists (helper of test_gpu_consistency.py, not a test).

``reference(J_A, rgb_A, views)``: ``views[k]`` is ``((u1, v1, u2, v2), J_B, rgb_B)`` -- the matches of the target with view k as
integer arrays, the view's restored image (H_k,W_k,3) or None (the view takes no part: a zero row), its uint8 colours or None
(zero raw sums; also when ``rgb_A`` is None).  A pair is valid when neither ``J_A[v1,u1]`` nor ``J_B[v2,u2]`` holds a NaN.
Returns ``(count, ssd, stats, stats_abs, valid)``: int64 (H,W), float64 (H,W,3), float64 (n_views,26) in the library's column
order -- matches, valid pairs, then sum d^2, a^2, b^2, a b per channel for J and for the raw colours k / 255 --, the same table
with every term replaced by its magnitude (what an accumulation's rounding error is proportional to), and per view the boolean
mask of its valid pairs over its match list.  Colours enter as the float32 values the kernel reads, widened exactly."""
import numpy as np


def unit_from_u8(k):
    """float32(k / 255): correctly rounded, so the same number as float32(k) / float32(255) in IEEE float32."""
    return (np.asarray(k, np.float64) / 255.0).astype(np.float32)


def lists_of_map(match_map, W2):
    """(u1, v1, u2, v2) of a dense map[(v1,u1)] = v2 * W2 + u2 (-1: none), in row-major order."""
    m = np.asarray(match_map)
    v1, u1 = np.nonzero(m >= 0)
    q = m[v1, u1].astype(np.int64)
    return u1, v1, q % W2, q // W2


def _four_sums(a, b):
    with np.errstate(invalid='ignore'):   # infinities in J are data: inf - inf and inf + -inf are NaN, silently
        d = a - b
        terms = [d * d, a * a, b * b, a * b]
        return np.concatenate([t.sum(axis=0) for t in terms]), np.concatenate([np.abs(t).sum(axis=0) for t in terms])


def reference(J_A, rgb_A, views):
    J_A = np.asarray(J_A, np.float32)
    H, W = J_A.shape[:2]
    count = np.zeros((H, W), np.int64)
    ssd = np.zeros((H, W, 3), np.float64)
    stats = np.zeros((len(views), 26), np.float64)
    stats_abs = np.zeros_like(stats)
    valids = []
    for k, ((u1, v1, u2, v2), J_B, rgb_B) in enumerate(views):
        if J_B is None:
            valids.append(None)
            continue
        J_B = np.asarray(J_B, np.float32)
        a32, b32 = J_A[v1, u1], J_B[v2, u2]
        valid = ~(np.isnan(a32).any(axis=1) | np.isnan(b32).any(axis=1))
        valids.append(valid)
        a, b = a32[valid].astype(np.float64), b32[valid].astype(np.float64)
        stats[k, 0], stats[k, 1] = len(u1), int(valid.sum())
        stats_abs[k, :2] = stats[k, :2]
        stats[k, 2:14], stats_abs[k, 2:14] = _four_sums(a, b)
        if rgb_A is not None and rgb_B is not None:
            ra = unit_from_u8(np.asarray(rgb_A)[v1, u1][valid]).astype(np.float64)
            rb = unit_from_u8(np.asarray(rgb_B)[v2, u2][valid]).astype(np.float64)
            stats[k, 14:26], stats_abs[k, 14:26] = _four_sums(ra, rb)
        np.add.at(count, (v1[valid], u1[valid]), 1)
        with np.errstate(invalid='ignore'):
            np.add.at(ssd, (v1[valid], u1[valid]), (a - b) ** 2)
    return count, ssd, stats, stats_abs, valids
