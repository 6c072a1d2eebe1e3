"""Numpy restatement of the mosaic's push-pull hole filling (sucre_amd/csrc/fill.h): the yardstick of tests/test_gpu_mosaic_fill.py.

It shares no code with the engine.  Everything is float32 and every line that computes performs ONE IEEE operation per element
(numpy does not contract a product and a sum of separate statements), so the device's bits can be compared exactly.  A level is a
dictionary ``c`` (H,W,6) float32, ``w`` (H,W) float32, ``g`` (H,W) float32 -- the eight floats of a record.
"""
import numpy as np

F = np.float32
TAPS = (F(9.0 / 16.0), F(3.0 / 16.0), F(3.0 / 16.0), F(1.0 / 16.0))   # all four exact in float32


def levels_for(R, gsd, Hm, Wm):
    """L: the smallest integer >= 1 with gsd 2^L >= R (float64), capped at the first level that is 1x1, at least 1."""
    R, gsd = float(R), float(gsd)
    L = 1
    while gsd * 2.0 ** L < R:
        L += 1
    cap, h, w = 0, int(Hm), int(Wm)
    while h > 1 or w > 1:
        h, w, cap = (h + 1) >> 1, (w + 1) >> 1, cap + 1
    return max(1, min(L, cap))


def level_sizes(Hm, Wm, L):
    """[(H_0, W_0), ..., (H_L, W_L)]"""
    out = [(int(Hm), int(Wm))]
    for _ in range(L):
        h, w = out[-1]
        out.append(((h + 1) >> 1, (w + 1) >> 1))
    return out


def pyramid_bytes(Hm, Wm, L):
    """What sucre_mosaic_fill_bytes gives: levels 1..L of 32-byte records, each level 256-byte aligned."""
    return sum((h * w * 32 + 255) // 256 * 256 for h, w in level_sizes(Hm, Wm, L)[1:])


def level0(J, raw, source):
    """The records level 0 stands for: valid where source >= 0 and the three J channels are finite; zeros elsewhere."""
    J = np.asarray(J, F)
    ok = (np.asarray(source) >= 0) & np.isfinite(J).all(axis=2)
    c = np.zeros(J.shape[:2] + (6,), F)
    c[..., 0:3] = J
    c[..., 3:6] = np.asarray(raw).astype(F)
    c[~ok] = F(0)
    return {'c': c, 'w': ok.astype(F), 'g': np.zeros(J.shape[:2], F)}


def pull(lv, index):
    """Level ``index`` = l + 1 from level l."""
    H, W = lv['w'].shape
    H1, W1 = (H + 1) >> 1, (W + 1) >> 1
    c = np.zeros((2 * H1, 2 * W1, 6), F)    # a child outside the level: a record of zeros
    w = np.zeros((2 * H1, 2 * W1), F)
    c[:H, :W] = lv['c']
    w[:H, :W] = lv['w']
    kids = [(c[dy::2, dx::2], w[dy::2, dx::2]) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    Wt = kids[0][1] + kids[1][1]
    Wt = Wt + kids[2][1]
    Wt = Wt + kids[3][1]
    p = [k[1][..., None] * k[0] for k in kids]     # each product rounded on its own
    S = p[0] + p[1]
    S = S + p[2]
    S = S + p[3]
    some = Wt > 0
    with np.errstate(all='ignore'):
        q = S / Wt[..., None]
    quarter = Wt * F(0.25)
    out = {'c': np.where(some[..., None], q, F(0)).astype(F), 'w': np.where(some, quarter, F(0)).astype(F),
           'g': np.where(some, F(index), F(0)).astype(F)}
    assert not np.signbit(out['c'][~some]).any()
    return out


def push(lv, up):
    """Fills the empty cells of ``lv`` (a level l, changed in place) from ``up`` (level l + 1, complete).  Returns lv."""
    H, W = lv['w'].shape
    H1, W1 = up['w'].shape
    y, x = np.arange(H), np.arange(W)
    py, px = y >> 1, x >> 1
    ny = np.clip(py + np.where(y & 1, 1, -1), 0, H1 - 1)
    nx = np.clip(px + np.where(x & 1, 1, -1), 0, W1 - 1)
    taps = [(py[:, None], px[None, :]), (py[:, None], nx[None, :]), (ny[:, None], px[None, :]), (ny[:, None], nx[None, :])]
    a = [np.where(up['w'][ty, tx] > 0, k, F(0)).astype(F) for (ty, tx), k in zip(taps, TAPS)]
    A = a[0] + a[1]
    A = A + a[2]
    A = A + a[3]
    p = [ai[..., None] * up['c'][ty, tx] for ai, (ty, tx) in zip(a, taps)]
    S = p[0] + p[1]
    S = S + p[2]
    S = S + p[3]
    g = np.zeros((H, W), F)
    for ai, (ty, tx) in zip(a, taps):
        g = np.where(ai > 0, np.maximum(g, up['g'][ty, tx]), g)
    fill = (lv['w'] == 0) & (A > 0)
    with np.errstate(all='ignore'):
        q = S / A[..., None]
    lv['c'][fill] = q[fill]
    lv['w'][fill] = F(1)
    lv['g'][fill] = g[fill]
    return lv


def fill(J, raw, source, L, check=True):
    """``J_filled`` (Hm,Wm,3) float32, ``raw_filled`` (Hm,Wm,3) uint8, ``fill_level`` (Hm,Wm) int32 and ``pyramid``, the levels
    1..L after the push as (h w, 8) float32 records.  ``check``: assert the two distance properties of the tap pattern."""
    J = np.ascontiguousarray(J, F)
    raw = np.ascontiguousarray(raw, np.uint8)
    source = np.ascontiguousarray(source, np.int32)
    L = int(L)
    assert L >= 1
    lv = [level0(J, raw, source)]
    for l in range(L):
        lv.append(pull(lv[l], l + 1))
    for l in range(L - 1, -1, -1):
        push(lv[l], lv[l + 1])
    base = lv[0]
    measured = source >= 0
    filled = ~measured & (base['w'] > 0)
    empty = ~measured & ~filled
    J_filled = J.copy()     # a measured cell: J bit for bit, a non-finite one included
    J_filled[filled] = base['c'][filled][:, 0:3]
    J_filled[empty] = np.uint32(0x7fc00000).view(F)
    raw_filled = raw.copy()
    lo = np.maximum(base['c'][..., 3:6], F(0))
    hi = np.minimum(lo, F(255))
    rounded = np.rint(hi).astype(np.uint8)
    raw_filled[filled] = rounded[filled]
    raw_filled[empty] = 0
    level = np.zeros(source.shape, np.int32)
    level[filled] = base['g'][filled].astype(np.int32)
    level[empty] = -1
    assert not filled.any() or (1 <= level[filled].min() and level[filled].max() <= L)
    if check:
        check_distances(base_valid(J, source), measured, filled, L)
    records = [np.concatenate([v['c'], v['w'][..., None], v['g'][..., None]], axis=2).reshape(-1, 8) for v in lv[1:]]
    return {'J_filled': J_filled, 'raw_filled': raw_filled, 'fill_level': level, 'pyramid': records}


def base_valid(J, source):
    return (np.asarray(source) >= 0) & np.isfinite(np.asarray(J, F)).all(axis=2)


def within(valid, d):
    """Cells within Chebyshev distance d of a valid cell (a box dilation by prefix sums)."""
    H, W = valid.shape
    s = np.zeros((H + 1, W + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(valid.astype(np.int64), axis=0), axis=1)
    y0, y1 = np.clip(np.arange(H) - d, 0, H), np.clip(np.arange(H) + d + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - d, 0, W), np.clip(np.arange(W) + d + 1, 0, W)
    return (s[y1[:, None], x1[None, :]] - s[y0[:, None], x1[None, :]] - s[y1[:, None], x0[None, :]] + s[y0[:, None], x0[None, :]]) > 0


def check_distances(valid, measured, filled, L):
    """Every empty cell within 2^(L-1) cells (Chebyshev) of a valid cell is filled; none at 3 x 2^L or more from every valid one."""
    near = within(valid, 1 << (L - 1))
    assert filled[near & ~measured].all(), 'a hole within 2^(L-1) cells of a valid cell stayed empty'
    far = ~within(valid, 3 * (1 << L) - 1)
    assert not filled[far].any(), 'a cell 3 x 2^L or more from every valid cell was filled'
