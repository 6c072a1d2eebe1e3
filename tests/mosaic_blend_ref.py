"""CPU restatement of the blended seabed mosaic (csrc/mosaic.h, "The blend"), helper of test_mosaic_blend_host.py and
test_gpu_mosaic_blend.py -- not a test.  It shares no code with the engine: the geometry and every cell's smallest range come from
tests/mosaic_ref.py (``pixels``, ``mosaic``), the weights and the quantised colours are numpy float32 arithmetic, one IEEE
operation per line, the sums are int64 (``np.add.at``: integer adds, any order), the final quotient is float64.
"""
import numpy as np
import torch

import mosaic_ref as ref

ACC_WORDS = 8   # per cell: wq Jq x 3, wq rgb x 3, wq, the sample count


def weights(z, zmin, H):
    """``wq`` (int64, 0..4096) of ranges ``z`` over their cells' smallest ranges ``zmin`` (float32 arrays) at the blend depth ``H``."""
    one, zero = np.float32(1), np.float32(0)
    inv_h = one / np.float32(H)
    assert inv_h.dtype == np.float32
    with np.errstate(over='ignore'):
        d = z - zmin
        s = d * inv_h
        t = np.maximum(one - s, zero)
        tt = t * t
        w = tt * np.float32(4096)
    assert all(q.dtype == np.float32 for q in (d, s, t, tt, w))
    return np.rint(w).astype(np.int64)      # round to nearest even


def quantised(J):
    """``Jq`` (int64, |Jq| <= 2^30) of float32 colours without NaN: clamped to +-1024 (infinities too), times 2^20, rounded."""
    lo = np.maximum(J, np.float32(-1024))
    c = np.minimum(lo, np.float32(1024))
    q = c * np.float32(1048576)
    assert q.dtype == np.float32
    return np.rint(q).astype(np.int64)


def blend(views, Js, axes, gsd, H, bounds=None, base=None):
    """The blended mosaic of ``views`` as a dict of CPU tensors ``J_blend, raw_blend, weight, samples`` (shaped like the engine's)
    and ``acc`` (Hm Wm, 8) int64, plus ``wq`` -- every sample's weight, in the order met -- and ``base``, ``mosaic_ref.mosaic``'s
    result for the same request (pass it to spare the second computation)."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if base is None:
        base = ref.mosaic(views, Js, axes, gsd, bounds=bounds)
    Hm, Wm = base['Hm'], base['Wm']
    lo_s, lo_t = np.float32(base['bounds'][0]), np.float32(base['bounds'][1])
    g = np.float32(gsd)
    zmin = base['range'].numpy().reshape(-1)
    acc = np.zeros((Hm * Wm, ACC_WORDS), np.int64)
    seen = []
    for view, J in zip(views, Js):
        p, z, a_s, a_t = ref.pixels(view, J, axes)
        qs, qt = (a_s.numpy() - lo_s) / g, (a_t.numpy() - lo_t) / g     # float32, IEEE
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)   # truncation
        p = p.numpy()[keep]
        wq = weights(z.numpy()[keep], zmin[cell], H)
        assert wq.min(initial=0) >= 0 and wq.max(initial=0) <= 4096
        seen.append(wq)
        use = wq > 0
        cell, p, wq = cell[use], p[use], wq[use]
        Jq = quantised(J.cpu().numpy().reshape(-1, 3)[p])
        rgb = view.rgb.cpu().numpy().reshape(-1, 3)[p].astype(np.int64)
        assert int(np.abs(Jq).max(initial=0)) <= 1 << 30
        for c in range(3):
            np.add.at(acc[:, c], cell, wq * Jq[:, c])
            np.add.at(acc[:, 3 + c], cell, wq * rgb[:, c])
        np.add.at(acc[:, 6], cell, wq)
        np.add.at(acc[:, 7], cell, 1)
    out = normalise(acc, Hm, Wm)
    out.update(acc=torch.from_numpy(acc), wq=np.concatenate(seen), base=base)
    return out


def normalise(acc, Hm, Wm):
    """The four outputs from the sums; asserts the bound under which no sum has wrapped."""
    count, wsum = acc[:, 7], acc[:, 6]
    assert int(count.max(initial=0)) < 2 ** 20
    filled = count > 0
    assert bool((wsum[filled] >= 4096).all())       # the winner of a cell has the full weight
    J = np.full((Hm * Wm, 3), np.nan, np.float32)
    raw = np.zeros((Hm * Wm, 3), np.uint8)
    weight = np.zeros(Hm * Wm, np.float32)
    w64 = wsum[filled].astype(np.float64)
    J[filled] = ((acc[filled, 0:3].astype(np.float64) / w64[:, None]) * 2.0 ** -20).astype(np.float32)
    raw[filled] = ((2 * acc[filled, 3:6] + wsum[filled, None]) // (2 * wsum[filled, None])).astype(np.uint8)    # all >= 0: floor = truncation
    weight[filled] = (w64 * 2.0 ** -12).astype(np.float32)
    return {'J_blend': torch.from_numpy(J).reshape(Hm, Wm, 3), 'raw_blend': torch.from_numpy(raw).reshape(Hm, Wm, 3),
            'weight': torch.from_numpy(weight).reshape(Hm, Wm), 'samples': torch.from_numpy(count.astype(np.int32)).reshape(Hm, Wm)}
