"""CPU restatement of the feathered mosaic blend (csrc/mosaic.h, "The feather"), helper of test_mosaic_feather_host.py and
test_gpu_mosaic_feather.py -- not a test.  It shares no code with the engine: the distance map is a brute force over the
definition, the weights are numpy float32 arithmetic, one IEEE operation per line, the geometry and every cell's smallest range
come from tests/mosaic_ref.py, the quantised colours from tests/mosaic_blend_ref.py, the sums are int64.

Two brute forces of one definition.  ``dist2_shifted`` is the literal one -- a false frame of width F round the mask, the
minimum over every offset with dx^2 + dy^2 < F^2 of the shifted masks -- and takes pi F^2 array operations: the host test runs
it for small F.  ``dist2`` takes, for every member, the minimum over ALL the non-members and over the ring of cells just outside
the image (a cell further out is further from every pixel than the ring cell on the way to it), which costs the same for every
F; the host test checks that the two agree.
"""
import numpy as np
import torch

import mosaic_blend_ref as bref
import mosaic_ref as ref

ACC_WORDS = bref.ACC_WORDS


def members(depth, J):
    """The pixels that take part: depth > 0 and no NaN in any channel of J (tensors or arrays)."""
    depth, J = np.asarray(depth, np.float32), np.asarray(J, np.float32)
    return (depth > 0) & ~np.isnan(J).any(axis=2)


def nearest2(member):
    """D2 (int64, (H,W)): per member the squared distance to the nearest non-member or cell outside the image; 0 for a non-member."""
    member = np.asarray(member, bool)
    H, W = member.shape
    v, u = np.nonzero(~member)
    ring_u = np.concatenate([np.arange(-1, W + 1), np.arange(-1, W + 1), np.full(H, -1), np.full(H, W)])
    ring_v = np.concatenate([np.full(W + 2, -1), np.full(W + 2, H), np.arange(H), np.arange(H)])
    ou, ov = np.concatenate([u, ring_u]).astype(np.int64), np.concatenate([v, ring_v]).astype(np.int64)
    mv, mu = np.nonzero(member)
    out = np.zeros((H, W), np.int64)
    step = max(1, (1 << 22) // len(ou))
    for i in range(0, len(mu), step):
        du = mu[i:i + step, None].astype(np.int64) - ou[None, :]
        dv = mv[i:i + step, None].astype(np.int64) - ov[None, :]
        out[mv[i:i + step], mu[i:i + step]] = (du * du + dv * dv).min(axis=1)
    return out


def dist2(member, F):
    """``min(D2, F^2)`` (int64, (H,W)); 0 for a non-member, at least 1 for a member."""
    return np.minimum(nearest2(member), int(F) * int(F))


def dist2_shifted(member, F):
    """The same by shifted masks: the literal brute force, pi F^2 array operations."""
    member, F = np.asarray(member, bool), int(F)
    H, W = member.shape
    padded = np.zeros((H + 2 * F, W + 2 * F), bool)
    padded[F:F + H, F:F + W] = member
    best = np.full((H, W), F * F, np.int64)
    for dy in range(-(F - 1), F):
        for dx in range(-(F - 1), F):
            if dx * dx + dy * dy < F * F:
                there = padded[F + dy:F + dy + H, F + dx:F + dx + W]
                best = np.where(~there, np.minimum(best, dx * dx + dy * dy), best)
    return np.where(member, best, 0)


def weights(z, zmin, H, d2, F):
    """``wq`` (int64, 0..4096) of ranges ``z`` over their cells' smallest ranges ``zmin`` (float32 arrays) at the blend depth ``H``,
    with capped squared border distances ``d2`` (integers) at the feather width ``F``."""
    one, zero = np.float32(1), np.float32(0)
    inv_h = one / np.float32(H)
    inv_f = one / np.float32(F)
    assert inv_h.dtype == np.float32 and inv_f.dtype == np.float32
    d2 = np.asarray(d2, np.int64)
    with np.errstate(over='ignore'):
        d = z - zmin
        s = d * inv_h
        t = np.maximum(one - s, zero)
        tt = t * t
        r = np.sqrt(d2.astype(np.float32))
        g = r * inv_f
        f = np.where(d2 >= int(F) * int(F), one, g)
        wf = tt * f
        w = wf * np.float32(4096)
    assert all(q.dtype == np.float32 for q in (d, s, t, tt, r, g, f, wf, w))
    return np.rint(w).astype(np.int64)      # round to nearest even


def normalise(acc, Hm, Wm):
    """mosaic_blend_ref.normalise with the feather's bound: a filled cell's winner has wq >= 4, not 4096."""
    count, wsum = acc[:, 7], acc[:, 6]
    assert int(count.max(initial=0)) < 2 ** 20
    filled = count > 0
    assert bool((wsum[filled] >= 4).all())
    J = np.full((Hm * Wm, 3), np.nan, np.float32)
    raw = np.zeros((Hm * Wm, 3), np.uint8)
    weight = np.zeros(Hm * Wm, np.float32)
    w64 = wsum[filled].astype(np.float64)
    J[filled] = ((acc[filled, 0:3].astype(np.float64) / w64[:, None]) * 2.0 ** -20).astype(np.float32)
    raw[filled] = ((2 * acc[filled, 3:6] + wsum[filled, None]) // (2 * wsum[filled, None])).astype(np.uint8)
    weight[filled] = (w64 * 2.0 ** -12).astype(np.float32)
    return {'J_blend': torch.from_numpy(J).reshape(Hm, Wm, 3), 'raw_blend': torch.from_numpy(raw).reshape(Hm, Wm, 3),
            'weight': torch.from_numpy(weight).reshape(Hm, Wm), 'samples': torch.from_numpy(count.astype(np.int32)).reshape(Hm, Wm)}


def blend(views, Js, axes, gsd, H, F, bounds=None, base=None, near=None):
    """The feathered blend of ``views`` as mosaic_blend_ref.blend gives the unfeathered one: ``J_blend, raw_blend, weight, samples``,
    ``acc`` (Hm Wm, 8) int64, ``wq`` and ``base``.  ``near``: per image ``nearest2`` of its members, to spare computing it again."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if base is None:
        base = ref.mosaic(views, Js, axes, gsd, bounds=bounds)
    Hm, Wm = base['Hm'], base['Wm']
    lo_s, lo_t = np.float32(base['bounds'][0]), np.float32(base['bounds'][1])
    g = np.float32(gsd)
    zmin = base['range'].numpy().reshape(-1)
    acc = np.zeros((Hm * Wm, ACC_WORDS), np.int64)
    seen = []
    for i, (view, J) in enumerate(zip(views, Js)):
        p, z, a_s, a_t = ref.pixels(view, J, axes)
        D2 = nearest2(members(view.depth.cpu().numpy(), J.cpu().numpy())) if near is None else near[i]
        d2 = np.minimum(D2, int(F) * int(F)).reshape(-1)
        qs, qt = (a_s.numpy() - lo_s) / g, (a_t.numpy() - lo_t) / g     # float32, IEEE
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)   # truncation
        p = p.numpy()[keep]
        assert bool((d2[p] >= 1).all())        # a pixel that takes part is a member
        wq = weights(z.numpy()[keep], zmin[cell], H, d2[p], F)
        assert wq.min(initial=0) >= 0 and wq.max(initial=0) <= 4096
        seen.append(wq)
        use = wq > 0
        cell, p, wq = cell[use], p[use], wq[use]
        Jq = bref.quantised(J.cpu().numpy().reshape(-1, 3)[p])
        rgb = view.rgb.cpu().numpy().reshape(-1, 3)[p].astype(np.int64)
        for c in range(3):
            np.add.at(acc[:, c], cell, wq * Jq[:, c])
            np.add.at(acc[:, 3 + c], cell, wq * rgb[:, c])
        np.add.at(acc[:, 6], cell, wq)
        np.add.at(acc[:, 7], cell, 1)
    out = normalise(acc, Hm, Wm)
    out.update(acc=torch.from_numpy(acc), wq=np.concatenate(seen), base=base)
    return out


# ---- the crafted pair of the seam property ----------------------------------------------------------------------------------------
SEAM_F = 16
SEAM_K = torch.tensor([[64.0, 0.0, 32.0], [0.0, 64.0, 24.0], [0.0, 0.0, 1.0]])
SEAM_KINV = torch.tensor([[2.0 ** -6, 0.0, -0.5], [0.0, 2.0 ** -6, -0.375], [0.0, 0.0, 1.0]])
SEAM_GSD = 2.0 ** -6      # one pixel's footprint at depth 1: c = 1 source pixel per cell along a row
SEAM_HW = (48, 64)        # A; B is its left half, 48 x 32


def seam_pair():
    """Two fronto-parallel images of a plane at depth 1 through one camera with dyadic intrinsics, so that pixel (u, v) lands in
    cell (v, u) exactly and the two images' ranges tie to the bit (t = 1 for both: the weights are the feather alone).  A, 64 x 48,
    covers the grid with J = 0.2; B, 32 x 48, covers the left half with J = 0.8.  ``(views, Js)`` as CPU tensors."""
    from types import SimpleNamespace
    H, W = SEAM_HW
    views, Js = [], []
    for w, colour in ((W, 0.2), (W // 2, 0.8)):
        rgb = torch.full((H, w, 3), int(colour * 255), dtype=torch.uint8)
        views.append(SimpleNamespace(depth=torch.ones(H, w), rgb=rgb, K=SEAM_K, R=torch.eye(3), t=torch.zeros(3, 1), Kinv=SEAM_KINV))
        Js.append(torch.full((H, w, 3), colour, dtype=torch.float32))
    return views, Js


def seam_bound(c=1, F=SEAM_F):
    """0.6 (c + 1) / F + 2^-19: d/df [(0.2 + 0.8 f) / (1 + f)] <= 0.6, and f moves by at most c / F per cell (float64)."""
    return 0.6 * (c + 1) / F + 2.0 ** -19


def largest_row_step(J_blend, F=SEAM_F):
    """The largest |difference| of horizontally adjacent cells of ``J_blend`` (Hm,Wm,3), over the rows that lie more than F
    pixels from the images' top and bottom edges (float64)."""
    J = np.asarray(J_blend, np.float64)
    rows = J[F:J.shape[0] - F]
    assert len(rows) > 0 and not np.isnan(rows).any()
    return float(np.abs(rows[:, 1:] - rows[:, :-1]).max())
