"""CPU float32 restatement of the seabed mosaic (csrc/mosaic.h), helper of test_gpu_mosaic.py and test_mosaic_host.py -- not a test.
It shares no code with the engine: the geometry restates the reference's formulas (``Image.unproject_depth``, sfm.py:90-93;
``Pose.transform``, sfm.py:49-55; ``axes @ wP``) operation by operation, the winner of a cell comes from a lexicographic sort.

Why not the reference's tensor expressions as they stand.  They were the plan, and they do not pin a bit, for three reasons, all
measured.  (1) ``R @ cP`` goes through the BLAS torch was built with, and what that does with three products and two sums
depends on the CPU it runs on: the very expression gave a lower bound of the 6-view survey one ulp apart on two machines.  The
engine defines a 3x3 product as ``fma(m2, z, fma(m1, y, m0 x))`` (match_pixel.h; what the reference's machine computed for the
goldens); ``fma32`` below is that operation exactly, on any machine: the product of two float32 is exact in float64, the
float64 sum is corrected to round-to-odd with the error term of Knuth's TwoSum, and a round-to-odd float64 rounds to the correctly
rounded float32 (53 >= 2 x 24 + 2).  (2) ``Tensor.norm`` contracts its accumulation into FMAs (23 808 of 200 001 random camera
points differ in the last bit from the unfused sum), while the range is, everywhere in the engine (invert.h, match.hip), the
unfused ``sqrt((x x + y y) + z z)``.  (3) torch's vectorised float32 square root is not correctly rounded (686 of 100 000 random
sums differ from the IEEE root; numpy's never).  So everything below is numpy float32 arithmetic, one IEEE operation per line, and
``pixels`` asserts that the result stays within a few ulps of the reference's own expressions evaluated by torch.

``view``: any object with ``depth`` (H,W) float32, ``rgb`` (H,W,3) uint8, ``K`` (3,3), ``R`` (3,3), ``t`` (3,1) float32 CPU tensors
(and optionally ``Kinv``); ``J``: (H,W,3) float32.
"""
import numpy as np
import torch


def fma32(a, b, c):
    """``float32(a * b + c)`` with ONE rounding, for float32 arrays (or scalars) -- see the module's docstring."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)   # exact: 48 bits
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                     # TwoSum: s + e == p + c exactly
    other = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))   # the exact sum lies between s and this neighbour
    odd = np.where((s.view(np.int64) & 1) == 1, s, other)
    return np.where(e != 0, odd, s).astype(np.float32)


def dot3(row, x, y, z):
    """match_pixel.h's dot3: ``fma(r2, z, fma(r1, y, r0 x))``."""
    row = np.asarray(row, np.float32)
    return fma32(row[2], z, fma32(row[1], y, row[0] * x))


def pixels(view, J, axes):
    """Of the pixels of one image that take part, in ascending pixel index: ``(p, z, a_s, a_t)``."""
    depth = view.depth.cpu().to(torch.float32)
    H, W = depth.shape
    J = J.cpu()
    ok = (depth > 0) & ~torch.isnan(J).any(dim=2)
    v, u = torch.where(ok)
    d = depth[v, u].numpy()
    Kinv = getattr(view, 'Kinv', None)
    Kinv = view.K.cpu().to(torch.float32).inverse() if Kinv is None else Kinv.cpu().to(torch.float32).view(3, 3)
    R, t = view.R.cpu().to(torch.float32).numpy(), view.t.cpu().to(torch.float32).numpy().reshape(3)
    A = torch.as_tensor(axes).cpu().to(torch.float32).view(3, 3).numpy()
    half = np.float32(0.5)
    x, y, w = d * (u.numpy().astype(np.float32) + half), d * (v.numpy().astype(np.float32) + half), d * np.float32(1.0)   # d * rays
    cP = [dot3(Kinv.numpy()[r], x, y, w) for r in range(3)]                                      # K^-1 @ (d * rays)
    z = np.sqrt((cP[0] * cP[0] + cP[1] * cP[1]) + cP[2] * cP[2])                                 # the engine's range chain
    wP = [dot3(R[r], cP[0], cP[1], cP[2]) + t[r] for r in range(3)]                              # R @ cP + t
    a_s, a_t = dot3(A[0], wP[0], wP[1], wP[2]), dot3(A[1], wP[0], wP[1], wP[2])                  # axes @ wP
    assert all(q.dtype == np.float32 for q in (x, z, wP[0], a_s, a_t))
    # the reference's expressions, by torch: the same numbers up to the last bits
    rays = torch.stack([u + 0.5, v + 0.5, torch.ones_like(u)])
    cP_t = Kinv @ (torch.from_numpy(d) * rays)
    a_ref = torch.from_numpy(A) @ (torch.from_numpy(R) @ cP_t + torch.from_numpy(t).view(3, 1))
    scale = float(np.abs(np.stack(wP)).max()) if len(d) else 0.0
    assert np.abs(np.stack([a_s, a_t]) - a_ref[:2].numpy()).max(initial=0.0) <= 8 * 2.0 ** -23 * scale
    assert (np.abs(z - cP_t.norm(dim=0).numpy()) <= 4 * 2.0 ** -23 * z).all()
    return (v * W + u).to(torch.int64), torch.from_numpy(z), torch.from_numpy(a_s), torch.from_numpy(a_t)


def bounds_of(views, Js, axes):
    """``(lo_s, lo_t, hi_s, hi_t)``: float32 min and max of the plane coordinates over all pixels that take part."""
    parts = [pixels(v, J, axes) for v, J in zip(views, Js)]
    a_s = torch.cat([p[2] for p in parts])
    a_t = torch.cat([p[3] for p in parts])
    return tuple(float(x) for x in (a_s.min(), a_t.min(), a_s.max(), a_t.max()))


def cells(lo, hi, gsd):
    return int((np.float32(hi) - np.float32(lo)) / np.float32(gsd)) + 1


def mosaic(views, Js, axes, gsd, bounds=None):
    """The mosaic of ``views`` (ordinal = position) as a dict of CPU tensors ``J, raw, source, pixel, range`` plus ``bounds``,
    ``Hm``, ``Wm`` and ``ties`` -- per filled cell the number of pixels that share the winner's range bits."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if bounds is None:
        bounds = bounds_of(views, Js, axes)
    lo_s, lo_t, hi_s, hi_t = (np.float32(x) for x in bounds)
    g = np.float32(gsd)
    Wm, Hm = cells(lo_s, hi_s, g), cells(lo_t, hi_t, g)
    rows = []
    for i, (view, J) in enumerate(zip(views, Js)):
        p, z, a_s, a_t = pixels(view, J, axes)
        qs, qt = torch.from_numpy((a_s.numpy() - lo_s) / g), torch.from_numpy((a_t.numpy() - lo_t) / g)    # float32, IEEE
        assert qs.dtype == torch.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].to(torch.int64) * Wm + qs[keep].to(torch.int64)     # Tensor.long(): truncation
        zbits = z[keep].contiguous().view(torch.int32).to(torch.int64)
        assert bool((zbits >= 0).all())    # z >= +0: the bits order like the values (0 itself: a subnormal depth, whose squares underflow)
        rows.append(torch.stack([cell, zbits, torch.full_like(cell, i), p[keep]], dim=1))
    rows = torch.cat(rows).numpy()
    order = np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))   # by cell, then (range bits, ordinal, pixel)
    rows = rows[order]
    first = np.ones(len(rows), bool)
    first[1:] = rows[1:, 0] != rows[:-1, 0]
    win = rows[first]
    same = np.zeros(Hm * Wm, np.int64)   # pixels of the cell with the winner's range bits
    start = np.flatnonzero(first)
    best_z = np.repeat(rows[start, 1], np.diff(np.append(start, len(rows))))
    np.add.at(same, rows[:, 0], (rows[:, 1] == best_z).astype(np.int64))
    out = {'J': torch.full((Hm * Wm, 3), float('nan'), dtype=torch.float32), 'raw': torch.zeros((Hm * Wm, 3), dtype=torch.uint8),
           'source': torch.full((Hm * Wm,), -1, dtype=torch.int32), 'pixel': torch.full((Hm * Wm,), -1, dtype=torch.int32),
           'range': torch.full((Hm * Wm,), float('nan'), dtype=torch.float32)}
    for i, (view, J) in enumerate(zip(views, Js)):
        mine = win[win[:, 2] == i]
        c, p = torch.from_numpy(mine[:, 0].copy()), torch.from_numpy(mine[:, 3].copy())
        out['J'][c] = J.cpu().reshape(-1, 3)[p]
        out['raw'][c] = view.rgb.cpu().reshape(-1, 3)[p]
        out['source'][c] = i
        out['pixel'][c] = p.to(torch.int32)
        out['range'][c] = torch.from_numpy(mine[:, 1].astype(np.int32).copy()).view(torch.float32)
    out = {k: v.reshape((Hm, Wm) + tuple(v.shape[1:])) for k, v in out.items()}
    out.update(bounds=tuple(float(x) for x in bounds), Hm=Hm, Wm=Wm, ties=torch.from_numpy(same).reshape(Hm, Wm))
    return out
