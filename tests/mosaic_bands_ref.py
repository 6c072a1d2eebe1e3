"""CPU restatement of the multi-band mosaic blend (csrc/bands.h), helper of test_mosaic_bands_host.py and
test_gpu_mosaic_bands.py -- not a test.  It shares no code with the engine: the band stack is numpy float32 arithmetic on shifted
arrays, one IEEE operation per line; the plan is written out again; every band's accumulator comes from tests/mosaic_blend_ref.py
or tests/mosaic_feather_ref.py with the band as the images' J (they are imported, not changed); the combine divides in float64
and adds in float32.  test_mosaic_bands_host.py checks the stack against plain per-pixel loops over the definition.
"""
from types import SimpleNamespace

import numpy as np
import torch

import mosaic_blend_ref as bref
import mosaic_feather_ref as fref
import mosaic_ref as ref

ACC_WORDS = bref.ACC_WORDS
BANDS_RANGE = (1, 6)


def clamped(J):
    """S_0 wherever it is defined: ``min(max(J, -1024), 1024)`` in float32 (an infinity becomes finite, a NaN stays)."""
    J = np.asarray(J, np.float32)
    lo = np.maximum(J, np.float32(-1024))
    return np.minimum(lo, np.float32(1024))


def shifted(x, du, dv):
    """``y(u, v) = x(u + du, v + dv)`` for an (H,W,...) array, +0 where that lies outside it."""
    H, W = x.shape[:2]
    y = np.zeros_like(x)
    us, vs = slice(max(0, -du), min(W, W - du)), slice(max(0, -dv), min(H, H - dv))
    if us.start < us.stop and vs.start < vs.stop:
        y[vs, us] = x[vs.start + dv:vs.stop + dv, us.start + du:us.stop + du]
    return y


def smooth(S, member, s):
    """One level: S_(j+1) from S_j ((H,W,3) float32, any value at a non-member) with the step ``s``; NaN at a non-member."""
    two = np.float32(2)
    a = np.where(member[:, :, None], S, np.float32(0)).astype(np.float32)      # +0.0f elsewhere
    m = member.astype(np.int64)
    t = two * a
    l = shifted(a, -s, 0) + t
    Nh = l + shifted(a, s, 0)
    Ah = (shifted(m, -s, 0) + 2 * m) + shifted(m, s, 0)
    t = two * Nh
    l = shifted(Nh, 0, -s) + t
    N = l + shifted(Nh, 0, s)
    A = (shifted(Ah, 0, -s) + 2 * Ah) + shifted(Ah, 0, s)
    assert all(q.dtype == np.float32 for q in (a, Nh, N)) and int(A.max(initial=0)) <= 16
    assert bool((A[member] >= 4).all())
    with np.errstate(invalid='ignore', divide='ignore'):
        out = N / A.astype(np.float32)[:, :, None]
    assert out.dtype == np.float32
    return np.where(member[:, :, None], out, np.float32(np.nan)).astype(np.float32)


def stack(depth, J, K):
    """The K + 1 (H,W,3) float32 arrays ``D_0 .. D_(K-1), S_K`` of an image; NaN in all three channels at a non-member."""
    depth, J = np.asarray(depth, np.float32), np.asarray(J, np.float32)
    K = int(K)
    assert BANDS_RANGE[0] <= K <= BANDS_RANGE[1]
    member = fref.members(depth, J)
    S = np.where(member[:, :, None], clamped(J), np.float32(np.nan)).astype(np.float32)
    out = []
    for j in range(K):
        nxt = smooth(S, member, 1 << j)
        with np.errstate(invalid='ignore'):
            D = S - nxt
        assert D.dtype == np.float32
        out.append(np.where(member[:, :, None], D, np.float32(np.nan)).astype(np.float32))
        S = nxt
    out.append(S)
    for band in out:
        assert np.array_equal(np.isnan(band), np.repeat(~member[:, :, None], 3, axis=2))      # NaN exactly at the non-members
    return out


def plan(H, F, K):
    """The K + 1 pairs ``(H_j, F_j)``, the finest band first and the residual, with the user's ``(H, F)``, last: float32
    ``H_j = max(H 2^(j-K), 1e-6)`` (an exact scaling) and ``F_j = max(F >> (K - j), 1)``, None without a feather."""
    H, K = np.float32(H), int(K)
    out = []
    for j in range(K):
        H_j = H * np.float32(2.0 ** (j - K))
        assert H_j.dtype == np.float32
        out.append((max(H_j, np.float32(1e-6)), None if F is None else max(int(F) >> (K - j), 1)))
    return out + [(H, None if F is None else int(F))]


def band_accumulators(views, Js, axes, gsd, H, F, K, bounds=None, base=None, near=None):
    """``(acc_bands (K + 1, Hm Wm, 8) int64, base)``: band j of every image blended by the blend's (``F`` None) or the feather's
    restatement with ``plan(H, F, K)[j]``.  ``base``: ``mosaic_ref.mosaic`` of the TRUE images; ``near``: per image
    ``mosaic_feather_ref.nearest2`` of its members (the band's members are the image's)."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if base is None:
        base = ref.mosaic(views, Js, axes, gsd, bounds=bounds)
    if F is not None and near is None:
        near = [fref.nearest2(fref.members(v.depth.cpu().numpy(), J.cpu().numpy())) for v, J in zip(views, Js)]
    stacks = [stack(v.depth.cpu().numpy(), J.cpu().numpy(), K) for v, J in zip(views, Js)]
    accs = []
    for j, (H_j, F_j) in enumerate(plan(H, F, K)):
        band = [torch.from_numpy(st[j]) for st in stacks]
        if F_j is None:      # (the blend's normalise pass asserts the unfeathered bound, wsum >= 4096: it holds for a band too)
            accs.append(bref.blend(views, band, axes, gsd, H_j, base=base)['acc'])
        else:
            accs.append(fref.blend(views, band, axes, gsd, H_j, F_j, base=base, near=near)['acc'])
    return torch.stack(accs), base


def combine(acc_bands, Hm, Wm, least=4):
    """``J_multiband`` (Hm,Wm,3) float32 from the K + 1 accumulators: every band's float64 quotient rounded to float32, added in
    float32 from the residual (the last slice) to the finest band; NaN where the residual has no sample."""
    acc = np.asarray(acc_bands, np.int64)
    n_bands = acc.shape[0]
    filled = acc[-1, :, 7] > 0
    J = np.full((Hm * Wm, 3), np.nan, np.float32)
    total = None
    for j in range(n_bands - 1, -1, -1):
        wsum = acc[j, filled, 6]
        assert bool((wsum >= least).all())       # the winner of a cell has t = 1 in every band, and f >= 1 / 1024
        B = ((acc[j, filled, 0:3].astype(np.float64) / wsum.astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32)
        total = B if total is None else total + B
        assert total.dtype == np.float32
    J[filled] = total
    return torch.from_numpy(J).reshape(Hm, Wm, 3)


def multiband(views, Js, axes, gsd, H, F, K, bounds=None, base=None, near=None):
    """``{'acc_bands', 'J_multiband', 'base'}`` of the request."""
    acc, base = band_accumulators(views, Js, axes, gsd, H, F, K, bounds=bounds, base=base, near=near)
    return {'acc_bands': acc, 'J_multiband': combine(acc.numpy(), base['Hm'], base['Wm']), 'base': base}


# ---- the crafted pair of the frequency property -------------------------------------------------------------------------------------
PAIR_HW = (48, 64)
PAIR_GSD = 2.0 ** -5          # one pixel's footprint of either view: 2 / 64 = 2.5 / 80
PAIR_H, PAIR_K = 2.0, 4       # the blend depth (the ranges differ by at most 0.5 m) and the detail bands
PAIR_OFFSET, PAIR_NOISE = 0.2, 0.15
PAIR_BOUNDS = (-1.0, -0.75, 1.0 - 2.0 ** -6, 0.75 - 2.0 ** -6)     # the plane coordinates of the pixel centres' cells: 64 x 48


def frequency_pair():
    """One plane seen from two altitudes through cameras whose pixels have the same footprint on it, so that pixel (u, v) of
    either view lands in the middle of cell (v, u): A from 2.0 m (f = 64), clean; B from 2.5 m (f = 80, moved back along the axis),
    its colour ``PAIR_OFFSET`` too high with ``PAIR_NOISE`` of uniform pixel noise either way.  Both cover every cell once.
    ``(views, Js)`` as CPU tensors."""
    H, W = PAIR_HW
    g = torch.Generator().manual_seed(7)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    x, y = (u + 0.5 - W / 2) / 32, (v + 0.5 - H / 2) / 32                      # the plane point of a pixel, metres
    clean = torch.stack([0.4 + 0.05 * torch.sin(2.0 * x + c) * torch.cos(1.5 * y - c) for c in (0.0, 1.0, 2.0)], dim=2)
    views, Js = [], []
    for f, d, J in ((64.0, 2.0, clean), (80.0, 2.5, clean + PAIR_OFFSET + PAIR_NOISE * (2 * torch.rand((H, W, 3), generator=g) - 1))):
        K = torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])
        Kinv = torch.tensor([[1 / f, 0.0, -W / 2 / f], [0.0, 1 / f, -H / 2 / f], [0.0, 0.0, 1.0]])
        rgb = (J.clamp(0, 1) * 255).to(torch.uint8)
        views.append(SimpleNamespace(depth=torch.full((H, W), d), rgb=rgb, K=K, R=torch.eye(3), t=torch.tensor([[0.0], [0.0], [2.0 - d]]),
                                     Kinv=Kinv))
        Js.append(J.to(torch.float32).contiguous())
    return views, Js


def hf(x, margin=2):
    """The fine detail of a picture (Hm,Wm,3): the mean absolute difference from the 3 x 3 box mean over the interior cells
    (float64); every cell of the interior and of its neighbourhood must be filled."""
    x = np.asarray(x, np.float64)
    assert not np.isnan(x).any()
    box = sum(x[1 + dy:x.shape[0] - 1 + dy, 1 + dx:x.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    d = np.abs(x[1:-1, 1:-1] - box)
    return float(d[margin - 1:d.shape[0] - margin + 1, margin - 1:d.shape[1] - margin + 1].mean())


def lf(x, margin=8):
    """The colour of a picture: the mean over the interior window ``margin`` cells inside (float64)."""
    x = np.asarray(x, np.float64)
    return float(x[margin:x.shape[0] - margin, margin:x.shape[1] - margin].mean())


def frequency_conditions(J, J_blend, J_multiband):
    """``(hf of the three, lf of the three, the two conditions)``: multi-band has less fine detail than the midpoint of best view and
    blend, and its colour is within a tenth of the blend's distance from the best view's."""
    h = [hf(p) for p in (J, J_blend, J_multiband)]
    l = [lf(p) for p in (J, J_blend, J_multiband)]
    return h, l, (h[2] < (h[0] + h[1]) / 2, abs(l[2] - l[1]) < 0.1 * abs(l[1] - l[0]))
