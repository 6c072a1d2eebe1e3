"""The crafted survey of the direct gain solve's property test (test_mosaic_gain_direct_host.py, test_gpu_mosaic_gain_direct.py) --
not a test.  The plane of mosaic_gains_crafted.py stretched into a CHAIN: ``N = 12`` cameras look straight down on one plane 2.0 m
below them from places ``STEP = 0.64`` m apart along x.  An image is 64 pixels of 0.02 m wide, so each view overlaps only its two
neighbours, by half its width (384 cells of 0.04 m per pair), and view i shares nothing with view i + 2.  Every image is one flat
colour, ``COLOUR`` times the image's factor ``RATIO^(i - 5.5)``: a slow exposure drift along a transect and nothing else.  Before any
solve the spread ``max |g_i k_i / (g_j k_j) - 1|`` is ``RATIO^11 - 1 = 0.71``.  The rounds need on the order of N^2 rounds for it
(8 rounds leave 0.468); one direct solve removes it.

The bound.  Every ``J`` is at least 0.35 x 1.05^-5.5 = 0.267 >= 0.25, so, as mosaic_gains_crafted.py derives, the exact minimiser
of the quantised objective makes two OVERLAPPING images agree to 6 x 2^-13 (the quantisation of Xq in the sums of either image
and of their common cells).  Along the chain the pairwise errors add: (N - 1) x 6 x 2^-13 = 8.1e-3 between its two ends.  The prior
mu = 2^-20 pulls every gain towards 1 with a weight that is 2^-20 of the data term; its share of the spread was measured on this
chain by comparing mu = 2^-20 with mu = 2^-30: 1.4e-5.  The gauge and float32 (2^-24) cancel or vanish in a ratio.  So
``BOUND = 2^-6 = 1.6e-2``, the next power of two above their sum; the restatement reaches 1.3e-4.
"""
from types import SimpleNamespace

import torch

import mosaic_gains_crafted as plane

N = 12
STEP = 0.64
RATIO = 1.05
HW, K, GSD, PLANE, COLOUR = plane.HW, plane.K, plane.GSD, plane.PLANE, plane.COLOUR
FACTORS = tuple(RATIO ** (i - (N - 1) / 2) for i in range(N))
LIMIT = 2.0
BOUND = 2.0 ** -6
ROUNDS_LEFT = 0.4       # 8 rounds of the relaxation leave a spread above this (0.468 measured with the restatement)


def survey(seed=7):
    """``(views, Js)`` as CPU tensors; ``R = I``, ``t = (STEP i, 0, 0)``, to be mosaicked with the identity as axes."""
    H, W = HW
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for i, k in enumerate(FACTORS):
        rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=torch.full((H, W), PLANE), rgb=rgb, K=K.clone(), R=torch.eye(3),
                                     t=torch.tensor([[STEP * i], [0.0], [0.0]])))
        Js.append((torch.tensor(COLOUR) * torch.tensor(k, dtype=torch.float32)).expand(H, W, 3).contiguous())
    return views, Js


def spread(gains):
    """``max |g_i k_i / (g_j k_j) - 1|`` over the images and channels of (N,3) gains, in float64."""
    gk = torch.as_tensor(gains).double() * torch.tensor(FACTORS, dtype=torch.float64)[:, None]
    return float((gk[:, None, :] / gk[None, :, :] - 1).abs().max())


def fan(n, shift, seed=11):
    """``(views, Js)`` as CPU tensors for the overflow rule: ``n`` views of 20 x 24 pixels of the plane, random colours with a NaN
    patch and a hole in the depth each, view i moved by ``shift`` i metres along x.  An image is 0.48 m wide, so a cell in the
    middle is reached by about ``0.48 / shift`` images and a cell near either end by few: with more than eight in the middle the
    request has overflowed cells, shared cells that did not overflow, and cells of one image."""
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for i in range(n):
        depth = torch.full((20, 24), PLANE)
        depth[int(torch.randint(0, 20, (1,), generator=g)), int(torch.randint(0, 24, (1,), generator=g))] = 0.0
        J = torch.rand((20, 24, 3), generator=g) * 1.2 + 0.05
        J[3 + i % 5, 2:6] = float('nan')
        rgb = torch.randint(0, 256, (20, 24, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=depth, rgb=rgb, K=torch.tensor([[100.0, 0.0, 12.0], [0.0, 100.0, 10.0], [0.0, 0.0, 1.0]]),
                                     R=torch.eye(3), t=torch.tensor([[shift * i], [0.0], [0.0]])))
        Js.append(J)
    return views, Js
