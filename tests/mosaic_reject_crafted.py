"""The crafted survey of the colour consensus' property test (test_mosaic_reject_host.py, test_gpu_mosaic_reject.py) -- not a test.
The geometry of mosaic_support_crafted.py -- one plane 2.0 m below three cameras that look straight down from slightly different
places -- but the depth is the plane's EVERYWHERE: the fish of view 1 is not in its depth map, as a transient object is not in a
depth map rendered from the reconstruction.  It has the seabed's height and its own colour, so no height test can see it
(``surface=0.1, support=2`` culls nothing), it is as near as the plane, and it wins best-view cells.

By construction: every image holds the constant plane colour, so the plane means of a cell tie exactly and order by ordinal; an
image with a fish sample in a cell has the strictly largest brightness there (0.9 + 0.1 + 0.8 > 3 x 0.4); so where the three views
overlap the reference is view 0 or 2, never the fish's view, and it is the plane colour to within half a step of the 2^-14
quantiser: a plane sample differs from it by at most 2^-15 and a fish sample by 0.5 - 2^-15 or more in the red channel."""
from types import SimpleNamespace

import numpy as np
import torch

import mosaic_support_crafted as geometry

HW, K, GSD, PLANE, FISH_VIEW, PATCH, OFFSETS, FISH_COLOUR = (geometry.HW, geometry.K, geometry.GSD, geometry.PLANE, geometry.FISH_VIEW,
                                                             geometry.PATCH, geometry.OFFSETS, geometry.FISH_COLOUR)
PLANE_COLOUR = (0.4, 0.4, 0.4)
TOL = 0.15
N_FISH = 16 * 24            # the samples of the patch


def survey(seed=9):
    """``(views, Js)`` as CPU tensors; ``R = I``, to be mosaicked with the identity as axes."""
    H, W = HW
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for i, (tx, ty) in enumerate(OFFSETS):
        J = torch.tensor(PLANE_COLOUR).repeat(H, W, 1).contiguous()
        if i == FISH_VIEW:
            J[PATCH] = torch.tensor(FISH_COLOUR)
        rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=torch.full((H, W), PLANE), rgb=rgb, K=K.clone(), R=torch.eye(3),
                                     t=torch.tensor([[tx], [ty], [0.0]])))
        Js.append(J)
    return views, Js


def fish_mask():
    """(H,W) bool: the fish's pixels in its view."""
    mask = np.zeros(HW, bool)
    mask[PATCH] = True
    return mask
