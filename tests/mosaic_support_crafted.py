"""The crafted survey of the supported surface's property test (test_mosaic_support_host.py, test_gpu_mosaic_support.py) -- not a
test.  One plane 2.0 m below three cameras that look straight down from slightly different places; in the depth map of ONE view a
rectangle lies 0.5 m nearer and has a colour of its own: the fish.  In its cells the fish is both the highest and the nearest
sample, so it wins the best view, and a plain-minimum surface test culls the seabed under it."""
from types import SimpleNamespace

import numpy as np
import torch

HW = (48, 64)
K = torch.tensor([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
GSD = 0.04                              # twice the median pixel footprint (sucre.mosaic_default_gsd of the survey)
PLANE, FISH = 2.0, 1.5                  # heights along the view axis: smaller is higher
FISH_VIEW = 1                           # its ordinal: neither the first image nor the last
PATCH = (slice(16, 32), slice(20, 44))  # rows, columns of the fish in its view
OFFSETS = ((0.0, 0.0), (0.013, -0.007), (-0.011, 0.009))     # the cameras' places in the plane, metres
FISH_COLOUR = (0.9, 0.1, 0.8)
TOL = 0.1


def survey(seed=9):
    """``(views, Js)`` as CPU tensors; ``R = I``, to be mosaicked with the identity as axes.  The plane's colours lie in
    [0.2, 0.6]; the fish's pixels hold ``FISH_COLOUR`` exactly."""
    H, W = HW
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for i, (tx, ty) in enumerate(OFFSETS):
        depth = torch.full((H, W), PLANE)
        J = (torch.rand((H, W, 3), generator=g) * 0.4 + 0.2).contiguous()
        if i == FISH_VIEW:
            depth[PATCH] = FISH
            J[PATCH] = torch.tensor(FISH_COLOUR)
        rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=depth, rgb=rgb, K=K.clone(), R=torch.eye(3), t=torch.tensor([[tx], [ty], [0.0]])))
        Js.append(J)
    return views, Js


def fish_pixels():
    """The pixel indices (v W + u) of the fish in its view, as a sorted int64 array."""
    H, W = HW
    mask = np.zeros((H, W), bool)
    mask[PATCH] = True
    return np.nonzero(mask.reshape(-1))[0].astype(np.int64)
