"""The crafted survey of the gain compensation's property test (test_mosaic_gains_host.py, test_gpu_mosaic_gains.py) -- not a test.
One plane 2.0 m below three cameras that look straight down from ONE place, so every cell holds the same pixels of all three
views; every image is one flat colour, ``COLOUR`` times the image's factor ``FACTORS[i]``: the views disagree by known gains and by
nothing else.  After one round the products ``gain x factor`` of the three images must agree, up to the quantisation of the sums.

The bound.  Every ``J`` is at least 0.25 in every channel, so ``Xq = rint(16384 J) >= 4096`` carries a relative error of at most
2^-13, and so does ``Mq`` (the mean lies between the images).  A gain ``sum Xq Mq / sum Xq Xq`` over identical samples is
``Mq / Xq``: at most 3 x 2^-13 relative error to first order (one for Mq, two for the Xq of numerator and denominator against the
exact ratio), and a ratio of two gains 6 x 2^-13 < 2^-10.  The gauge and the float32 rounding (2^-24) cancel or vanish in the ratio.
"""
from types import SimpleNamespace

import torch

HW = (48, 64)
K = torch.tensor([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
GSD = 0.04                              # twice the pixel footprint at 2 m
PLANE = 2.0
COLOUR = (0.4, 0.5, 0.35)               # times the smallest factor: 0.28 >= 0.25 in every channel
FACTORS = (0.8, 1.0, 1.25)
LIMIT = 2.0
BOUND = 2.0 ** -10


def survey(seed=5):
    """``(views, Js)`` as CPU tensors; ``R = I``, ``t = 0``, to be mosaicked with the identity as axes."""
    H, W = HW
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for k in FACTORS:
        rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=torch.full((H, W), PLANE), rgb=rgb, K=K.clone(), R=torch.eye(3), t=torch.zeros(3, 1)))
        Js.append((torch.tensor(COLOUR) * torch.tensor(k, dtype=torch.float32)).expand(H, W, 3).contiguous())
    return views, Js


def spread(gains):
    """``max |g_i k_i / (g_j k_j) - 1|`` over the images and channels of (n,3) gains, in float64."""
    gk = torch.as_tensor(gains).double() * torch.tensor(FACTORS, dtype=torch.float64)[:, None]
    return float((gk[:, None, :] / gk[None, :, :] - 1).abs().max())
