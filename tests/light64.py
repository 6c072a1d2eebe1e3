"""The light model's cost and gradient in plain torch float64, differentiated by autograd: the yardstick the analytic gradients
of the CPU oracle (oracle_fit_light) and of the HIP engine (csrc/light.hip) are both measured against.

Written from the reference's formulas (sucre.py:52-64, 66-82, 141-146; se3.py:22-27), not from either implementation:

    R, t = matrix_exp(hat(cam2light));  Sigma = sigma^T sigma;  lP = R cP + t;  lp = lP.xy / lP.z
    l = exp(-lp^T Sigma^-1 lp / 2);  z = ||cP|| + ||lP||;  Ihat = l (J a + B (1 - g));  L = sum r^2 / (3 n_obs)

Samples are the oracle's: per kept view ``(u1 int16[n], v1 int16[n], cP float32[3,n], I float32[3,n])``.  An *image* is
``Image(H, W, samples, J0)``; several images share the 19 parameters (B, beta, gamma, cam2light[6], sigma[4] row-major) and one
n_obs, each keeps its own J (engine.HipWaterGroup).

How a gradient is read through a public interface.  Adam's first step is ``p0 - lr g / (|g| + eps)`` for any betas (m_hat = g,
sqrt(v_hat) = |g|): ``step64``.  With eps several times the largest |g| that is an almost linear, invertible image of g, so ONE
iteration at ``LR, EPS`` from a chosen point shows every component of the gradient in the parameters and in J after it; the
parameters after such a step mean nothing, only the step is read.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

LR, EPS = 1024.0, 1.0        # powers of two; EPS >= 4 max |g64| over every point below (asserted where a step is read)
GROUPS = (('water', slice(0, 9)), ('twist', slice(9, 15)), ('sigma', slice(15, 19)))
ROLL = 11                     # cam2light's rotation about the optical axis: its gradient is 0 by symmetry at 'start'

WATER = [.094, .121, .119, .321, .073, .072, .140, .137, .142]     # tests/test_gpu_invert.py::WATER (asserted equal there)
_SIGMA = [0.9, 0.1, -0.05, 1.1]


def _point(twist):
    return np.array(WATER + list(twist) + _SIGMA, np.float32)


# every twist turns mostly about the optical axis: the lamp keeps lighting the scene (l in [0.38, 1], lP.z >= 2 on the 48x32 scene)
POINTS = {
    'start': np.array([0.1] * 9 + [0.0] * 6 + [1.0, 0.0, 0.0, 1.0], np.float32),   # the reference's start (sucre.py:41-46)
    'small': _point((.02, -.03, .01, .05, -.04, .03)),        # series branch of se3_coefficients, Q != 0
    'below': _point((.3, -.2, .3464, .2, -.1, .05)),          # theta^2 = 0.24999: the last of the series
    'above': _point((.3, -.2, .3467, .2, -.1, .05)),          # theta^2 = 0.2502: the first of the trigonometric branch
    'roll2': _point((.1, -.15, 2.0, .2, -.1, .05)),           # theta ~ 2
    'roll3': _point((.05, .02, 3.1, .3, .2, -.1)),            # theta ~ pi: A = sin(theta) / theta ~ 0
}
TWISTED = ('small', 'below', 'above', 'roll2', 'roll3')


@dataclass
class Image:
    H: int
    W: int
    samples: list
    J0: np.ndarray | None = None      # (H,W,3) float32, NaN where the target has no depth; None in closed-form mode

    def n_obs(self):
        return int(sum(len(s[0]) for s in self.samples))


class _Obs:
    """One image's observations as float64 tensors."""

    def __init__(self, im):
        ss = [s for s in im.samples if len(s[0])]
        self.px = torch.from_numpy(np.concatenate([v.astype(np.int64) * im.W + u.astype(np.int64) for u, v, _, _ in ss]))
        self.cP = torch.from_numpy(np.concatenate([np.asarray(cP, np.float64) for _, _, cP, _ in ss], axis=1))    # (3, n)
        self.I = torch.from_numpy(np.concatenate([np.asarray(I, np.float64) for _, _, _, I in ss], axis=1))       # (3, n)
        self.npx = im.H * im.W


def se3_exp(xi):
    """se3.py:22-27 -- xi (..., 6) -> R (..., 3, 3), t (..., 3, 1)."""
    w1, w2, w3, p1, p2, p3 = xi.unbind(-1)
    zero = torch.zeros_like(w1)
    T = torch.stack([zero, -w3, w2, p1, w3, zero, -w1, p2, -w2, w1, zero, p3, zero, zero, zero, zero], dim=-1)
    T = torch.matrix_exp(T.reshape(xi.shape[:-1] + (4, 4)))
    return T[..., :3, :3], T[..., :3, 3:4]


def _l_z(p, cP, light):
    """compute_l_z (sucre.py:52-64) for p (19,) or, one parameter vector per observation, (n, 19)."""
    z = cP.norm(dim=0)
    if not light:
        return torch.ones_like(z), z
    R, t = se3_exp(p[..., 9:15])
    sigma = p[..., 15:19].reshape(p.shape[:-1] + (2, 2))
    Sinv = (sigma.transpose(-1, -2) @ sigma).inverse()
    if p.dim() == 1:
        lP = R @ cP + t
        lp = lP[:2] / lP[2]
        q = (lp * (Sinv @ lp)).sum(dim=0)
    else:
        lP = (R @ cP.T.unsqueeze(-1) + t).squeeze(-1).T
        lp = lP[:2] / lP[2]
        q = torch.einsum('in,nij,jn->n', lp, Sinv, lp)
    return torch.exp(-q / 2), z + lP.norm(dim=0)


def _col(p, k):
    """Parameters k..k+2 as (3, 1) or, per observation, (3, n)."""
    return p[k:k + 3].reshape(3, 1) if p.dim() == 1 else p[:, k:k + 3].T


def _residuals(p, J, ob, light):
    l, z = _l_z(p, ob.cP, light)
    B, beta, gamma = _col(p, 0), _col(p, 3), _col(p, 6)
    return ob.I - l * (J[ob.px].T * torch.exp(-beta * z) + B * (1 - torch.exp(-gamma * z)))      # sucre.py:79-82, 144


def _solve_J(p, ob, light):
    """update_J (sucre.py:66-77): (npx, 3), NaN where a pixel has no observation."""
    l, z = _l_z(p, ob.cP, light)
    a = l * torch.exp(-_col(p, 3) * z)
    b = l * _col(p, 0) * (1 - torch.exp(-_col(p, 6) * z))
    num = torch.zeros(ob.npx, 3, dtype=torch.float64).index_add_(0, ob.px, ((ob.I - b) * a).T)
    den = torch.zeros(ob.npx, 3, dtype=torch.float64).index_add_(0, ob.px, (a * a).T)
    return num / den


@dataclass
class Result:
    cost: float                 # sum r^2 over all images
    n_obs: int
    g: np.ndarray               # (19,) dL/dp; the ten light components are 0 without light
    gJ: list                    # per image (H,W,3) dL/dJ (zeros in closed-form mode, where J takes no step)
    J: list                     # per image (H,W,3) the J the gradient was taken at
    seen: list                  # per image (H,W) bool: the pixel has an observation
    abs_terms: np.ndarray | None = None   # (19,) sum over the observations of |d l_i / d p_k|, l_i = sum_c r_ic^2 / (3 n_obs)


def evaluate(images, params, light=True, closed=False, per_observation=False):
    """Cost, autograd gradient of the 19 parameters and of every image's J at ``params`` (cast to float64 from what they are).
    ``closed``: J is first solved in float64 (sucre.py:141) and is a constant of the gradient."""
    p = torch.tensor(np.asarray(params, np.float64).reshape(19), dtype=torch.float64, requires_grad=True)
    obs = [_Obs(im) for im in images]
    n_obs = int(sum(len(ob.px) for ob in obs))
    Js = []
    for im, ob in zip(images, obs):
        if closed:
            J = _solve_J(p.detach(), ob, light)
        else:
            J = torch.from_numpy(np.asarray(im.J0, np.float64).reshape(ob.npx, 3).copy())
        Js.append(J.requires_grad_(not closed))
    cost = sum((_residuals(p, J, ob, light) ** 2).sum() for J, ob in zip(Js, obs))
    (cost / n_obs / 3).backward()                                                    # sucre.py:145
    g = np.zeros(19) if p.grad is None else p.grad.numpy().copy()
    gJ = [(np.zeros((im.H, im.W, 3)) if J.grad is None else J.grad.numpy().reshape(im.H, im.W, 3).copy()) for im, J in zip(images, Js)]
    seen = [np.bincount(ob.px.numpy(), minlength=ob.npx).reshape(im.H, im.W) > 0 for im, ob in zip(images, obs)]
    res = Result(float(cost.detach()), n_obs, g, gJ, [J.detach().numpy().reshape(im.H, im.W, 3) for im, J in zip(images, Js)], seen)
    if per_observation:
        tot, acc = np.zeros(19), np.zeros(19)
        for J, ob in zip(Js, obs):
            P = p.detach().expand(len(ob.px), 19).clone().requires_grad_(True)        # one copy of the parameters per observation
            ((_residuals(P, J.detach(), ob, light) ** 2).sum() / n_obs / 3).backward()
            tot += P.grad.sum(dim=0).numpy()
            acc += P.grad.abs().sum(dim=0).numpy()
        assert np.abs(tot - g).max() <= 1e-12 * max(np.abs(g).max(), 1e-300), 'per-observation terms do not add up to the gradient'
        res.abs_terms = acc
    return res


def scene_image(scene, samples=None, J0=None):
    """The scene's target as an Image: the oracle's match lists and the J the reference starts from (sucre.py:47-49)."""
    import helpers
    from oracle import oracle
    if samples is None:
        _, samples = helpers.oracle_scene_samples(scene)
    if J0 is None:
        tgt = scene.views[scene.target]
        J0 = oracle.init_J(tgt.rgb_u8.numpy(), tgt.depth_f32().numpy())
    return Image(scene.height, scene.width, samples, J0)


def oracle_step(images, p0, closed, light=True, lr=LR, eps=EPS):
    """ONE iteration of the CPU oracle from ``p0``: (cost, parameters after it (19,) float64, per image J after it or None in
    closed-form mode).  Several images go side by side as one oracle problem -- a J per pixel, every parameter shared, one
    n_obs: the tied objective exactly; rows below a shorter image have no observation."""
    from oracle import oracle
    Hc, Wc = max(im.H for im in images), sum(im.W for im in images)
    samples, J0s, off = [], [], 0
    for im in images:
        samples += [((np.asarray(u, np.int64) + off).astype(np.int16), v, cP, I) for u, v, cP, I in im.samples]
        if not closed:
            J0s.append(np.concatenate([im.J0, np.full((Hc - im.H, im.W, 3), np.nan, np.float32)], axis=0))
        off += im.W
    J0 = None if closed else np.concatenate(J0s, axis=1)
    p0 = np.asarray(p0, np.float32)
    if light:
        J, p1, trace = oracle.fit_light(Hc, Wc, samples, J0, params0=p0, num_iter=1, lr=lr, use_closed_form=closed, eps=eps)
    else:
        J, p1, trace = oracle.fit(Hc, Wc, samples, J0, params0=p0[:9], num_iter=1, lr=lr, use_closed_form=closed, eps=eps)
        p1 = np.concatenate([p1, p0[9:]])
    Js, off = [], 0
    for im in images:
        Js.append(None if closed else J[:im.H, off:off + im.W])
        off += im.W
    return float(trace[0, 0]), p1.astype(np.float64), Js


def step64(p0, g, lr=LR, eps=EPS):
    """Adam's first step in float64, any betas."""
    p0, g = np.asarray(p0, np.float64), np.asarray(g, np.float64)
    return p0 - lr * g / (np.abs(g) + eps)


def delta64(g, lr=LR, eps=EPS):
    return step64(np.zeros_like(np.asarray(g, np.float64)), g, lr, eps)


def rounding_bar(p0, p1):
    """The float32 rounding of the step itself: 4 x 2^-24 x max(|p0|, |p1|), per component."""
    return 4.0 * 2.0 ** -24 * np.maximum(np.abs(np.asarray(p0, np.float64)), np.abs(np.asarray(p1, np.float64)))


def lane_sum_bar(res, lr=LR, eps=EPS):
    """What float32 accumulation and 1-ulp hardware reciprocals may move a step by: 2^-22 sum_obs |term_k| in the gradient,
    through the step's slope d/dg [lr g / (|g| + eps)] = lr eps / (|g| + eps)^2."""
    return 2.0 ** -22 * res.abs_terms * lr * eps / (np.abs(res.g) + eps) ** 2


def crafted_bar(d64, d_oracle, p0, extra=None):
    """The project's crafted rule per component: max(8 |oracle - float64|, float32 rounding of the step[, extra])."""
    p0 = np.asarray(p0, np.float64)
    bar = np.maximum(8.0 * np.abs(d_oracle - d64), rounding_bar(p0, p0 + d64))
    return bar if extra is None else np.maximum(bar, extra)
