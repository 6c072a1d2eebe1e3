"""The operation in plain float64 numpy: SUCRe.update_J (sucre.py:66-82) and sucre.adam (sucre.py:124-157) restated once more,
as oracle/ restates them in float32 -- what the float32 oracle and the HIP engine are both measured against in
tests/crafted.py.  Samples are the oracle's: per kept view (u1 int16[n], v1 int16[n], cP float32[3,n], I float32[3,n])."""
import numpy as np


def _flat(H, W, samples):
    """All views' observations as float64 arrays: pixel index, range z = ||cP||, colours (n, 3)."""
    if not samples:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3))
    px = np.concatenate([v.astype(np.int64) * W + u.astype(np.int64) for u, v, _, _ in samples])
    z = np.concatenate([np.sqrt((np.asarray(cP, np.float64) ** 2).sum(axis=0)) for _, _, cP, _ in samples])
    I = np.concatenate([np.asarray(I, np.float64).T for _, _, _, I in samples])
    return px, z, I


def _solve_J(npx, px, z, I, p):
    B, beta, gamma = p[0:3], p[3:6], p[6:9]
    a = np.exp(-beta[None, :] * z[:, None])
    y = I - B[None, :] * (1.0 - np.exp(-gamma[None, :] * z[:, None]))
    num, den = np.zeros((npx, 3)), np.zeros((npx, 3))
    np.add.at(num, px, y * a)
    np.add.at(den, px, a * a)
    with np.errstate(invalid='ignore', divide='ignore'):
        return num / den        # 0/0 = NaN where a pixel has no observation


def closed_form_J(H, W, samples, params):
    """J = sum y a / sum a^2 with y = I - B (1 - e^(-gamma z)), a = e^(-beta z): (H,W,3) float64, NaN without observation."""
    px, z, I = _flat(H, W, samples)
    return _solve_J(H * W, px, z, I, np.asarray(params, np.float64).reshape(9)).reshape(H, W, 3)


def adam_fit(H, W, samples, J0, params0, T, lr=0.05, use_closed_form=False, betas=(0.9, 0.999), eps=1e-8):
    """T full-batch Adam iterations on {B, beta, gamma, J} for L = sum r^2 / (3 n_obs), torch's update (bias corrections,
    eps outside the square root).  Closed-form mode: J is re-solved at the top of every iteration and after the last, and takes
    no step.  Returns (J (H,W,3), parameters (9,), trace (T,10): the cost sum r^2 before the step, the parameters after it)."""
    px, z, I = _flat(H, W, samples)
    npx, n_obs = H * W, len(px)
    p = np.asarray(params0, np.float64).reshape(9).copy()
    J = np.zeros((npx, 3)) if J0 is None else np.asarray(J0, np.float64).reshape(npx, 3).copy()
    mp, vp, mJ, vJ = np.zeros(9), np.zeros(9), np.zeros((npx, 3)), np.zeros((npx, 3))
    trace = np.zeros((T, 10))
    b1, b2 = betas
    for it in range(1, T + 1):
        if use_closed_form:
            J = _solve_J(npx, px, z, I, p)
        B, beta, gamma = p[0:3], p[3:6], p[6:9]
        a, g = np.exp(-beta[None, :] * z[:, None]), np.exp(-gamma[None, :] * z[:, None])
        Jo = J[px]
        r = I - (Jo * a + B[None, :] * (1.0 - g))
        dr = -2.0 * r / (3.0 * n_obs)
        gp = np.concatenate([(dr * (1.0 - g)).sum(axis=0), (dr * Jo * a * -z[:, None]).sum(axis=0),
                             (dr * B[None, :] * g * z[:, None]).sum(axis=0)])
        gJ = np.zeros((npx, 3))
        np.add.at(gJ, px, dr * a)
        trace[it - 1, 0] = (r * r).sum()
        bc1, bc2 = 1.0 - b1 ** it, 1.0 - b2 ** it
        mp += (1.0 - b1) * (gp - mp)
        vp = b2 * vp + (1.0 - b2) * gp * gp
        p = p - (lr / bc1) * mp / (np.sqrt(vp) / np.sqrt(bc2) + eps)
        if not use_closed_form:
            mJ += (1.0 - b1) * (gJ - mJ)
            vJ = b2 * vJ + (1.0 - b2) * gJ * gJ
            J = J - (lr / bc1) * mJ / (np.sqrt(vJ) / np.sqrt(bc2) + eps)
        trace[it - 1, 1:] = p
    if use_closed_form:
        J = _solve_J(npx, px, z, I, p)
    return J.reshape(H, W, 3), p, trace
