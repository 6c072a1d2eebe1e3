"""Float64 numpy references for the uncertainty pass (sucre_fit_uncertainty*, engine.water_uncertainty, engine.j_standard_error).

Per observation and channel, at float32 J, B, beta, gamma, z and I promoted to float64 (sucre.py:79-82, 144):

    a = exp(-beta z), g = exp(-gamma z);  dJ = a, dB = 1 - g, dbeta = -J z a, dgamma = B z g;  r = I - (J a + B dB)

``restatement``: the cancellation-free form the device is held to.  Sweep 1 gives A_p = sum dJ^2 and k_p = sum dJ d / A_p per pixel;
sweep 2 sums the products of e = d - k_p dJ -- the part of d = (dB, dbeta, dgamma) that is orthogonal to the pixel's own J column --
H = sum e e^T.  The device (and ``one_pass``) forms H = sum d d^T - sum_p b_p b_p^T / A_p instead, a 30-65x cancellation.

``dense``: the check of the formulas themselves -- the full N x (P + 3) Jacobian of one channel, s^2 (J^T J)^-1, its last three rows
and columns and the diagonal of its first P.
"""
import numpy as np

WORDS = 24


def flatten(samples, W, u16mm=False):
    """(px (N,) int64, z (N,) float32, I (N,3) float32) of the oracle's samples [(u1, v1, cP (3,n), I (3,n))], view after view.  z is
    the float32 range the store holds (sucre.py:53); ``u16mm``: the one the fit of a u16mm store reads."""
    px, zs, Is = [], [], []
    for u1, v1, cP, I in samples:
        cP = np.asarray(cP, np.float32)
        z = np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2])
        assert z.dtype == np.float32
        px.append(np.asarray(v1, np.int64) * W + np.asarray(u1, np.int64))
        zs.append(z)
        Is.append(np.asarray(I, np.float32).T)
    z = np.concatenate(zs)
    if u16mm:
        z = np.clip(np.rint(z * np.float32(1000.0)), np.float32(1.0), np.float32(65535.0)) * np.float32(0.001)
        assert z.dtype == np.float32
    return np.concatenate(px), z, np.concatenate(Is)


def derivatives(px, z, I, J, params):
    """dJ, dB, dbeta, dgamma, r: (N,3) float64 each."""
    p = np.asarray(params, np.float32).astype(np.float64)
    B, beta, gamma = p[0:3], p[3:6], p[6:9]
    z = np.asarray(z, np.float32).astype(np.float64)[:, None]
    Jo = np.asarray(J, np.float32).reshape(-1, 3).astype(np.float64)[px]
    a, g = np.exp(-beta * z), np.exp(-gamma * z)
    dB = 1.0 - g
    r = np.asarray(I, np.float32).astype(np.float64) - (Jo * a + B * dB)
    return a, dB, -Jo * z * a, B * z * g, r


def _pixel_sums(px, npx, x):
    out = np.zeros((npx,) + x.shape[1:])
    np.add.at(out, px, x)
    return out


def finish(Hm, SSR, N, P):
    """cov (3,3,3), se (3,3), s2 (3,) from the normal matrices: H scaled by its diagonal, inverted, scaled back."""
    dof = N - P - 3
    s2 = SSR / dof
    cov = np.empty((3, 3, 3))
    for c in range(3):
        d = np.sqrt(np.diag(Hm[c]))
        cov[c] = s2[c] * np.linalg.inv(Hm[c] / np.outer(d, d)) / np.outer(d, d)
    with np.errstate(invalid='ignore'):   # (a garbage H -- float32 sums -- may leave a negative variance: NaN)
        return cov, np.sqrt(np.einsum('cii->ci', cov)), s2


def _package(count, A, k, Hm, SSR, H, W):
    N, P = int(count.sum()), int((count > 0).sum())
    seen = count > 0
    jterms = np.zeros((H * W, 3, 4))
    jterms[seen, :, 0] = 1.0 / A[seen]
    jterms[seen, :, 1:] = k[seen]
    sums = np.zeros(WORDS)
    sums[0], sums[1] = N, P
    for c in range(3):
        sums[3 + 7 * c:10 + 7 * c] = [Hm[c, 0, 0], Hm[c, 0, 1], Hm[c, 0, 2], Hm[c, 1, 1], Hm[c, 1, 2], Hm[c, 2, 2], SSR[c]]
    out = dict(count=count.reshape(H, W), jterms=jterms.reshape(H, W, 3, 4), H=Hm, SSR=SSR, N=N, P=P, sums=sums)
    if N - P - 3 > 0:
        cov, se, s2 = finish(Hm, SSR, N, P)
        var = s2 * jterms[..., 0] + np.einsum('pci,cij,pcj->pc', jterms[..., 1:], cov, jterms[..., 1:])
        with np.errstate(invalid='ignore'):
            J_se = np.where(seen[:, None], np.sqrt(var), np.nan)
        out.update(cov=cov, se=se, s2=s2, J_se=J_se.reshape(H, W, 3))
    return out


def restatement(px, z, I, J, params, H, W):
    """The cancellation-free two-sweep form."""
    npx = H * W
    dJ, dB, db, dg, r = derivatives(px, z, I, J, params)
    d = np.stack([dB, db, dg], axis=-1)                      # (N,3 channels,3 parameters)
    count = np.bincount(px, minlength=npx)
    A = _pixel_sums(px, npx, dJ * dJ)                        # sweep 1
    b = _pixel_sums(px, npx, dJ[..., None] * d)
    with np.errstate(invalid='ignore', divide='ignore'):
        k = np.where((count > 0)[:, None, None], b / A[..., None], 0.0)
    e = d - k[px] * dJ[..., None]                            # sweep 2
    Hm = np.einsum('nci,ncj->cij', e, e)
    return _package(count, A, k, Hm, (r * r).sum(axis=0), H, W)


def one_pass(px, z, I, J, params, H, W, dtype=np.float64):
    """The device's form, H = sum d d^T - sum_p b_p b_p^T / A_p, with the sums held in ``dtype``."""
    npx = H * W
    dJ, dB, db, dg, r = [x.astype(dtype) for x in derivatives(px, z, I, J, params)]
    d = np.stack([dB, db, dg], axis=-1)
    count = np.bincount(px, minlength=npx)
    A = _pixel_sums(px, npx, dJ * dJ).astype(dtype)
    b = _pixel_sums(px, npx, dJ[..., None] * d).astype(dtype)
    seen = count > 0
    k = np.zeros_like(b)
    k[seen] = b[seen] / A[seen][..., None]
    S = np.zeros((3, 3, 3), dtype)
    for n in range(0, len(px), 4096):    # (running sums in ``dtype``, as an accumulator would hold them)
        S = (S + np.einsum('nci,ncj->cij', d[n:n + 4096], d[n:n + 4096]).astype(dtype)).astype(dtype)
    Hm = (S - np.einsum('pci,pcj->cij', k[seen], b[seen]).astype(dtype)).astype(np.float64)
    return _package(count, A.astype(np.float64), k.astype(np.float64), Hm, (r * r).sum(axis=0).astype(np.float64), H, W)


def scaled_distance(H_got, H_ref):
    """max over the channels of ||D (H_got - H_ref) D||_F / ||D H_ref D||_F with D = diag(H_ref)^-1/2."""
    worst = 0.0
    for c in range(3):
        d = np.sqrt(np.diag(H_ref[c]))
        s = np.outer(d, d)
        worst = max(worst, float(np.linalg.norm((H_got[c] - H_ref[c]) / s) / np.linalg.norm(H_ref[c] / s)))
    return worst


def normal_of(sums):
    """(3,3,3) H and (3,) SSR from the 24 words."""
    sums = np.asarray(sums, np.float64)
    Hm, SSR = np.empty((3, 3, 3)), np.empty(3)
    for c in range(3):
        hBB, hBb, hBg, hbb, hbg, hgg, SSR[c] = sums[3 + 7 * c:10 + 7 * c]
        Hm[c] = [[hBB, hBb, hBg], [hBb, hbb, hbg], [hBg, hbg, hgg]]
    return Hm, SSR


def dense(px, z, I, J, params, H, W):
    """The full Jacobian per channel: columns = the J of the P observed pixels, then B, beta, gamma.  Returns se (3,3) and J_se (H,W,3)
    from s^2 (J^T J)^-1 with s^2 = SSR / (N - P - 3); the columns are scaled to unit length before the inversion."""
    npx = H * W
    dJ, dB, db, dg, r = derivatives(px, z, I, J, params)
    count = np.bincount(px, minlength=npx)
    cols = np.cumsum(count > 0) - 1                          # pixel -> column
    N, P = len(px), int((count > 0).sum())
    se, J_se = np.empty((3, 3)), np.full((npx, 3), np.nan)
    rows = np.arange(N)
    for c in range(3):
        Jac = np.zeros((N, P + 3))
        Jac[rows, cols[px]] = dJ[:, c]
        Jac[:, P], Jac[:, P + 1], Jac[:, P + 2] = dB[:, c], db[:, c], dg[:, c]
        norm = np.sqrt((Jac * Jac).sum(axis=0))
        Jn = Jac / norm
        cov = np.linalg.inv(Jn.T @ Jn) / np.outer(norm, norm) * ((r[:, c] ** 2).sum() / (N - P - 3))
        sd = np.sqrt(np.diag(cov))
        se[c] = sd[P:]
        J_se[count > 0, c] = sd[:P]
    return se, J_se.reshape(H, W, 3)
