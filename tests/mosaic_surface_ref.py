"""CPU restatement of the mosaic's surface test (csrc/surface.h), helper of test_mosaic_surface_host.py and
test_gpu_mosaic_surface.py -- not a test.  It shares no code with the engine: the geometry restates the reference's formulas with
tests/mosaic_ref.py's ``dot3`` / ``fma32`` (one IEEE float32 operation per line; ``heights`` asserts that its plane coordinates are
``mosaic_ref.pixels``' to the bit), the top of a cell is ``np.minimum.at`` over the order keys of the heights, the cull is one
float32 subtraction and one comparison, the counts are integer adds.  Every expected mosaic output is then one of the EXISTING
restatements (``mosaic_ref.mosaic``, ``mosaic_blend_ref``, ``mosaic_feather_ref``, ``mosaic_bands_ref``; imported, not changed)
applied to the culled images with the un-culled bounds -- ``expected`` does that.
"""
import numpy as np
import torch

import mosaic_bands_ref as mref
import mosaic_blend_ref as bref
import mosaic_feather_ref as fref
import mosaic_ref as ref

NAN_BITS = 0x7fc00000
EMPTY = np.uint32(0xffffffff)


def order_key(x):
    """csrc/order_key.h: the uint32 whose unsigned order is the order of the float32 values (-0.0 below +0.0)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def heights(view, J, axes):
    """Of the pixels of one image that take part, in ascending pixel index: ``(p, a_s, a_t, a_n)`` -- int64 and float32 arrays --,
    ``a_n = dot3(e3, wP)`` with the very ``wP`` the plane coordinates are formed from."""
    depth = view.depth.cpu().to(torch.float32).numpy()
    H, W = depth.shape
    Jn = J.cpu().numpy()
    v, u = np.nonzero(fref.members(depth, Jn))
    d = depth[v, u]
    Kinv = getattr(view, 'Kinv', None)
    Kinv = (view.K.cpu().to(torch.float32).inverse() if Kinv is None else Kinv.cpu().to(torch.float32).view(3, 3)).numpy()
    R, t = view.R.cpu().to(torch.float32).numpy(), view.t.cpu().to(torch.float32).numpy().reshape(3)
    A = torch.as_tensor(axes).cpu().to(torch.float32).view(3, 3).numpy()
    half = np.float32(0.5)
    x, y, w = d * (u.astype(np.float32) + half), d * (v.astype(np.float32) + half), d * np.float32(1.0)
    cP = [ref.dot3(Kinv[r], x, y, w) for r in range(3)]
    wP = [ref.dot3(R[r], cP[0], cP[1], cP[2]) + t[r] for r in range(3)]
    a_s, a_t, a_n = (ref.dot3(A[r], wP[0], wP[1], wP[2]) for r in range(3))
    assert all(q.dtype == np.float32 for q in (x, wP[0], a_s, a_t, a_n)) and bool(np.isfinite(a_n).all())
    p = (v * W + u).astype(np.int64)
    p0, _, s0, t0 = ref.pixels(view, J, axes)      # the best view's restatement sees the same pixels at the same place, to the bit
    assert np.array_equal(p, p0.numpy()) and a_s.tobytes() == s0.numpy().tobytes() and a_t.tobytes() == t0.numpy().tobytes()
    return p, a_s, a_t, a_n


def surface(views, Js, axes, gsd, T, bounds=None):
    """The surface test of the request: ``surface`` (Hm,Wm) float32 (NaN: empty), ``culled`` (Hm,Wm) int32, ``counts`` (culled
    samples, samples with a cell), ``share`` (their quotient), ``Js`` -- per image the culled (H,W,3) float32 image: the NaN
    0x7fc00000 at a pixel that does not take part or is culled, J bit for bit elsewhere --, ``mask`` -- per image the (H,W) bool of
    its culled pixels --, ``top`` (uint32 keys), ``bounds`` (those of ALL the pixels that take part, or the caller's), ``Hm``, ``Wm``."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if bounds is None:
        bounds = ref.bounds_of(views, Js, axes)
    lo_s, lo_t, hi_s, hi_t = (np.float32(x) for x in bounds)
    g, T = np.float32(gsd), np.float32(T)
    Wm, Hm = ref.cells(lo_s, hi_s, g), ref.cells(lo_t, hi_t, g)
    per = []
    top = np.full(Hm * Wm, EMPTY, np.uint32)
    for view, J in zip(views, Js):
        p, a_s, a_t, a_n = heights(view, J, axes)
        qs, qt = (a_s - lo_s) / g, (a_t - lo_t) / g                      # float32, IEEE
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)   # truncation
        np.minimum.at(top, cell, order_key(a_n[keep]))
        per.append((p, keep, cell, a_n[keep]))
    culled = np.zeros(Hm * Wm, np.int64)
    n_culled = n_cell = 0
    out_J, masks = [], []
    for (p, keep, cell, a_n), J in zip(per, Js):
        below = a_n - key_value(top[cell])                               # float32; a sample's own cell is never empty
        assert below.dtype == np.float32 and bool((below >= 0).all())
        gone = below > T
        np.add.at(culled, cell[gone], 1)
        n_culled, n_cell = n_culled + int(gone.sum()), n_cell + len(cell)
        bits = J.cpu().contiguous().numpy().view(np.uint32).reshape(-1, 3)
        stay = p[~keep].tolist() + p[keep][~gone].tolist()               # a member without a cell is not tested
        Jc = np.full(bits.shape, NAN_BITS, np.uint32)
        Jc[stay] = bits[stay]
        mask = np.zeros(bits.shape[0], bool)
        mask[p[keep][gone]] = True
        out_J.append(torch.from_numpy(Jc.view(np.float32).reshape(tuple(J.shape))))
        masks.append(mask.reshape(tuple(J.shape[:2])))
    height = np.where(top == EMPTY, np.uint32(NAN_BITS), key_value(top).view(np.uint32)).astype(np.uint32).view(np.float32)
    return {'surface': torch.from_numpy(height.reshape(Hm, Wm)), 'culled': torch.from_numpy(culled.astype(np.int32).reshape(Hm, Wm)),
            'counts': (n_culled, n_cell), 'share': n_culled / max(1, n_cell), 'Js': out_J, 'mask': masks, 'top': top,
            'bounds': tuple(float(x) for x in bounds), 'Hm': Hm, 'Wm': Wm}


def expected(views, Js, axes, gsd, T, H=None, F=None, K=None, bounds=None):
    """Every output of a mosaic with the surface test: ``surface``'s dictionary, the five best-view keys of ``mosaic_ref.mosaic`` of
    the culled images on the un-culled bounds (also whole as ``base``), with ``H`` the blend's four outputs and ``acc`` (feathered
    with ``F``; the border distances recomputed from the culled members), with ``K`` ``acc_bands`` and ``J_multiband``."""
    out = surface(views, Js, axes, gsd, T, bounds=bounds)
    cJ = out['Js']
    base = ref.mosaic(views, cJ, axes, gsd, bounds=out['bounds'])
    assert (base['Hm'], base['Wm']) == (out['Hm'], out['Wm'])
    out.update({k: base[k] for k in ('J', 'raw', 'source', 'pixel', 'range')}, base=base)
    if H is None:
        return out
    near = None if F is None else [fref.nearest2(fref.members(v.depth.cpu().numpy(), J.numpy())) for v, J in zip(views, cJ)]
    blend = bref.blend(views, cJ, axes, gsd, H, base=base) if F is None else fref.blend(views, cJ, axes, gsd, H, F, base=base, near=near)
    out.update({k: blend[k] for k in ('J_blend', 'raw_blend', 'weight', 'samples', 'acc')})
    if K is not None:
        bands = mref.multiband(views, cJ, axes, gsd, H, F, K, base=base, near=near)
        out.update(acc_bands=bands['acc_bands'], J_multiband=bands['J_multiband'])
    return out


# ---- the crafted pair of the two layers -----------------------------------------------------------------------------------------------
LAYERS_HW = (48, 64)
LAYERS_K = torch.tensor([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
LAYERS_GSD = 0.035          # twice the median pixel footprint (sucre.mosaic_default_gsd of the pair)
LAYERS_CELLS = (27, 37)     # Hm, Wm


def two_layers(seed=5):
    """View A looks from the origin at a surface 2.0 m away, view B from 1 m further along the axis at one 1.5 m away: B's surface
    lies 0.5 m LOWER (a_n = 2.5 against 2.0) and its ranges are smaller, so range alone lets the lower layer win wherever B has a
    sample.  ``(views, Js)`` as CPU tensors; ``R = I``, to be mosaicked with the identity as axes."""
    from types import SimpleNamespace
    H, W = LAYERS_HW
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for tz, d in ((0.0, 2.0), (1.0, 1.5)):
        rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=torch.full((H, W), d), rgb=rgb, K=LAYERS_K.clone(), R=torch.eye(3),
                                     t=torch.tensor([[0.0], [0.0], [tz]])))
        Js.append((torch.rand((H, W, 3), generator=g) * 0.9 + 0.05).contiguous())
    return views, Js
