"""CPU restatement of the mosaic's view-supported surface (csrc/support.h), helper of test_mosaic_support_host.py and
test_gpu_mosaic_support.py -- not a test.  It shares no code with the engine and is built on tests/mosaic_surface_ref.py and
tests/mosaic_ref.py by import: the samples -- cell, height, ordinal -- come from ``mosaic_surface_ref.heights`` and the float32
cell chain of ``mosaic_surface_ref.surface``; the levels of a cell come from ONE lexicographic sort of the per-image tops by
(cell, height key, ordinal), not from repeated minima as on the device; the cull is one float32 subtraction and two comparisons;
the counts are integer adds.  Every expected mosaic output is then one of the EXISTING restatements applied to the culled images
on the un-culled bounds, as ``mosaic_surface_ref.expected`` does it.
"""
import numpy as np
import torch

import mosaic_bands_ref as mref
import mosaic_blend_ref as bref
import mosaic_feather_ref as fref
import mosaic_ref as ref
import mosaic_surface_ref as sref

NO_RANK = np.uint64(0xffffffffffffffff)


def ranks(cell, a_n, ordinal, n_cells, M):
    """(M, n_cells) uint64: per cell the M smallest per-image tops as ``order_key << 32 | ordinal``, ascending, one per ordinal;
    all ones where a cell has fewer.  ``cell``, ``a_n`` (float32), ``ordinal``: one entry per sample; a NaN height adds nothing."""
    cell, ordinal = np.asarray(cell, np.int64), np.asarray(ordinal, np.int64)
    a_n = np.asarray(a_n, np.float32)
    ok = ~np.isnan(a_n)
    c, o, k = cell[ok], ordinal[ok], sref.order_key(a_n[ok]).astype(np.uint64)
    out = np.full((M, n_cells), NO_RANK, np.uint64)
    if len(c) == 0:
        return out
    by_image = np.lexsort((k, o, c))                                     # (cell, ordinal, key): an image's top of a cell comes first
    c, o, k = c[by_image], o[by_image], k[by_image]
    first = np.r_[True, (c[1:] != c[:-1]) | (o[1:] != o[:-1])]
    c, o, k = c[first], o[first], k[first]                               # one entry per (cell, image)
    by_height = np.lexsort((o, k, c))                                    # (cell, key, ordinal): a tie goes to the earlier image
    c, o, k = c[by_height], o[by_height], k[by_height]
    at = np.arange(len(c))
    start = np.r_[True, c[1:] != c[:-1]]
    level = at - np.maximum.accumulate(np.where(start, at, 0))
    take = level < M
    out[level[take], c[take]] = (k[take] << np.uint64(32)) | o[take].astype(np.uint64)
    return out


def supported_top(rank):
    """``(top, support, source)`` of every cell from its (M, n_cells) ranks: the uint32 key of the last level that holds something
    (all ones: none), the count of such levels (int32), the ordinal of that level (int32, -1: none)."""
    held = rank != NO_RANK
    n = held.sum(axis=0).astype(np.int32)
    assert bool((held[:-1] >= held[1:]).all())                           # nothing holds above an empty level
    last = rank[np.maximum(n - 1, 0), np.arange(rank.shape[1])]
    top = np.where(n > 0, (last >> np.uint64(32)).astype(np.uint32), sref.EMPTY).astype(np.uint32)
    source = np.where(n > 0, (last & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    return top, n, source


def cull_sides(cell, a_n, top, T):
    """``(below, above)`` bool per sample: ``d = a_n - key_value(top[cell])`` in float32, ``d > T`` and ``d < -T``; a cell whose top
    is all ones culls nothing, and neither does a NaN."""
    cell = np.asarray(cell, np.int64)
    k = top[cell]
    with np.errstate(invalid='ignore'):
        d = np.asarray(a_n, np.float32) - sref.key_value(k)
    assert d.dtype == np.float32
    T = np.float32(T)
    seen = k != sref.EMPTY
    with np.errstate(invalid='ignore'):
        return seen & (d > T), seen & (d < -T)


def heights_of(key):
    """(n,) float32 of uint32 keys, NaN where all ones."""
    return np.where(key == sref.EMPTY, np.uint32(sref.NAN_BITS), sref.key_value(key).view(np.uint32)).astype(np.uint32).view(np.float32)


def support(views, Js, axes, gsd, T, M, bounds=None):
    """The supported surface of the request: ``rank`` (M, Hm Wm) uint64, ``top`` (uint32 keys), ``surface`` (Hm,Wm) float32 (NaN:
    empty; the supported top), ``surface_top`` (the plain minimum, level 0), ``support`` and ``surface_source`` (Hm,Wm) int32,
    ``culled`` and ``culled_above`` (Hm,Wm) int32, ``counts`` (culled below, culled above, samples with a cell), ``Js`` -- per image
    the culled (H,W,3) float32 image --, ``mask_below`` / ``mask_above`` -- per image (H,W) bool --, ``cells`` -- per image (pixel
    indices, their cells) of its samples --, ``bounds`` (those of ALL the pixels that take part, or the caller's), ``Hm``, ``Wm``."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if bounds is None:
        bounds = ref.bounds_of(views, Js, axes)
    lo_s, lo_t, hi_s, hi_t = (np.float32(x) for x in bounds)
    g = np.float32(gsd)
    Wm, Hm = ref.cells(lo_s, hi_s, g), ref.cells(lo_t, hi_t, g)
    per = []
    for view, J in zip(views, Js):
        p, a_s, a_t, a_n = sref.heights(view, J, axes)
        qs, qt = (a_s - lo_s) / g, (a_t - lo_t) / g                      # float32, IEEE
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)   # truncation
        per.append((p, keep, cell, a_n[keep]))
    rank = ranks(np.concatenate([cell for _, _, cell, _ in per]), np.concatenate([a for *_, a in per]),
                 np.concatenate([np.full(len(cell), i, np.int64) for i, (_, _, cell, _) in enumerate(per)]), Hm * Wm, M)
    top, n, source = supported_top(rank)
    culled, culled_above = np.zeros(Hm * Wm, np.int64), np.zeros(Hm * Wm, np.int64)
    counts = [0, 0, 0]
    out_J, masks_below, masks_above = [], [], []
    for (p, keep, cell, a_n), J in zip(per, Js):
        below, above = cull_sides(cell, a_n, top, T)
        assert not bool((below & above).any())
        np.add.at(culled, cell[below], 1)
        np.add.at(culled_above, cell[above], 1)
        counts = [counts[0] + int(below.sum()), counts[1] + int(above.sum()), counts[2] + len(cell)]
        bits = J.cpu().contiguous().numpy().view(np.uint32).reshape(-1, 3)
        gone = below | above
        stay = p[~keep].tolist() + p[keep][~gone].tolist()               # a member without a cell is not tested
        Jc = np.full(bits.shape, sref.NAN_BITS, np.uint32)
        Jc[stay] = bits[stay]
        out_J.append(torch.from_numpy(Jc.view(np.float32).reshape(tuple(J.shape))))
        for side, masks in ((below, masks_below), (above, masks_above)):
            mask = np.zeros(bits.shape[0], bool)
            mask[p[keep][side]] = True
            masks.append(mask.reshape(tuple(J.shape[:2])))
    grid = lambda x, dtype: torch.from_numpy(np.ascontiguousarray(x).astype(dtype).reshape(Hm, Wm))
    return {'rank': rank, 'top': top, 'surface': grid(heights_of(top), np.float32),
            'surface_top': grid(heights_of(np.where(rank[0] == NO_RANK, sref.EMPTY, (rank[0] >> np.uint64(32)).astype(np.uint32)).astype(np.uint32)),
                                np.float32),
            'support': grid(n, np.int32), 'surface_source': grid(source, np.int32), 'culled': grid(culled, np.int32),
            'culled_above': grid(culled_above, np.int32), 'counts': tuple(counts), 'Js': out_J, 'mask_below': masks_below,
            'mask_above': masks_above, 'cells': [(p[keep], cell) for p, keep, cell, _ in per], 'bounds': tuple(float(x) for x in bounds), 'Hm': Hm, 'Wm': Wm}


def expected(views, Js, axes, gsd, T, M, H=None, F=None, K=None, bounds=None):
    """Every output of a mosaic with the supported surface: ``support``'s dictionary, the five best-view keys of
    ``mosaic_ref.mosaic`` of the culled images on the un-culled bounds, with ``H`` the blend's four outputs and ``acc`` (feathered
    with ``F``), with ``K`` ``acc_bands`` and ``J_multiband`` -- ``mosaic_surface_ref.expected`` with the other cull."""
    out = support(views, Js, axes, gsd, T, M, bounds=bounds)
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
