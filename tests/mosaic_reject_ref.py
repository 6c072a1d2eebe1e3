"""CPU restatement of the mosaic's colour consensus across views (csrc/reject.h), helper of test_mosaic_reject_host.py and
test_gpu_mosaic_reject.py -- not a test.  It shares no code with the engine: the samples and their cells come from
``mosaic_surface_ref.heights`` and the float32 cell chain of ``mosaic_surface_ref.surface``; a cell's eight ordinals come from ONE
sort of the distinct (cell, ordinal) pairs, not from a chain of minima; the sums are ``np.add.at`` on Python-exact int64; the median
image of a cell comes from a sort with exact rational keys (``fractions.Fraction``), not from cross-multiplied comparisons; the
reference colour is one float64 division, one exact scaling and one rounding; the cull is one float32 subtraction and one comparison.
"""
from fractions import Fraction

import numpy as np
import torch

import mosaic_gains_ref as gref
import mosaic_ref as ref
import mosaic_surface_ref as sref

SLOTS = 8
MIN_VIEWS = 3
FREE = np.uint32(0xffffffff)
MAX_SAMPLES = 1 << 20


def slots_of(cell, ordinal, n_cells):
    """``(slot_ord (n_cells, 8) uint32, slot_over (n_cells,) uint32)``: per cell the 8 smallest distinct ordinals of its samples,
    ascending, all ones behind them; 1 where a ninth exists."""
    cell, ordinal = np.asarray(cell, np.int64), np.asarray(ordinal, np.int64)
    slot_ord = np.full((n_cells, SLOTS), FREE, np.uint32)
    slot_over = np.zeros(n_cells, np.uint32)
    if len(cell) == 0:
        return slot_ord, slot_over
    pairs = np.unique(np.stack([cell, ordinal], axis=1), axis=0)            # distinct, sorted by (cell, ordinal)
    c, o = pairs[:, 0], pairs[:, 1]
    at = np.arange(len(c))
    start = np.r_[True, c[1:] != c[:-1]]
    place = at - np.maximum.accumulate(np.where(start, at, 0))
    take = place < SLOTS
    slot_ord[c[take], place[take]] = o[take].astype(np.uint32)
    slot_over[np.unique(c[~take])] = 1
    return slot_ord, slot_over


def sums_of(cell, ordinal, xq, slot_ord):
    """``slot_sum`` (n_cells, 8, 4) int64: per slot the count and the three sums of the quantised colours ``xq`` (n, 3) int64 of
    the samples of the slot's ordinal; a sample whose ordinal holds no slot of its cell adds nothing."""
    cell, ordinal = np.asarray(cell, np.int64), np.asarray(ordinal, np.int64)
    slot_sum = np.zeros(slot_ord.shape + (4,), np.int64)
    if len(cell) == 0:
        return slot_sum
    hit = slot_ord[cell].astype(np.int64) == ordinal[:, None]               # (n, 8): at most one per row
    assert int(hit.sum(axis=1).max()) <= 1
    votes = hit.any(axis=1)
    slot = hit.argmax(axis=1)
    np.add.at(slot_sum[:, :, 0], (cell[votes], slot[votes]), 1)
    for c in range(3):
        np.add.at(slot_sum[:, :, 1 + c], (cell[votes], slot[votes]), xq[votes, c])
    return slot_sum


def consensus_of(slot_ord, slot_sum):
    """``(ref (n_cells, 3) float32, source (n_cells,) int32, views (n_cells,) int32)``: the cell's median image by mean brightness
    (exact rationals; ties by ordinal; the lower median) and its mean colour; NaN and -1 where fewer than three images hold slots."""
    n_cells = slot_ord.shape[0]
    out = np.full((n_cells, 3), sref.NAN_BITS, np.uint32).view(np.float32)
    source = np.full(n_cells, -1, np.int32)
    views = (slot_ord != FREE).sum(axis=1).astype(np.int32)
    assert bool(((slot_ord[:, :-1] < slot_ord[:, 1:]) | (slot_ord[:, 1:] == FREE)).all())      # ascending, free words last
    for cell in np.nonzero(views >= MIN_VIEWS)[0]:
        k = int(views[cell])
        rows = [[int(x) for x in slot_sum[cell, a]] for a in range(k)]
        assert all(0 < row[0] < MAX_SAMPLES for row in rows)
        order = sorted(range(k), key=lambda a: (Fraction(rows[a][1] + rows[a][2] + rows[a][3], rows[a][0]), int(slot_ord[cell, a])))
        a = order[(k - 1) // 2]
        source[cell] = int(slot_ord[cell, a])
        n = np.float64(rows[a][0])
        for c in range(3):
            out[cell, c] = np.float32((np.float64(rows[a][1 + c]) / n) * np.float64(2.0 ** -14))
    return out, source, views


def samples_of(views, Js, axes, gsd, bounds=None):
    """``(per, Hm, Wm, bounds)``: per image ``(p, keep, cell)`` -- the pixel indices of its members, which of them have a cell,
    and those cells --, with the float32 cell chain of the other restatements, on the bounds of all members (or the caller's)."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    if bounds is None:
        bounds = ref.bounds_of(views, Js, axes)
    lo_s, lo_t, hi_s, hi_t = (np.float32(x) for x in bounds)
    g = np.float32(gsd)
    Wm, Hm = ref.cells(lo_s, hi_s, g), ref.cells(lo_t, hi_t, g)
    per = []
    for view, J in zip(views, Js):
        p, a_s, a_t, _ = sref.heights(view, J, axes)
        qs, qt = (a_s - lo_s) / g, (a_t - lo_t) / g                      # float32, IEEE
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)   # truncation
        per.append((p, keep, cell))
    return per, Hm, Wm, tuple(float(x) for x in bounds)


def reject(views, Js, axes, gsd, T, bounds=None, first_ordinal=0):
    """The colour consensus of the request (``Js``: the images as the claim sees them -- surface-culled when there is a surface
    test): ``slot_ord`` (cells, 8) uint32, ``slot_sum`` (cells, 8, 4) int64, ``slot_over`` (cells,) uint32, ``reject_ref`` (Hm,Wm,3)
    float32, ``reject_source``, ``reject_views``, ``rejected`` (Hm,Wm) int32, ``reject_overflow`` (Hm,Wm) bool, ``per_image`` (n,2)
    int64 -- samples in cells with a reference, samples rejected --, ``Js`` -- per image the NaN copy --, ``mask`` -- per image
    the (H,W) bool of its rejected pixels --, ``cells`` -- per image (pixel indices, cells) of its samples --, ``bounds``, ``Hm``,
    ``Wm``."""
    per, Hm, Wm, bounds = samples_of(views, Js, axes, gsd, bounds)
    n_cells = Hm * Wm
    cell = np.concatenate([c for _, _, c in per]) if per else np.zeros(0, np.int64)
    ordinal = np.concatenate([np.full(len(c), first_ordinal + i, np.int64) for i, (_, _, c) in enumerate(per)])
    colours = [J.cpu().contiguous().numpy().reshape(-1, 3)[p[keep]] for (p, keep, _), J in zip(per, Js)]
    xq = np.concatenate([gref.quantise(x) for x in colours]) if per else np.zeros((0, 3), np.int64)
    slot_ord, slot_over = slots_of(cell, ordinal, n_cells)
    slot_sum = sums_of(cell, ordinal, xq, slot_ord)
    cref, source, n_views = consensus_of(slot_ord, slot_sum)
    T = np.float32(T)
    rejected = np.zeros(n_cells, np.int64)
    per_image = np.zeros((len(per), 2), np.int64)
    out_J, masks = [], []
    for i, ((p, keep, c), J, x) in enumerate(zip(per, Js, colours)):
        tested = source[c] >= 0
        with np.errstate(invalid='ignore'):
            d = np.abs(x - cref[c])                                      # float32: one subtraction; a NaN reference compares false
            assert d.dtype == np.float32
            gone = tested & (source[c] != first_ordinal + i) & (d > T).any(axis=1)
        np.add.at(rejected, c[gone], 1)
        per_image[i] = (int(tested.sum()), int(gone.sum()))
        bits = J.cpu().contiguous().numpy().view(np.uint32).reshape(-1, 3)
        stay = p[~keep].tolist() + p[keep][~gone].tolist()               # a member without a cell is not tested
        Jc = np.full(bits.shape, sref.NAN_BITS, np.uint32)
        Jc[stay] = bits[stay]
        mask = np.zeros(bits.shape[0], bool)
        mask[p[keep][gone]] = True
        out_J.append(torch.from_numpy(Jc.view(np.float32).reshape(tuple(J.shape))))
        masks.append(mask.reshape(tuple(J.shape[:2])))
    grid = lambda x, dtype, *tail: torch.from_numpy(np.ascontiguousarray(x).astype(dtype).reshape(Hm, Wm, *tail))
    return {'slot_ord': slot_ord, 'slot_sum': slot_sum, 'slot_over': slot_over,
            'reject_ref': torch.from_numpy(np.ascontiguousarray(cref).reshape(Hm, Wm, 3)), 'reject_source': grid(source, np.int32),
            'reject_views': grid(n_views, np.int32), 'rejected': grid(rejected, np.int32), 'reject_overflow': grid(slot_over != 0, bool),
            'per_image': per_image, 'Js': out_J, 'mask': masks, 'cells': [(p[keep], c) for p, keep, c in per], 'bounds': bounds,
            'Hm': Hm, 'Wm': Wm}


def chain_steps(words, v, start=0):
    """The claim's chain of csrc/reject.h for one lane as a generator of atomic steps: every ``next()`` performs ONE atomicMin on
    ``words`` (a list of 8 ints, 0xffffffff: free) and the generator returns True when a value was carried past the last slot."""
    s = start
    while s < SLOTS:
        old = words[s]
        words[s] = min(old, v)                                           # the atomic step
        yield
        if old == v:
            return False
        if old > v:
            if old == int(FREE):
                return False
            v = old
        s += 1
    return True
