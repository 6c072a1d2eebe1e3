"""CPU restatement of the mosaic's per-image gain compensation (csrc/gains_mosaic.h), helper of test_mosaic_gains_host.py and
test_gpu_mosaic_gains.py -- not a test.  It shares no code with the engine and is built on tests/mosaic_ref.py and
tests/mosaic_blend_ref.py by import: the samples -- pixel, range, cell -- come from ``mosaic_ref.pixels`` and the float32 cell chain
of ``mosaic_ref.mosaic``; the reference pass's weights are ``mosaic_blend_ref.weights`` at the depth 2^126 (whose float32
reciprocal is the smallest normal number) and its colours ``mosaic_blend_ref.quantised``; the cell mean is the float64 quotient of
``mosaic_blend_ref.normalise``.  The span is one integer minimum and maximum per cell (``np.minimum.at``), the ten sums are int64
adds, the solve is float64 with ``math.fsum``.  ``Js``: the images as the gain kernels see them (the culled ones of a surface test).
"""
import math

import numpy as np
import torch

import mosaic_blend_ref as bref
import mosaic_ref as ref

WORDS = 10
NO_LO = np.uint32(0xffffffff)
MEAN_DEPTH = 2.0 ** 126      # 1 / float32(2^126) = 0x1p-126f, the reference pass's inv_h


def quantise(x):
    """``(int64)rint(min(max(x, -8), 8) 16384)`` of float32 values without NaN, one float32 operation per step."""
    x = np.asarray(x, np.float32)
    lo = np.maximum(x, np.float32(-8))
    c = np.minimum(lo, np.float32(8))
    q = c * np.float32(16384)
    assert q.dtype == np.float32
    return np.rint(q).astype(np.int64)


def samples_of(views, Js, axes, gsd, base):
    """Per image ``(p, cell, z)`` of its samples -- the pixels that take part and have a cell --, in ascending pixel index."""
    Hm, Wm = base['Hm'], base['Wm']
    lo_s, lo_t = np.float32(base['bounds'][0]), np.float32(base['bounds'][1])
    g = np.float32(gsd)
    out = []
    for view, J in zip(views, Js):
        p, z, a_s, a_t = ref.pixels(view, J, axes)
        qs, qt = (a_s.numpy() - lo_s) / g, (a_t.numpy() - lo_t) / g      # float32, IEEE
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)   # truncation
        out.append((p.numpy()[keep], cell, z.numpy()[keep]))
    return out


def span_of(samples, n_cells, first=0):
    """(n_cells, 2) uint32: per cell the smallest and the largest ordinal of its samples; (all ones, 0) for an empty cell."""
    lo, hi = np.full(n_cells, NO_LO, np.uint32), np.zeros(n_cells, np.uint32)
    for i, (_, cell, _) in enumerate(samples):
        np.minimum.at(lo, cell, np.uint32(first + i))
        np.maximum.at(hi, cell, np.uint32(first + i))
    return np.stack([lo, hi], axis=1)


def reference(views, Js, samples, G, zmin, n_cells):
    """``(acc (n_cells, 8) int64, mean (n_cells, 3) float32)`` of the reference pass at gains ``G``: the blend's sums over
    ``J x G`` with every weight 4096, and the blend's quotient (NaN in an empty cell)."""
    acc = np.zeros((n_cells, bref.ACC_WORDS), np.int64)
    for i, ((p, cell, z), view, J) in enumerate(zip(samples, views, Js)):
        wq = bref.weights(z, zmin[cell], MEAN_DEPTH)
        assert bool((wq == 4096).all())                                   # the plain per-sample mean
        Jg = J.cpu().numpy().reshape(-1, 3)[p] * np.asarray(G[i], np.float32)[None, :]
        assert Jg.dtype == np.float32
        Jq = bref.quantised(Jg)
        rgb = view.rgb.cpu().numpy().reshape(-1, 3)[p].astype(np.int64)
        for c in range(3):
            np.add.at(acc[:, c], cell, wq * Jq[:, c])
            np.add.at(acc[:, 3 + c], cell, wq * rgb[:, c])
        np.add.at(acc[:, 6], cell, wq)
        np.add.at(acc[:, 7], cell, 1)
    assert int(acc[:, 7].max(initial=0)) < 2 ** 20
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = ((acc[:, 0:3].astype(np.float64) / acc[:, 6].astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32)
    return acc, mean


def sums_of(Js, samples, G, span, mean):
    """(n, 10) int64: per image 1, Xq Mq x 3, Xq Xq x 3, Rq Rq x 3 over its samples in shared cells."""
    shared = span[:, 0] < span[:, 1]
    out = np.zeros((len(samples), WORDS), np.int64)
    for i, ((p, cell, _), J) in enumerate(zip(samples, Js)):
        use = shared[cell]
        Jp = J.cpu().numpy().reshape(-1, 3)[p[use]]
        X, M = quantise(Jp), quantise(mean[cell[use]])
        Y = quantise(Jp * np.asarray(G[i], np.float32)[None, :])
        assert int(np.abs(X).max(initial=0)) <= 1 << 17 and int(np.abs(Y - M).max(initial=0)) <= 1 << 18
        out[i, 0] = int(use.sum())
        out[i, 1:4] = (X * M).sum(axis=0)
        out[i, 4:7] = (X * X).sum(axis=0)
        out[i, 7:10] = ((Y - M) * (Y - M)).sum(axis=0)
    return out


def solve(sums, G, L):
    """The next gains, (n, 3) float32, from one pass's sums and its gains ``G``: per channel ``float(A) / float(B)`` where n > 0,
    A > 0 and B > 0, else the old gain; divided by the overlap-weighted mean (``math.fsum``); clamped to [1 / L, L]; an image
    without a sample in a shared cell stays at exactly 1."""
    n = [int(row[0]) for row in sums]
    out = np.ones((len(n), 3), np.float32)
    seen = [i for i in range(len(n)) if n[i] > 0]
    if not seen:
        return out
    total = math.fsum(float(n[i]) for i in seen)
    for c in range(3):
        g = []
        for i in seen:
            A, B = int(sums[i][1 + c]), int(sums[i][4 + c])
            g.append(float(A) / float(B) if A > 0 and B > 0 else float(np.float32(G[i][c])))
        s = math.fsum(float(n[i]) * gi for i, gi in zip(seen, g)) / total
        for i, gi in zip(seen, g):
            out[i, c] = np.float32(min(max(gi / s if s > 0 else gi, 1.0 / float(L)), float(L)))
    return out


def rms_of(sums):
    """``[sqrt(sum word(7 + c) / sum word 0) / 16384]`` of one pass, Python integers under a float64 root; zeros without a sample."""
    n = sum(int(row[0]) for row in sums)
    return [math.sqrt(sum(int(row[7 + c]) for row in sums) / n) / 16384.0 if n else 0.0 for c in range(3)]


def gains(views, Js, axes, gsd, R, L=2.0, bounds=None):
    """The gain compensation of the request: ``span`` (Hm Wm, 2) uint32, ``sums`` (R + 1, n, 10) int64, ``tables`` -- the R + 1 gain
    tables, the one entering each pass --, ``gains`` (n, 3) float32 (the last table), ``rms`` (R + 1, 3) float64, ``overlap`` (n,)
    int64, ``acc`` -- the last pass's reference accumulator --, ``base`` (``mosaic_ref.mosaic``'s result), ``Hm``, ``Wm``."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    base = ref.mosaic(views, Js, axes, gsd, bounds=bounds)
    n_cells = base['Hm'] * base['Wm']
    samples = samples_of(views, Js, axes, gsd, base)
    span = span_of(samples, n_cells)
    zmin = base['range'].numpy().reshape(-1)
    G = np.ones((len(views), 3), np.float32)
    tables, sums = [], []
    for r in range(R + 1):
        tables.append(G.copy())
        acc, mean = reference(views, Js, samples, G, zmin, n_cells)
        sums.append(sums_of(Js, samples, G, span, mean))
        if r < R:
            G = solve(sums[-1], G, L)
    sums = np.stack(sums)
    return {'span': span, 'sums': sums, 'tables': tables, 'gains': tables[-1], 'rms': np.array([rms_of(s) for s in sums], np.float64),
            'overlap': sums[-1][:, 0].copy(), 'acc': acc, 'base': base, 'Hm': base['Hm'], 'Wm': base['Wm'], 'samples': samples}


def loops(views, Js, axes, gsd, G, base):
    """``(span, sums)`` of ONE pass at gains ``G`` by plain Python loops over the samples, from the definition: the self-check of the
    vectorised functions above (small requests only)."""
    n_cells = base['Hm'] * base['Wm']
    samples = samples_of(views, Js, axes, gsd, base)
    lo, hi = [0xffffffff] * n_cells, [0] * n_cells
    tot, cnt = [[0, 0, 0] for _ in range(n_cells)], [0] * n_cells
    flat = [J.cpu().numpy().reshape(-1, 3) for J in Js]
    for i, (p, cell, _) in enumerate(samples):
        for pp, c in zip(p.tolist(), cell.tolist()):
            lo[c], hi[c] = min(lo[c], i), max(hi[c], i)
            cnt[c] += 1
            for ch in range(3):
                jg = np.float32(flat[i][pp, ch]) * np.float32(G[i][ch])
                tot[c][ch] += 4096 * int(np.rint(np.minimum(np.maximum(jg, np.float32(-1024)), np.float32(1024)) * np.float32(1048576)))
    sums = [[0] * WORDS for _ in samples]
    for i, (p, cell, _) in enumerate(samples):
        for pp, c in zip(p.tolist(), cell.tolist()):
            if not lo[c] < hi[c]:
                continue
            sums[i][0] += 1
            for ch in range(3):
                m = np.float32((float(tot[c][ch]) / float(4096 * cnt[c])) * 2.0 ** -20)
                x = np.float32(flat[i][pp, ch])
                X, M, Y = int(quantise(x)), int(quantise(m)), int(quantise(x * np.float32(G[i][ch])))
                sums[i][1 + ch] += X * M
                sums[i][4 + ch] += X * X
                sums[i][7 + ch] += (Y - M) ** 2
    return np.array(list(zip(lo, hi)), np.uint32).reshape(n_cells, 2), np.array(sums, np.int64)
