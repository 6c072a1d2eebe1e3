"""CPU restatement of the direct solve of the mosaic's gain compensation (csrc/gains_direct.h), helper of
test_mosaic_gain_direct_host.py and test_gpu_mosaic_gain_direct.py -- not a test.  It shares no code with the engine and is built on
tests/mosaic_ref.py and tests/mosaic_gains_ref.py by import: the samples, the span, the quantiser, the reference pass and the rounds'
solve are theirs.  New here: the per (cell, image) sums (``np.add.at`` into a dense (n, cells, 4) array -- small requests only), the
overflow rule (a shared cell that more than ``SLOTS`` different ordinals reach), the pair words (float64: one multiply, one divide,
``np.rint``), the diag, and the solve (``numpy.linalg.solve`` of the full system, built entry by entry from Python integers).
"""
import math

import numpy as np
import torch

import mosaic_gains_ref as gref
import mosaic_ref as ref

SLOTS = 8
FREE = np.uint32(0xffffffff)
PRIOR = 2.0 ** -20


def cell_sums(Js, samples, span, n_cells):
    """(n, n_cells, 4) int64: per image and cell the count and ``sum Xq`` x 3 of the image's samples there; shared cells only."""
    shared = span[:, 0] < span[:, 1]
    S = np.zeros((len(samples), n_cells, 4), np.int64)
    for i, ((p, cell, _), J) in enumerate(zip(samples, Js)):
        use = shared[cell]
        X = gref.quantise(J.cpu().numpy().reshape(-1, 3)[p[use]])
        np.add.at(S[i, :, 0], cell[use], 1)
        for c in range(3):
            np.add.at(S[i, :, 1 + c], cell[use], X[:, c])
    return S


def overflow_of(S):
    """(n_cells,) bool: more than ``SLOTS`` different images have a sample in the (shared) cell."""
    return (S[:, :, 0] > 0).sum(axis=0) > SLOTS


def slots_of(S, over, first=0):
    """``(slot_ord (cells, 8) uint32, slot_sum (cells, 8, 4) int64)`` with every cell's slots in ascending ordinal; the slots of an
    overflowed cell are left free and zero here: what the device holds there depends on arrival, and nothing may read it."""
    n, n_cells, _ = S.shape
    slot_ord = np.full((n_cells, SLOTS), FREE, np.uint32)
    slot_sum = np.zeros((n_cells, SLOTS, 4), np.int64)
    present = S[:, :, 0] > 0
    for cell in np.nonzero(present.any(axis=0) & ~over)[0]:
        ords = np.nonzero(present[:, cell])[0]
        slot_ord[cell, :len(ords)] = ords + first
        slot_sum[cell, :len(ords)] = S[ords, cell]
    return slot_ord, slot_sum


def pairs_of(S, over):
    """(n, n, 4) int64, the upper triangle: per pair i <= j, over the cells both reach that did not overflow,
    ``sum rint((float64(S_i) float64(S_j)) / float64(N))`` x 3 and the number of such cells."""
    n = S.shape[0]
    present = S[:, :, 0] > 0
    N = S[:, :, 0].sum(axis=0).astype(np.float64)
    out = np.zeros((n, n, 4), np.int64)
    for i in range(n):
        for j in range(i, n):
            both = present[i] & present[j] & ~over
            if not both.any():
                continue
            for c in range(3):
                prod = S[i, both, 1 + c].astype(np.float64) * S[j, both, 1 + c].astype(np.float64)
                out[i, j, c] = int(np.rint(prod / N[both]).astype(np.int64).sum())
            out[i, j, 3] = int(both.sum())
    return out


def diag_of(Js, samples, span, over):
    """(n, 4) int64: per image the count and ``sum Xq Xq`` x 3 of its samples in shared cells that did not overflow."""
    ok = (span[:, 0] < span[:, 1]) & ~over
    out = np.zeros((len(samples), 4), np.int64)
    for i, ((p, cell, _), J) in enumerate(zip(samples, Js)):
        use = ok[cell]
        X = gref.quantise(J.cpu().numpy().reshape(-1, 3)[p[use]])
        out[i, 0] = int(use.sum())
        out[i, 1:4] = (X * X).sum(axis=0)
    return out


def solve(pairs, diag, G, L, prior=PRIOR):
    """``(gains (n, 3) float32, kept)``: per channel, over the images with n > 0 and Q > 0, ``(A + mu diag Q) g = mu Q`` with
    ``A = diag Q - P``; every other image keeps its gain; a channel without a finite positive solution keeps all of them (``kept``);
    then the n-weighted ``fsum`` mean over the images with n > 0 becomes 1, the clamp to [1 / L, L], float32."""
    n = len(diag)
    out = np.array(G, np.float32).reshape(n, 3).copy()
    seen = [i for i in range(n) if int(diag[i][0]) > 0]
    kept = []
    for c in range(3):
        act = [i for i in seen if int(diag[i][1 + c]) > 0]
        g = {i: float(out[i, c]) for i in seen}
        if act:
            A = np.zeros((len(act), len(act)), np.float64)
            for a, i in enumerate(act):
                for b, j in enumerate(act):
                    A[a, b] = -float(int(pairs[min(i, j)][max(i, j)][c]))
            Q = np.array([float(int(diag[i][1 + c])) for i in act], np.float64)
            A += np.diag(Q)
            try:
                x = np.linalg.solve(A + prior * np.diag(Q), prior * Q)
            except np.linalg.LinAlgError:
                x = np.full(len(act), np.nan)
            if not (np.isfinite(x).all() and (x > 0).all()):
                kept.append(c)
                continue
            for i, v in zip(act, x):
                g[i] = float(v)
        if seen:
            s = math.fsum(float(int(diag[i][0])) * g[i] for i in seen) / math.fsum(float(int(diag[i][0])) for i in seen)
            for i in seen:
                out[i, c] = np.float32(min(max(g[i] / s if s > 0 else g[i], 1.0 / float(L)), float(L)))
    return out, kept


def residual(pairs, diag, g, c, prior=PRIOR):
    """``max |((A + mu diag Q) g - mu Q)_i| / Q_i`` of channel ``c`` over the images with n > 0 and Q > 0, in float64, from the
    integers: how well ``g`` (before gauge and clamp) solves the normal equations."""
    act = [i for i in range(len(diag)) if int(diag[i][0]) > 0 and int(diag[i][1 + c]) > 0]
    worst = 0.0
    for i in act:
        Q = float(int(diag[i][1 + c]))
        r = Q * (1.0 + prior) * float(g[i]) - prior * Q
        r -= math.fsum(float(int(pairs[min(i, j)][max(i, j)][c])) * float(g[j]) for j in act)
        worst = max(worst, abs(r) / Q)
    return worst


def components(pairs, diag):
    """Connected groups among the images with n > 0, joined where a pair shares a cell."""
    seen = [i for i in range(len(diag)) if int(diag[i][0]) > 0]
    group = {i: i for i in seen}
    for _ in seen:
        for i in seen:
            for j in seen:
                if i < j and int(pairs[i][j][3]) > 0:
                    group[i] = group[j] = min(group[i], group[j])
    return len(set(group.values()))


def state(views, Js, axes, gsd, bounds=None):
    """The integer state of the direct solve for the request: ``span``, ``S`` (``cell_sums``), ``over``, ``slot_ord``, ``slot_sum``,
    ``pairs``, ``diag``, ``excluded`` (the overflowed cells), ``samples``, ``base``, ``Hm``, ``Wm``."""
    axes = torch.as_tensor(axes, dtype=torch.float32).view(3, 3)
    base = ref.mosaic(views, Js, axes, gsd, bounds=bounds)
    n_cells = base['Hm'] * base['Wm']
    samples = gref.samples_of(views, Js, axes, gsd, base)
    span = gref.span_of(samples, n_cells)
    S = cell_sums(Js, samples, span, n_cells)
    over = overflow_of(S)
    slot_ord, slot_sum = slots_of(S, over)
    return {'span': span, 'S': S, 'over': over, 'slot_ord': slot_ord, 'slot_sum': slot_sum, 'pairs': pairs_of(S, over),
            'diag': diag_of(Js, samples, span, over), 'excluded': int(over.sum()), 'samples': samples, 'base': base,
            'Hm': base['Hm'], 'Wm': base['Wm']}


def gains(views, Js, axes, gsd, R, L=2.0, bounds=None):
    """The gain compensation of the request with the direct solve in place of the first round's: ``state``'s keys, and, as
    ``mosaic_gains_ref.gains``, ``sums`` (R + 1, n, 10), ``tables``, ``gains``, ``rms``, ``overlap``; ``direct``: the table the direct
    solve produced, ``kept``: its channels that kept their gains."""
    st = state(views, Js, axes, gsd, bounds)
    n_cells = st['Hm'] * st['Wm']
    zmin = st['base']['range'].numpy().reshape(-1)
    G = np.ones((len(views), 3), np.float32)
    tables, sums = [], []
    for r in range(R + 1):
        tables.append(G.copy())
        _, mean = gref.reference(views, Js, st['samples'], G, zmin, n_cells)
        sums.append(gref.sums_of(Js, st['samples'], G, st['span'], mean))
        if r == 0:
            G, kept = solve(st['pairs'], st['diag'], G, L)
            direct = G.copy()
        elif r < R:
            G = gref.solve(sums[-1], G, L)
    sums = np.stack(sums)
    return {**st, 'sums': sums, 'tables': tables, 'gains': tables[-1], 'direct': direct, 'kept': kept,
            'rms': np.array([gref.rms_of(s) for s in sums], np.float64), 'overlap': sums[-1][:, 0].copy()}


def loops(views, Js, axes, gsd, base):
    """``(per_cell, over, pairs, diag)`` by plain Python loops over the samples, from the definition -- the self-check of the
    vectorised functions above (small requests only).  ``per_cell``: cell -> {ordinal: [n, sum Xq x 3]} for the shared cells."""
    n_cells = base['Hm'] * base['Wm']
    samples = gref.samples_of(views, Js, axes, gsd, base)
    reach = [set() for _ in range(n_cells)]
    for i, (_, cell, _) in enumerate(samples):
        for c in cell.tolist():
            reach[c].add(i)
    flat = [J.cpu().numpy().reshape(-1, 3) for J in Js]
    per_cell = {}
    for i, (p, cell, _) in enumerate(samples):
        for pp, c in zip(p.tolist(), cell.tolist()):
            if len(reach[c]) < 2:
                continue
            row = per_cell.setdefault(c, {}).setdefault(i, [0, 0, 0, 0])
            row[0] += 1
            for ch in range(3):
                row[1 + ch] += int(gref.quantise(np.float32(flat[i][pp, ch])))
    over = {c for c, held in per_cell.items() if len(held) > SLOTS}
    n = len(samples)
    pairs = [[[0, 0, 0, 0] for _ in range(n)] for _ in range(n)]
    for c, held in per_cell.items():
        if c in over:
            continue
        N = sum(row[0] for row in held.values())
        for i in held:
            for j in held:
                if i <= j:
                    for ch in range(3):
                        pairs[i][j][ch] += int(np.rint((float(held[i][1 + ch]) * float(held[j][1 + ch])) / float(N)))
                    pairs[i][j][3] += 1
    diag = [[0, 0, 0, 0] for _ in range(n)]
    for i, (p, cell, _) in enumerate(samples):
        for pp, c in zip(p.tolist(), cell.tolist()):
            if c in per_cell and c not in over:
                diag[i][0] += 1
                for ch in range(3):
                    diag[i][1 + ch] += int(gref.quantise(np.float32(flat[i][pp, ch]))) ** 2
    return per_cell, over, np.array(pairs, np.int64), np.array(diag, np.int64)
