"""GPU test of the one cull kernel behind ``sucre_mosaic_cull`` and ``sucre_mosaic_cull_supported`` (csrc/surface.hip:
``mosaic_cull_kernel<kCount, kTwoSided>``), at the shapes where a merge of the two can go wrong: a partial last block, an exact
256-pixel block and a one-row image in ONE call, so that the image boundaries fall inside one workgroup's 32-block window of the
counting form; ordinals that do not start at 0; a top written by hand, so that samples lie below, above and within the tolerance,
some have no cell and one cell was never seen by the surface phase.

The yardstick is the restatements' own pieces (tests/mosaic_surface_ref.py: the samples' heights, the order keys, the NaN;
tests/mosaic_support_ref.py: ``cull_sides``), not the engine.  Every comparison is exact, bit for bit, the NaN's payload included.
"""
import numpy as np
import pytest
import torch

import mosaic_ref as ref
import mosaic_support_ref as pref
import mosaic_surface_ref as sref
from test_gpu_mosaic_support import device_view
from test_gpu_mosaic_surface import host_view, same_bits
from sucre_amd import engine

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [(17, 19), (16, 16), (1, 300)]      # H x W: 323 pixels (a partial second block), 256 (one exact block), one row of 300
T = 0.05
GSD = 0.02
FIRST = 5                                   # the ordinal of the call's first image


@pytest.fixture(scope='module')
def case():
    """The three images, the caller's bounds -- cut short along s, so that the far end of the long row has no cell --, per image
    its samples ``(pixel, has a cell, cell, height)`` from the restatement, and the two tops: the crafted one and the plain minimum."""
    g = torch.Generator().manual_seed(4100)
    views, Js = [], []
    for i, (H, W) in enumerate(SIZES):
        depth = 2.0 + (torch.rand((H, W), generator=g) - 0.5) * 0.3      # the height IS the depth here: 1.85 .. 2.15 around a top of 2.0
        J = torch.rand((H, W, 3), generator=g) * 3 - 1
        depth.view(-1)[::11] = 0.0                                       # pixels that do not take part: no depth ...
        J.view(-1, 3)[5::13, i] = float('nan')                           # ... or a NaN in one channel
        J.view(-1, 3)[3::17] = torch.tensor([float('inf'), -0.0, -2000.0])
        views.append(device_view(depth, f'{H}x{W}', tx=0.004 * i, ty=0.003 * i))
        Js.append(J.to(DEV))
    axes = torch.eye(3)
    hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
    lo_s, lo_t, hi_s, hi_t = (np.float32(x) for x in ref.bounds_of(hv, hJ, axes))
    bounds = (lo_s, lo_t, np.float32(lo_s + np.float32(0.6) * (hi_s - lo_s)), hi_t)
    g32 = np.float32(GSD)
    Wm, Hm = ref.cells(bounds[0], bounds[2], g32), ref.cells(bounds[1], bounds[3], g32)
    samples = []
    for v, J in zip(hv, hJ):
        p, a_s, a_t, a_n = sref.heights(v, J, axes)
        qs, qt = (a_s - bounds[0]) / g32, (a_t - bounds[1]) / g32         # float32, IEEE: mosaic_surface_ref.surface's chain
        assert qs.dtype == np.float32
        keep = (qs >= 0) & (qs < Wm) & (qt >= 0) & (qt < Hm)
        cell = qt[keep].astype(np.int64) * Wm + qs[keep].astype(np.int64)
        samples.append((p, keep, cell, a_n[keep]))
    reached = np.unique(np.concatenate([cell for _, _, cell, _ in samples]))
    crafted = np.full(Hm * Wm, sref.order_key(np.float32(2.0)), np.uint32)
    crafted[1::5] = sref.order_key(np.float32(2.12))                     # most samples of these cells stand above the top
    crafted[2::5] = sref.order_key(np.float32(1.88))                     # ... and of these lie below it
    crafted[reached[::4]] = sref.EMPTY                                   # cells the surface phase never saw
    plain = np.full(Hm * Wm, sref.EMPTY, np.uint32)
    for _, _, cell, a_n in samples:
        np.minimum.at(plain, cell, sref.order_key(a_n))
    return dict(views=views, Js=Js, hJ=hJ, bounds=tuple(float(x) for x in bounds), Hm=Hm, Wm=Wm, samples=samples, crafted=crafted, plain=plain)


def expected(case, top, two_sided):
    """The copies, the per-cell counts and the counters of one cull against ``top``, from ``mosaic_support_ref.cull_sides``; the
    one-sided cull has no second side."""
    n_cells = case['Hm'] * case['Wm']
    culled, culled_above = np.zeros(n_cells, np.int64), np.zeros(n_cells, np.int64)
    n_below = n_above = n_cell = 0
    copies = []
    for (p, keep, cell, a_n), J in zip(case['samples'], case['hJ']):
        below, above = pref.cull_sides(cell, a_n, top, T)
        if not two_sided:
            above = np.zeros_like(above)
        assert not bool((below & above).any())
        np.add.at(culled, cell[below], 1)
        np.add.at(culled_above, cell[above], 1)
        n_below, n_above, n_cell = n_below + int(below.sum()), n_above + int(above.sum()), n_cell + len(cell)
        bits = J.contiguous().numpy().view(np.uint32).reshape(-1, 3)
        stay = p[~keep].tolist() + p[keep][~(below | above)].tolist()    # a member without a cell is not tested
        Jc = np.full(bits.shape, sref.NAN_BITS, np.uint32)
        Jc[stay] = bits[stay]
        copies.append(torch.from_numpy(Jc.view(np.float32).reshape(tuple(J.shape))))
    grid = lambda x: torch.from_numpy(x.astype(np.int32).reshape(case['Hm'], case['Wm']))      # noqa: E731
    return dict(Js=copies, culled=grid(culled), culled_above=grid(culled_above), below=n_below, above=n_above, cell=n_cell)


def cull(case, top, support, count):
    """A begun mosaic whose ``top`` is ``top``, and its one cull of the three images: ``(mosaic, copies)``."""
    m = engine.Mosaic(torch.eye(3), GSD, DEV)
    m.begin(bounds=case['bounds'], surface=T, **({} if support is None else {'support': support}))
    assert (m.Hm, m.Wm) == (case['Hm'], case['Wm'])
    m.top.copy_(torch.from_numpy(top.view(np.int32)))
    return m, m.culled_images(case['views'], case['Js'], FIRST, count=count)


def test_the_crafted_top_has_every_kind_of_sample(case):
    want = expected(case, case['crafted'], True)
    total = sum(len(p) for p, *_ in case['samples'])
    print(f'{case["Wm"]} x {case["Hm"]} cells; {total} members, {want["cell"]} with a cell; below {want["below"]}, above {want["above"]}')
    assert 0 < want['below'] and 0 < want['above'] and want['below'] + want['above'] < want['cell'] < total      # below, above, within, no cell
    unseen = np.concatenate([cell for _, _, cell, _ in case['samples']])
    assert int((case['crafted'][unseen] == sref.EMPTY).sum()) > 0        # samples in cells the surface phase never saw
    assert sum(-(-H * W // 256) for H, W in SIZES) == 5 < 32              # one workgroup of the counting form walks all three images
    assert [H * W % 256 for H, W in SIZES] == [67, 0, 44]
    nothing_above = expected(case, case['plain'], True)
    assert nothing_above['above'] == 0 and nothing_above['below'] > 0


@pytest.mark.parametrize('count', [False, True])
@pytest.mark.parametrize('support', [None, 1, 2])
def test_one_kernel_serves_both_culls_in_both_forms(case, support, count):
    want = expected(case, case['crafted'], support is not None)
    m, copies = cull(case, case['crafted'], support, count)
    for i, (J, w) in enumerate(zip(copies, want['Js'])):
        assert J.dtype == torch.float32 and same_bits(J, w), (support, count, SIZES[i])
    gone = torch.cat([J.reshape(-1) for J in copies]).cpu().numpy().view(np.uint32)
    assert set(gone[np.isnan(gone.view(np.float32))].tolist()) == {sref.NAN_BITS}      # the one NaN: the images' own NaN do not pass
    out = m.result()
    zero = torch.zeros((m.Hm, m.Wm), dtype=torch.int32)
    assert same_bits(out['culled'], want['culled'] if count else zero)
    if support is None:
        assert 'culled_above' not in out and m.support_counts is None
        assert [int(x) for x in m.surface_counts.cpu()] == ([want['below'], want['cell']] if count else [0, 0])
    else:
        assert same_bits(out['culled_above'], want['culled_above'] if count else zero)
        assert [int(x) for x in m.support_counts.cpu()] == ([want['below'], want['above'], want['cell']] if count else [0, 0, 0])
        assert [int(x) for x in m.surface_counts.cpu()] == ([want['below'], want['cell']] if count else [0, 0])


def test_a_support_of_one_is_the_one_sided_cull_where_nothing_lies_above(case):
    want = expected(case, case['plain'], False)
    one, copies_one = cull(case, case['plain'], None, True)
    two, copies_two = cull(case, case['plain'], 1, True)
    for a, b, w in zip(copies_one, copies_two, want['Js']):
        assert same_bits(a, w) and same_bits(b, w)
    assert same_bits(one.result()['culled'], want['culled']) and same_bits(two.result()['culled'], want['culled'])
    assert not bool(two.result()['culled_above'].any())
    counts = [int(x) for x in two.support_counts.cpu()]
    assert counts == [want['below'], 0, want['cell']]
    assert [int(x) for x in one.surface_counts.cpu()] == [counts[0], counts[2]] == [int(x) for x in two.surface_counts.cpu()]
