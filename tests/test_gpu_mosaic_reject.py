"""GPU tests of the mosaic's colour consensus across views (sucre_mosaic_reject_claim / _sums / _consensus / _cull, engine.Mosaic,
sucre.mosaic, --mosaic-reject).

The yardstick is tests/mosaic_reject_ref.py, a numpy restatement that shares no code with the engine and sorts where the device
chains atomic minima; test_mosaic_reject_host.py checks it against plain loops over the definition.  Every comparison is EXACT, bit
for bit, NaN included: the slots are integer minima, the sums integer sums, the median an integer comparison, the reference one
float64 division and one rounding, the test one float32 subtraction.
"""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import mosaic_ref as ref
import mosaic_reject_crafted as crafted
import mosaic_reject_ref as rref
import mosaic_surface_ref as sref
from test_gpu_mosaic_support import scene_case
from test_gpu_mosaic_surface import host_view, same_bits
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BEST = ('J', 'raw', 'source', 'pixel', 'range')
GRID_KEYS = ('rejected', 'reject_ref', 'reject_source', 'reject_views', 'reject_overflow')
NEW = GRID_KEYS + ('reject_per_image', 'reject_tol')
T_SOME = 0.3           # random colours in [0.01, 0.99]: some samples differ from the median image's mean by more, some by less
_CACHE = {}


def oracle(key, T):
    ck = ('oracle', key, T)
    if ck not in _CACHE:
        _, _, axes, gsd, hv, hJ = scene_case(key)
        _CACHE[ck] = rref.reject(hv, hJ, axes, gsd, T)
    return _CACHE[ck]


def by_hand(views, Js, axes, gsd, T, claim=None, sums=None, plain=False, bounds=None):
    """begin, the claim and then the sums over the parts ``[(a, b), ...]`` in the order given, the slots as they stand then,
    finish_reject, one counted cull of everything."""
    m = engine.Mosaic(axes, gsd, DEV)
    if bounds is None:
        m.add_bounds(views, Js)
    m.begin(bounds, reject=T)
    whole = [(0, len(views))]
    for a, b in claim or whole:
        m.add_reject_claim(views[a:b], Js[a:b], a, plain_atomic=plain)
    for a, b in sums or whole:
        m.add_reject_sums(views[a:b], Js[a:b], a, plain=plain)
    slots = (m.reject_slot_ord.clone(), m.reject_slot_sum.clone(), m.reject_slot_over.clone())
    m.finish_reject()
    assert m.reject_slot_ord is None and m.reject_slot_sum is None and m.reject_slot_over is None      # 292 bytes per cell freed
    copies = [J.clone() for J in m.rejected_images(views, Js, 0, count=True)]
    return m, slots, copies


def check_slots(slots, want, what):
    ord_, sum_, over = slots
    assert ord_.dtype == torch.int32 and same_bits(ord_, torch.from_numpy(want['slot_ord'].view(np.int32))), (what, 'slot_ord')
    assert sum_.dtype == torch.int64 and same_bits(sum_, torch.from_numpy(want['slot_sum'])), (what, 'slot_sum')
    assert same_bits(over, torch.from_numpy(want['slot_over'].view(np.int32))), (what, 'slot_over')


def check_result(m, want, what):
    got = m.result()
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']), what
    for k in GRID_KEYS:
        assert same_bits(got[k], want[k]), (what, k, int((got[k].cpu() != want[k]).sum()))
    assert same_bits(got['reject_per_image'], torch.from_numpy(want['per_image'])), (what, got['reject_per_image'].tolist(), want['per_image'].tolist())
    assert got['reject_tol'] == float(np.float32(m.reject)) and type(got['reject_tol']) is float


def check_by_hand(m, slots, copies, want, what):
    check_slots(slots, want, what)
    check_result(m, want, what)
    for i, (J, w) in enumerate(zip(copies, want['Js'])):
        assert J.dtype == torch.float32 and same_bits(J, w), (what, i)


# ---- 1. every tensor equals the restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_every_tensor_equals_the_restatement(key):
    views, Js, axes, gsd, hv, hJ = scene_case(key)
    want = oracle(key, T_SOME)
    tested, gone = want['per_image'].sum(axis=0).tolist()
    n_views = want['reject_views'].numpy().reshape(-1)
    print(f'{key}: {want["Wm"]} x {want["Hm"]} cells, views histogram {np.bincount(n_views, minlength=9).tolist()}, {gone} of {tested} tested '
          f'samples rejected, {int((want["reject_source"] >= 0).sum())} cells with a consensus')
    assert 0 < gone < tested and int((n_views >= 3).sum()) > 0 and int(((n_views > 0) & (n_views < 3)).sum()) > 0      # of the restatement
    m, slots, copies = by_hand(views, Js, axes, gsd, T_SOME)
    check_by_hand(m, slots, copies, want, key)
    # the whole run: the same consensus, and every later phase sees the rejected copies on the bounds of all members
    run = engine.mosaic_of(views, Js, axes, gsd, reject=T_SOME)
    check_result(run, want, (key, 'run'))
    base = ref.mosaic(hv, want['Js'], axes, gsd, bounds=want['bounds'])
    for k in BEST:
        assert same_bits(run.result()[k], base[k]), (key, k)
    assert run.reject_slot_ord is None and run._held == {}      # nothing of the run is held after it


def test_the_consensus_sees_the_surface_culled_images():
    views, Js, axes, gsd, hv, hJ = scene_case('deep')
    T_surface = 0.005
    culled = sref.surface(hv, hJ, axes, gsd, T_surface)
    assert culled['counts'][0] > 0
    want = rref.reject(hv, culled['Js'], axes, gsd, T_SOME, bounds=culled['bounds'])
    for kw in (dict(), dict(batch=2)):
        run = engine.mosaic_of(views, Js, axes, gsd, surface=T_surface, reject=T_SOME, **kw)
        check_result(run, want, kw)
        assert tuple(int(x) for x in run.surface_counts.cpu()) == culled['counts']       # each counted once
        base = ref.mosaic(hv, want['Js'], axes, gsd, bounds=culled['bounds'])
        for k in BEST:
            assert same_bits(run.result()[k], base[k]), (kw, k)


def plane_views(sizes, seed, poses=None, colours=None):
    """Views of one plane 2.0 m below cameras with the crafted survey's intrinsics; ``(views, Js, host views, host Js)``."""
    g = torch.Generator().manual_seed(seed)
    views, Js = [], []
    for i, (H, W) in enumerate(sizes):
        tx, ty = (0.01 * (i % 3) - 0.01, 0.007 * (i % 2)) if poses is None else poses[i]
        J = torch.rand((H, W, 3), generator=g) * 0.6 + 0.2 if colours is None else torch.tensor(colours[i]).repeat(H, W, 1)
        rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        views.append(engine.DeviceView(depth=torch.full((H, W), 2.0, device=DEV), rgb=rgb.to(DEV), K=crafted.K, R=torch.eye(3),
                                       t=torch.tensor([[tx], [ty], [0.0]]), name=f'v{i}'))
        Js.append(J.contiguous().to(DEV))
    return views, Js, [host_view(v) for v in views], [J.cpu() for J in Js]


def test_an_image_that_is_no_multiple_of_the_block():
    """One 37 x 53 image (1961 pixels: 7 blocks and 169 pixels) between 48 x 64 ones: its block of the copy starts where the padded
    blocks before it end, and the counts of every image stand in its own row."""
    views, Js, hv, hJ = plane_views([(48, 64), (37, 53), (48, 64), (48, 64)], 31)
    Js[1][5:9, 7:20] = float('nan')
    hJ[1] = Js[1].cpu()
    want = rref.reject(hv, hJ, torch.eye(3), crafted.GSD, 0.25)
    assert all(0 < want['per_image'][i, 1] < want['per_image'][i, 0] for i in range(4))
    m, slots, copies = by_hand(views, Js, torch.eye(3), crafted.GSD, 0.25)
    check_by_hand(m, slots, copies, want, '37x53')
    alone = m.rejected_images([views[1]], [Js[1]], 1)[0]      # its block starts the buffer; not counted again
    assert same_bits(alone, want['Js'][1])
    check_result(m, want, 'after one more cull')


# ---- 2. any order, any split, either form -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_batches_orders_and_the_plain_form_give_the_same_bits(key):
    views, Js, axes, gsd, *_ = scene_case(key)
    want = oracle(key, T_SOME)
    n = len(views)
    ones, twos = [(i, i + 1) for i in range(n)], [(i, min(i + 2, n)) for i in range(0, n, 2)]
    for kw in (dict(claim=ones, sums=ones), dict(claim=twos, sums=twos), dict(claim=ones[::-1], sums=twos[::-1]),
               dict(claim=twos[::-1], sums=ones[::-1], plain=True), dict(plain=True), dict(claim=twos[::-1])):
        m, slots, copies = by_hand(views, Js, axes, gsd, T_SOME, **kw)
        check_by_hand(m, slots, copies, want, (key, kw))
    first = engine.mosaic_of(views, Js, axes, gsd, reject=T_SOME, blend=0.5).result()
    for kw in (dict(batch=1), dict(batch=2), dict(batch=32, plain_atomic=True), dict(batch=4, plain_atomic=True)):
        got = engine.mosaic_of(views, Js, axes, gsd, reject=T_SOME, blend=0.5, **kw).result()
        assert list(got) == list(first)
        for k, v in first.items():
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, (kw, k)


# ---- 3. more images than slots ------------------------------------------------------------------------------------------------------------

PLANE_C, FISH_C = crafted.PLANE_COLOUR, crafted.FISH_COLOUR


def overlapping(n, fish=()):
    """``n`` views of 24 x 32 from ONE place, all of the plane colour; ``fish``: (ordinal, rows, columns) patches of the fish colour."""
    views, Js, hv, hJ = plane_views([(24, 32)] * n, 5, poses=[(0.0, 0.0)] * n, colours=[PLANE_C] * n)
    for i, rows, cols in fish:
        Js[i][rows, cols] = torch.tensor(FISH_C, device=DEV)
        hJ[i] = Js[i].cpu()
    return views, Js, hv, hJ


def test_ten_views_keep_the_eight_earliest_and_test_all_ten():
    early, late = (0, slice(2, 8), slice(3, 12)), (9, slice(14, 20), slice(18, 30))
    views, Js, hv, hJ = overlapping(10, [early, late])
    want = rref.reject(hv, hJ, torch.eye(3), crafted.GSD, crafted.TOL)
    reached = want['reject_views'].numpy().reshape(-1) > 0
    assert bool((want['slot_ord'][reached] == np.arange(8, dtype=np.uint32)).all()) and bool((want['slot_over'][reached] == 1).all())
    assert want['per_image'][:, 1].tolist() == [6 * 9] + [0] * 8 + [6 * 12]      # both fish, and nothing else
    source = want['reject_source'].numpy().reshape(-1)
    assert set(source[reached].tolist()) == {3, 4}      # plane means tie: ordinal 3 of 0..7; where ordinal 0 is the brightest, 4
    for plain in (False, True):
        m, slots, copies = by_hand(views, Js, torch.eye(3), crafted.GSD, crafted.TOL, claim=[(7, 10), (0, 3), (3, 7)], plain=plain)
        check_by_hand(m, slots, copies, want, ('ten', plain))
        assert bool(m.result()['reject_overflow'].view(-1)[torch.from_numpy(reached).to(DEV)].all())
        assert bool(torch.isnan(copies[9][late[1], late[2]]).all()) and bool(torch.isnan(copies[0][early[1], early[2]]).all())
    run = engine.mosaic_of(views, Js, torch.eye(3), crafted.GSD, reject=crafted.TOL, blend=0.5).result()
    filled = run['source'] >= 0
    assert bool((run['J'][filled] == torch.tensor(PLANE_C, device=DEV)).all()) and bool((run['J_blend'][filled] == run['J_blend'][filled][0]).all())


def test_eight_views_fill_the_slots_without_the_flag_and_a_view_listed_twice_counts_twice():
    views, Js, hv, hJ = overlapping(8, [(2, slice(4, 9), slice(5, 15))])
    want = rref.reject(hv, hJ, torch.eye(3), crafted.GSD, crafted.TOL)
    assert not want['slot_over'].any() and int(want['reject_views'].max()) == 8 and want['per_image'][:, 1].tolist() == [0, 0, 50, 0, 0, 0, 0, 0]
    m, slots, copies = by_hand(views, Js, torch.eye(3), crafted.GSD, crafted.TOL)
    check_by_hand(m, slots, copies, want, 'eight')
    assert not bool(m.result()['reject_overflow'].any())
    # [a, b]: two images, no consensus; [a, b, b]: three ordinals, b is the median twice over and a's fish goes
    views, Js, hv, hJ = overlapping(2, [(0, slice(4, 9), slice(5, 15))])
    for twice, gone in ((False, 0), (True, 50)):
        v, J, h, hj = (views + views[1:], Js + Js[1:], hv + hv[1:], hJ + hJ[1:]) if twice else (views, Js, hv, hJ)
        want = rref.reject(h, hj, torch.eye(3), crafted.GSD, crafted.TOL)
        assert int(want['reject_views'].max()) == len(v) and int(want['rejected'].sum()) == gone
        m, slots, copies = by_hand(v, J, torch.eye(3), crafted.GSD, crafted.TOL)
        check_by_hand(m, slots, copies, want, ('twice', twice))


# ---- 4. two images cannot say which of them is wrong --------------------------------------------------------------------------------------

def test_a_cell_that_two_images_reach_rejects_nothing():
    views, Js, hv, hJ = plane_views([(48, 64), (40, 50)], 77)
    Js[0][3:7, 3:9, 1] = float('nan')
    Js[1][10, 10] = torch.tensor([float('inf'), -50.0, 1e30], device=DEV)
    hJ = [J.cpu() for J in Js]
    want = rref.reject(hv, hJ, torch.eye(3), crafted.GSD, 1e-6)
    assert int(want['reject_views'].max()) == 2 and not bool(want['rejected'].any())
    m, slots, copies = by_hand(views, Js, torch.eye(3), crafted.GSD, 1e-6)
    check_by_hand(m, slots, copies, want, 'two')
    for J, copy in zip(Js, copies):      # the copy IS J at the members, NaN elsewhere
        member = ~torch.isnan(J).any(dim=-1)
        assert same_bits(copy[member], J[member]) and bool(torch.isnan(copy[~member]).all())
    got = m.result()
    assert bool((got['reject_source'] == -1).all()) and bool(torch.isnan(got['reject_ref']).all()) and not bool(got['reject_per_image'].any())


# ---- 5. a tolerance that rejects nothing; the filled set at every tolerance ---------------------------------------------------------------

@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_a_tolerance_that_rejects_nothing_leaves_every_other_key_alone(key):
    views, Js, axes, gsd, *_ = scene_case(key)
    half = np.float32(gsd * np.float32(0.5))      # half the default gsd: holes for the fill
    for extra in (dict(gains=2), dict(gains=2, gain_solve='direct')):
        kw = dict(blend=0.5, feather=8, bands=2, fill=3 * float(half), surface=0.05, support=2, **extra)
        was = engine.mosaic_of(views, Js, axes, half, **kw).result()
        got = engine.mosaic_of(views, Js, axes, half, reject=1e6, **kw).result()
        assert [k for k in got if k not in NEW] == list(was) and [k for k in got if k in NEW] == list(NEW)
        for k, v in was.items():
            assert (same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v), (extra, k)
        assert not bool(got['rejected'].any()) and not bool(got['reject_per_image'][:, 1].any()) and bool(got['reject_per_image'][:, 0].any())
        assert int((got['fill_level'] > 0).sum()) > 0 and bool((got['reject_source'] >= 0).any())
    plain = engine.mosaic_of(views, Js, axes, gsd).result()
    for T in (1e-6, 0.05, T_SOME):
        m = engine.mosaic_of(views, Js, axes, gsd, reject=T)
        got = m.result()
        assert torch.equal(got['source'] >= 0, plain['source'] >= 0) and (m.Hm, m.Wm, m.lo) == tuple(plain['source'].shape) + (m.lo,), T
        assert bool((got['rejected'] > 0).any())


# ---- 6. the fish --------------------------------------------------------------------------------------------------------------------------

def test_a_fish_with_the_seabed_s_depth_no_longer_owns_its_cells():
    hv, hJ = crafted.survey()
    views = [engine.DeviceView(depth=v.depth.to(DEV), rgb=v.rgb.to(DEV), K=v.K, R=v.R, t=v.t, name='ABC'[i]) for i, v in enumerate(hv)]
    Js = [J.to(DEV) for J in hJ]
    axes, T, fish = torch.eye(3), crafted.TOL, crafted.FISH_VIEW
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * 3)
    assert float(gsd) == float(np.float32(crafted.GSD))
    want = rref.reject(hv, hJ, axes, gsd, T)
    px, cell = want['cells'][fish]      # the patch, from the restatement alone
    is_fish = crafted.fish_mask().reshape(-1)[px]
    reached = sorted(set(cell[is_fish].tolist()))
    patch = torch.zeros(want['Hm'] * want['Wm'], dtype=torch.bool)
    patch[reached] = True
    patch = patch.view(want['Hm'], want['Wm']).to(DEV)
    colour, plane = torch.tensor(crafted.FISH_COLOUR, device=DEV), torch.tensor(crafted.PLANE_COLOUR, device=DEV)

    owned = None
    for kw in (dict(), dict(surface=0.1, support=2)):      # without the flag, and equally with the height tests: they see nothing
        was = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, **kw).result()
        assert 'culled' not in was or (int(was['culled'].sum()) == 0 and int(was['culled_above'].sum()) == 0)
        by_fish = (was['J'] == colour).all(dim=-1)
        assert int(by_fish.sum()) > 0 and bool((was['source'][by_fish] == fish).all()) and not bool(by_fish[~patch].any())
        assert bool((was['J_blend'][patch] != plane).any(dim=-1).all())      # the fish shifts the blend in every cell it reaches
        assert owned is None or owned == int(by_fish.sum())
        owned = int(by_fish.sum())

    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, reject=T)
    got = m.result()
    check_result(m, want, 'fish')
    assert got['reject_per_image'][:, 1].tolist() == [0, crafted.N_FISH, 0] and int(got['rejected'].sum()) == crafted.N_FISH == 384
    assert torch.equal(got['rejected'] > 0, patch)
    assert not bool((got['reject_source'][patch] == fish).any())      # the source never names the fish's view inside the patch
    assert not bool((got['J'] == colour).all(dim=-1).any())
    assert bool((got['J'][patch] == plane).all())
    outside = (got['source'] >= 0) & ~patch
    blended = was['J_blend'][outside][0]      # the plane's colour as the blend's fixed point holds it: one value in every cell the fish spares
    assert bool((was['J_blend'][outside] == blended).all()) and bool(((blended - plane).abs() < 1e-3).all())
    assert bool((got['J_blend'][patch] == blended).all())
    for k in BEST + ('J_blend', 'raw_blend', 'weight', 'samples'):      # outside the patch every cell keeps its bits
        assert same_bits(got[k][~patch], was[k][~patch]), k
    assert torch.equal(got['source'] >= 0, was['source'] >= 0)
    print(f'fish: the patch reaches {len(reached)} of {int((got["source"] >= 0).sum())} filled cells; without the flag (and with surface 0.1, '
          f'support 2) the fish owns {owned} best-view cells and shifts the blend in all {len(reached)}; with reject {T} its {crafted.N_FISH} '
          f'samples are rejected in {int((got["rejected"] > 0).sum())} cells and none is left')


# ---- 7. the order of the phases, the arguments, the bound ----------------------------------------------------------------------------------

def test_the_phases_refuse_the_wrong_order():
    views, Js, axes, gsd, *_ = scene_case('scene')
    m = engine.Mosaic(axes, gsd, DEV)
    m.add_bounds(views, Js)
    m.begin()
    for call in (lambda: m.add_reject_claim(views, Js, 0), lambda: m.add_reject_sums(views, Js, 0), m.finish_reject,
                 lambda: m.rejected_images(views, Js, 0)):
        with pytest.raises(ValueError, match='begin\\(\\) was not given a reject tolerance'):
            call()
    m.begin(reject=0.1)
    with pytest.raises(ValueError, match='add_reject_claim\\(\\) over every image comes first'):
        m.add_reject_sums(views, Js, 0)                      # no claim yet
    m.add_reject_claim(views[:3], Js[:3], 0)
    with pytest.raises(ValueError, match=f'ordinals 3..{len(views) - 1}, but the claim has seen 3 images'):
        m.add_reject_sums(views[3:], Js[3:], 3)              # the claim has not finished
    with pytest.raises(ValueError, match='add_reject_sums\\(\\) over every image come first'):
        m.finish_reject()
    with pytest.raises(ValueError, match='finish_reject\\(\\) comes first'):
        m.rejected_images(views, Js, 0)
    with pytest.raises(ValueError, match='finish_reject\\(\\) comes first'):
        m.splat(views, Js, 0)                                # the splat sees the rejected copies: there are none yet
    m.add_reject_claim(views[3:], Js[3:], 3)
    m.add_reject_sums(views, Js, 0)
    with pytest.raises(ValueError, match='add_reject_sums\\(\\) has read the slots already'):
        m.add_reject_claim(views, Js, 0)
    m.finish_reject()
    for call, text in ((m.finish_reject, 'formed already'), (lambda: m.add_reject_sums(views, Js, 0), 'formed the consensus already')):
        with pytest.raises(ValueError, match=text):
            call()
    check_result(m, {**oracle('scene', 0.1), 'per_image': np.zeros((len(views), 2), np.int64), 'rejected': torch.zeros((m.Hm, m.Wm), dtype=torch.int32)},
                 'nothing counted yet')


def test_the_entries_check_their_arguments_before_any_launch():
    views, Js, axes, gsd, *_ = scene_case('scene')
    m = engine.Mosaic(axes, gsd, DEV)
    m.add_bounds(views, Js)
    m.begin(reject=0.1)
    images = m._images(views[:2], Js[:2])
    odd = m.reject_slot_ord.view(-1)[1:]
    for entry, rest, text in (
            ('sucre_mosaic_reject_claim', (m.reject_slot_ord, m.reject_slot_over, 2), 'unknown mosaic flags'),
            ('sucre_mosaic_reject_claim', (odd, m.reject_slot_over, 0), 'slot_ord_dev is NULL or not 32-byte aligned'),
            ('sucre_mosaic_reject_claim', (m.reject_slot_ord, None, 0), 'slot_over_dev is NULL'),
            ('sucre_mosaic_reject_sums', (None, m.reject_slot_sum, 0), 'slot_ord_dev is NULL'),
            ('sucre_mosaic_reject_sums', (m.reject_slot_ord, None, 0), 'slot_sum_dev is NULL'),
            ('sucre_mosaic_reject_sums', (m.reject_slot_ord, m.reject_slot_sum, 4), 'unknown mosaic flags')):
        with pytest.raises(_lib.SucreError, match=text):
            m._walk(entry, images, 0, _lib.C.byref(m.grid), *rest)
    o = m._out
    buf = torch.empty(2 * 96 * 64 * 3 + 1024, dtype=torch.float32, device=DEV)
    counts = torch.zeros((2, 16), dtype=torch.int64, device=DEV)
    cull = lambda *rest: m._walk('sucre_mosaic_reject_cull', images, *rest)
    g = _lib.C.byref(m.grid)
    f = _lib.C.c_float
    for rest, text in (((0, g, o['reject_ref'], o['reject_source'], f(0.0), buf, None, 2, None), 'tol=0 must be finite and > 0'),
                       ((0, g, o['reject_ref'], o['reject_source'], f(float('nan')), buf, None, 2, None), 'must be finite and > 0'),
                       ((0, g, None, o['reject_source'], f(0.1), buf, None, 2, None), 'ref_dev is NULL'),
                       ((0, g, o['reject_ref'], None, f(0.1), buf, None, 2, None), 'source_dev is NULL'),
                       ((0, g, o['reject_ref'], o['reject_source'], f(0.1), None, None, 2, None), 'J_out is NULL'),
                       ((0, g, o['reject_ref'], o['reject_source'], f(0.1), Js[1], None, 2, None), 'J_out overlaps'),
                       ((1, g, o['reject_ref'], o['reject_source'], f(0.1), buf, None, 2, counts), 'outside the 2 rows'),
                       ((0, g, o['reject_ref'], o['reject_source'], f(0.1), buf, None, 2, counts.view(-1)[1:]), 'counts_dev is not 128-byte aligned')):
        with pytest.raises(_lib.SucreError, match=text):
            cull(*rest)
    assert bool((m.reject_slot_ord == -1).all()) and not bool(m.reject_slot_sum.any())      # nothing was launched


def test_a_million_samples_of_one_image_in_one_cell_stop_the_run():
    """Three images of 1024 x 1024 from one place on a grid of one cell: each holds 2^20 samples there, the bound of the integer
    comparison of two means; one row fewer passes."""
    def three(H):
        depth = torch.full((H, 1024), 2.0, device=DEV)
        rgb = torch.zeros((H, 1024, 3), dtype=torch.uint8, device=DEV)
        views = [engine.DeviceView(depth=depth, rgb=rgb, K=crafted.K, R=torch.eye(3), t=torch.zeros(3, 1), name=f'big{i}') for i in range(3)]
        return views, [torch.full((H, 1024, 3), 0.25 * (i + 1), device=DEV) for i in range(3)]
    views, Js = three(1024)
    with pytest.raises(ValueError, match=r'mosaic reject: 3 times an image holds 1048576 samples or more in one cell.*--mosaic-gsd') as e:
        engine.mosaic_of(views, Js, torch.eye(3), 1000.0, reject=0.1)
    assert e.value.field == 'reject'
    views, Js = three(1023)
    got = engine.mosaic_of(views, Js, torch.eye(3), 1000.0, reject=0.1).result()
    assert tuple(got['source'].shape) == (1, 1) and got['reject_source'].tolist() == [[1]] and got['reject_views'].tolist() == [[3]]
    assert got['reject_ref'].tolist() == [[[0.5, 0.5, 0.5]]] and got['reject_per_image'].tolist() == [[1023 * 1024, 1023 * 1024], [1023 * 1024, 0], [1023 * 1024, 1023 * 1024]]
    assert got['rejected'].tolist() == [[2 * 1023 * 1024]] and got['source'].tolist() == [[1]]


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------------
CLI_T = 0.02

LINE = re.compile(r"^mosaic reject of (\S+): (\d+) of (\d+) filled cells have a consensus of 3 or more images \((\d+) hold more than 8: the 8 "
                  r"earliest vote\); (\d+) of (\d+) samples \((\S+) %\) differ from it by more than (\S+), in (\d+) cells; most rejected (\S+) "
                  r"\((\d+) samples\)$")


@pytest.fixture(scope='module')
def reject_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_reject_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    rest = ['--mosaic-blend', '0.5', '--mosaic-feather', '8', '--mosaic-fill', '0.05', '--mosaic-bands', '2', '--mosaic-surface', '0.05',
            '--mosaic-support', '2', '--mosaic-gains', '2', '--mosaic-gain-solve', 'direct']
    runs = {'all': rest, 'all_nothing': rest + ['--mosaic-reject', '1e6'], 'some': ['--mosaic-blend', '0.5', '--mosaic-reject', str(CLI_T)]}
    printed = {}
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        for name, extra in runs.items():
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                sucre.main(base + ['--output-dir', str(root / name), '--mosaic', str(restored)] + extra)
            printed[name] = text.getvalue()
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, scene, restored, printed, base


def test_cli_writes_the_new_file_and_leaves_every_other_file_alone(reject_run):
    from PIL import Image as PILImage
    root, scene, restored, printed, _ = reject_run
    before = sorted(p.name for p in (root / 'all').iterdir())
    assert sorted(p.name for p in (root / 'all_nothing').iterdir()) == sorted(before + ['mosaic_rejected.png'])
    for name in before:
        if name != 'mosaic.pt':
            assert (root / 'all' / name).read_bytes() == (root / 'all_nothing' / name).read_bytes(), name
    was, got = torch.load(root / 'all' / 'mosaic.pt'), torch.load(root / 'all_nothing' / 'mosaic.pt')
    assert set(got) - set(was) == set(NEW) and not set(was) - set(got)
    for k, v in was.items():
        assert (same_bits(v, got[k]) if torch.is_tensor(v) else v == got[k]), k
    assert got['reject_tol'] == 1e6 and not bool(got['rejected'].any())
    assert np.array_equal(np.asarray(PILImage.open(root / 'all_nothing' / 'mosaic_rejected.png')), sucre.mosaic_culled_picture(got['rejected'].numpy()))
    # the lines: those of the run without the flag, with one more after the support's
    lines_was, lines = printed['all'].splitlines(), printed['all_nothing'].splitlines()
    at = next(i for i, line in enumerate(lines_was) if line.startswith('mosaic support of ')) + 1
    assert lines[:at] == lines_was[:at] and lines[at + 1:] == lines_was[at:] and len(lines) == len(lines_was) + 1
    hit = LINE.match(lines[at])
    assert hit, lines[at]
    assert hit.group(1, 4, 5, 7, 8, 9, 11) == ('1e+06', '0', '0', '0.0', '1e+06', '0', '0') and int(hit.group(2)) > 0
    assert 'mosaic reject' not in printed['all']


def test_cli_rejects_what_the_engine_rejects(reject_run):
    from PIL import Image as PILImage
    from sucre_amd import sfm
    root, scene, restored, printed, _ = reject_run
    names = [v.name for v in scene.views]
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, reject=CLI_T, batch=4)
    got = torch.load(root / 'some' / 'mosaic.pt')
    for k, v in m.result().items():
        assert (same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v), k
    want = rref.reject([host_view(v) for v in views], [J.cpu() for J in Js], axes, gsd, CLI_T)
    check_result(m, want, 'cli')
    per = got['reject_per_image']
    tested, gone = int(per[:, 0].sum()), int(per[:, 1].sum())
    assert 0 < gone < tested
    hit = LINE.match(next(line for line in printed['some'].splitlines() if line.startswith('mosaic reject')))
    filled = got['source'] >= 0
    worst = int(per[:, 1].argmax())
    assert hit and hit.groups() == (f'{CLI_T:.6g}', str(int(((got['reject_source'] >= 0) & filled).sum())), str(int(filled.sum())),
                                    str(int(got['reject_overflow'].sum())), str(gone), str(tested), f'{100.0 * gone / tested:.1f}', f'{CLI_T:.6g}',
                                    str(int((got['rejected'] > 0).sum())), names[worst], str(int(per[worst, 1])))
    assert int(got['rejected'].sum()) == gone
    assert np.array_equal(np.asarray(PILImage.open(root / 'some' / 'mosaic_rejected.png')), sucre.mosaic_culled_picture(got['rejected'].numpy()))
