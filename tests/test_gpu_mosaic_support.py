"""GPU tests of the mosaic's view-supported surface (sucre_mosaic_support / _support_top / _cull_supported, engine.Mosaic,
sucre.mosaic, --mosaic-support).

The yardstick is tests/mosaic_support_ref.py, a numpy restatement that shares no code with the engine and forms the levels by one
lexicographic sort; test_mosaic_support_host.py checks it against plain loops over the definition.  Every comparison is EXACT, bit
for bit, NaN included: a height is a fixed chain of IEEE operations, a level an integer minimum, the counts integer sums.
"""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import mosaic_support_crafted as crafted
import mosaic_support_ref as pref
import mosaic_surface_ref as sref
from test_gpu_mosaic_surface import MASKS, WIDE_K, host_view, masked_image, restored_like, same_bits
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
BEST = ('J', 'raw', 'source', 'pixel', 'range')
BLENDED = ('J_blend', 'raw_blend', 'weight', 'samples')
NEW = ('support', 'surface_source', 'culled_above', 'surface_top', 'surface_support')
BLEND_H = 0.5
TOLS = (0.005, 0.05, 1e6)       # the surface tests' three
_CACHE = {}


def scene_case(key):
    """(views, Js, axes, gsd, host views, host Js) of ``make_scene(96, 64, 6)`` ('scene') or ``make_deep_scene(96, 64, 6)``
    ('deep'), in the request's order or (``key`` ending in ' reversed') reversed -- made once, never changed."""
    if key not in _CACHE:
        if key.endswith(' reversed'):
            views, Js, axes, gsd, hv, hJ = scene_case(key[:-len(' reversed')])
            _CACHE[key] = (views[::-1], Js[::-1], axes, gsd, hv[::-1], hJ[::-1])
        else:
            scene = synth.make_scene(96, 64, 6) if key == 'scene' else synth.make_deep_scene(96, 64, 6)
            views = engine.device_views_from_scene(scene, DEV)
            Js = [restored_like(v, 700 + k) for k, v in enumerate(views)]
            axes = sucre.mosaic_axes(views)
            gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
            _CACHE[key] = (views, Js, axes, gsd, [host_view(v) for v in views], [J.cpu() for J in Js])
    return _CACHE[key]


def oracle(key, T, M, whole=False):
    """``pref.support`` of the case, or (``whole``) ``pref.expected`` with the blend -- computed once."""
    ck = (key, T, M, whole)
    if ck not in _CACHE:
        views, Js, axes, gsd, hv, hJ = scene_case(key)
        _CACHE[ck] = pref.expected(hv, hJ, axes, gsd, T, M, H=BLEND_H) if whole else pref.support(hv, hJ, axes, gsd, T, M)
    return _CACHE[ck]


def samples_of(hv, hJ, axes, gsd):
    """(cell, a_n, ordinal) of every sample of the request, from the restatement."""
    whole = pref.support(hv, hJ, axes, gsd, 1.0, 1)
    heights = [sref.heights(v, J, axes)[3] for v, J in zip(hv, hJ)]
    cell = np.concatenate([c for _, c in whole['cells']])
    assert all(len(h) == len(c) for h, (_, c) in zip(heights, whole['cells']))      # every member has a cell on its own bounds
    return cell, np.concatenate(heights), np.concatenate([np.full(len(c), i, np.int64) for i, (_, c) in enumerate(whole['cells'])])


def unflagged(key, **kw):
    ck = (key, 'unflagged', tuple(sorted(kw.items())))
    if ck not in _CACHE:
        views, Js, axes, gsd, _, _ = scene_case(key)
        _CACHE[ck] = engine.mosaic_of(views, Js, axes, gsd, **kw)
    return _CACHE[ck]


def check_ranks(m, want, what):
    """The rank words, the top and the per-cell outputs of the support phase, the cull's counts and per-cell counts."""
    got = m.result()
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']), what
    assert same_bits(m.rank, torch.from_numpy(want['rank'].view(np.int64))), (what, 'rank')
    assert same_bits(m.top, torch.from_numpy(want['top'].view(np.int32))), (what, 'top')
    for k in ('surface', 'surface_top', 'support', 'surface_source', 'culled', 'culled_above'):
        assert same_bits(got[k], want[k]), (what, k, int((got[k].cpu() != want[k]).sum()))
    assert tuple(int(x) for x in m.support_counts.cpu()) == want['counts'], what
    assert tuple(int(x) for x in m.surface_counts.cpu()) == want['counts'][::2], what


# ---- 1. the rank words ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M', [1, 2, 3, 4])
@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_rank_words_equal_the_restatement_in_every_form(key, M):
    views, Js, axes, gsd, *_ = scene_case(key)
    T = 0.005
    want = oracle(key, T, M)
    n = want['support'].numpy()
    print(f'{key}, M = {M}: {want["Wm"]} x {want["Hm"]} cells, support histogram {np.bincount(n.reshape(-1), minlength=5).tolist()}, culled below '
          f'{want["counts"][0]}, above {want["counts"][1]} of {want["counts"][2]} samples')
    assert int((n == M).sum()) > 0 and (M == 1 or int(((n > 0) & (n < M)).sum()) > 0)      # of the restatement: full and partial support
    assert (want['counts'][1] > 0) == (M > 1)
    first = None
    for kw in (dict(), dict(batch=1), dict(batch=4), dict(batch=32), dict(plain_atomic=True), dict(batch=4, plain_atomic=True), dict()):
        m = engine.mosaic_of(views, Js, axes, gsd, surface=T, support=M, **kw)
        assert m.rank.dtype == torch.int64 and tuple(m.rank.shape) == (M, m.Hm * m.Wm)
        check_ranks(m, want, (key, M, kw))
        assert m.result()['surface_support'] == M and type(m.result()['surface_support']) is int
        if first is None:
            first = m.result()
        for k, v in first.items():      # two runs, every form: the same bits
            assert same_bits(m.result()[k], v) if torch.is_tensor(v) else m.result()[k] == v, (kw, k)


@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_a_reversed_request_gives_the_same_surface(key):
    views, Js, axes, gsd, *_ = scene_case(key)
    rviews, rJs, *_ = scene_case(key + ' reversed')
    T = 0.005
    for M in (2, 3):
        fwd = engine.mosaic_of(views, Js, axes, gsd, surface=T, support=M).result()
        m = engine.mosaic_of(rviews, rJs, axes, gsd, surface=T, support=M)
        check_ranks(m, oracle(key + ' reversed', T, M), (key, M, 'reversed'))
        rev = m.result()
        for k in ('surface', 'surface_top', 'support', 'culled', 'culled_above'):      # values: the ordinals differ, these do not
            assert same_bits(rev[k], fwd[k]), (M, k)
        # the source as image names: the same image, unless several images hold the top's height to the bit -- an exact tie goes to
        # the earlier image of the request, so there both orders name one of the holders (the restatement says which cells)
        _, _, _, _, hv, hJ = scene_case(key)
        want_cells = m.Hm * m.Wm
        every = pref.ranks(*samples_of(hv, hJ, axes, gsd), want_cells, len(views))      # every image's top of every cell
        high, low = (every >> np.uint64(32)).astype(np.int64), (every & np.uint64(0xffffffff)).astype(np.int64)
        top = m.top.cpu().numpy().view(np.uint32).astype(np.int64)
        holds = (high == top[None, :]) & (every != pref.NO_RANK)
        tied = holds.sum(axis=0) > 1
        assert int(tied.sum()) < 0.01 * want_cells
        a = fwd['surface_source'].cpu().numpy().reshape(-1)
        b = rev['surface_source'].cpu().numpy().reshape(-1)
        b = np.where(b >= 0, len(views) - 1 - b, -1)      # the reversed request's ordinal as the image's place in the forward one
        assert [views[i].name for i in range(len(views))] == [rviews[len(views) - 1 - i].name for i in range(len(views))]
        assert np.array_equal(a[~tied], b[~tied])
        for c in np.nonzero(tied)[0]:
            holders = set(low[holds[:, c], c].tolist())
            assert a[c] in holders and b[c] in holders, c


# ---- 2. tiny shapes ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 9), (3, 523), (207, 333)]      # H x W; 523 columns cross two 256-lane segments; 207 x 333: 270 workgroups


def device_view(depth, name, tx=0.0, ty=0.0):
    H, W = depth.shape
    return engine.DeviceView(depth=depth.to(DEV).contiguous(), rgb=torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), K=WIDE_K,
                             R=torch.eye(3), t=torch.tensor([[tx], [ty], [0.0]]), name=name)


def by_hand(views, Js, T, M, gsd, plain_level=None, split=None):
    """begin, every level over every image (in one call, or in two at ``split``), finish_support, one counted cull: what the
    three entries of the library leave, and the restatement of it."""
    hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
    want = pref.support(hv, hJ, torch.eye(3), gsd, T, M)
    m = engine.Mosaic(torch.eye(3), gsd, DEV)
    m.add_bounds(views, Js)
    m.begin(surface=T, support=M)
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']) and bool((m.rank == -1).all())
    parts = [(0, len(views))] if split is None else [(0, split), (split, len(views))]
    for level in range(M):
        for a, b in parts:
            m.add_support(views[a:b], Js[a:b], a, level, plain_atomic=level == plain_level)
    m.finish_support()
    culled = m.culled_images(views, Js, 0, count=True)
    return m, want, culled


def check_by_hand(m, want, culled, what):
    check_ranks(m, want, what)
    for i, (J, w) in enumerate(zip(culled, want['Js'])):
        assert J.dtype == torch.float32 and same_bits(J, w), (what, i)


@pytest.mark.parametrize('M', [1, 2, 4])
def test_every_size_and_mask_in_one_call(M):
    """16 images of four sizes with the four masks in one call: the rank words, the top, the culled copy and the counts."""
    views, Js = [], []
    for i, (H, W, kind) in enumerate((H, W, kind) for H, W in SIZES for kind in MASKS):
        depth, J = masked_image(H, W, kind, 6000 + i)
        views.append(device_view(depth, f'{H}x{W} {kind}'))
        Js.append(J.to(DEV))
    m, want, culled = by_hand(views, Js, 0.02, M, 0.05, plain_level=0 if M == 4 else None)
    assert want['counts'][0] > 0 and (want['counts'][1] > 0) == (M > 1) and want['counts'][0] + want['counts'][1] < want['counts'][2]
    check_by_hand(m, want, culled, M)
    kept = torch.cat([J.reshape(-1) for J in culled])
    assert bool(torch.isinf(kept).any()) and bool(((kept == 0) & torch.signbit(kept)).any()) and bool((kept.abs() > 1024).any())
    for i in (0, 7, 13):      # one image at a time: its block starts the buffer; not counted again
        alone = m.culled_images([views[i]], [Js[i]], i)[0]
        assert same_bits(alone, want['Js'][i]), views[i].name
    assert tuple(int(x) for x in m.support_counts.cpu()) == want['counts']


def test_forty_images_cross_a_launch():
    views, Js = [], []
    for i in range(40):
        depth, J = masked_image(8, 8, MASKS[i % 4], 7000 + i)
        views.append(device_view(depth, f'{i}'))
        Js.append(J.to(DEV))
    m, want, culled = by_hand(views, Js, 0.02, 4, 0.02)
    assert int((want['support'] == 4).sum()) > 0 and want['counts'][0] > 0 and want['counts'][1] > 0
    held = want['rank'] != pref.NO_RANK
    assert int((want['rank'][held] & np.uint64(0xffffffff)).max()) >= 32       # an image of the second launch holds a cell's level
    check_by_hand(m, want, culled, 'forty')
    m2, _, culled2 = by_hand(views, Js, 0.02, 4, 0.02, split=7)      # the same in two calls per level
    check_by_hand(m2, want, culled2, 'forty, split')


def flat_image(H, W, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.full((H, W), d), torch.rand((H, W, 3), generator=g)


def test_exact_ties_and_cells_with_one_two_and_three_images():
    """Hand-built: four identical 2 x 2 images at one place -- a four-way exact tie of a_n in their cells --, and cells that exactly
    one, two and three images of different heights reach, at M = 4."""
    # (tx, depth): with 0.05 m cells the groups land in cells 6, 0, 2 and 4 of row 0, 0.1 of a cell or more away from every border
    spec = [(0.31, 1.0)] * 4 + [(0.0, 1.0), (0.11, 1.0), (0.11, 1.1), (0.21, 1.0), (0.21, 1.1), (0.21, 1.2)]
    views, Js = [], []
    for i, (tx, d) in enumerate(spec):
        depth, J = flat_image(2, 2, d, 8000 + i)
        views.append(device_view(depth, f'{i}', tx=tx))
        Js.append(J.to(DEV))
    m, want, culled = by_hand(views, Js, 0.05, 4, 0.05, split=3)
    n, rank = want['support'].numpy().reshape(-1), want['rank']
    assert {1, 2, 3, 4} <= set(n.tolist())
    tie = np.nonzero(n == 4)[0]
    assert len(tie) > 0
    for c in tie:      # one height, the ordinals 0, 1, 2, 3 in this order
        assert len({int(w) >> 32 for w in rank[:, c]}) == 1 and [int(w) & 0xffffffff for w in rank[:, c]] == [0, 1, 2, 3]
    check_by_hand(m, want, culled, 'hand-built')
    got = m.result()
    two, three = got['support'] == 2, got['support'] == 3
    assert bool((got['surface'][two] == np.float32(1.1)).all()) and bool((got['surface'][three] == np.float32(1.2)).all())      # the lowest of the tops
    assert bool((got['surface_top'][two | three] == 1.0).all()) and bool((got['culled_above'][two | three] > 0).all())


def test_one_image_alone_at_four_views_equals_one_view():
    depth, J = masked_image(37, 53, 'NaN patch', 8100)
    views, Js = [device_view(depth, 'alone')], [J.to(DEV)]
    m4, want4, culled4 = by_hand(views, Js, 0.2, 4, 0.05)
    m1, want1, culled1 = by_hand(views, Js, 0.2, 1, 0.05)
    check_by_hand(m4, want4, culled4, 'alone, M = 4')
    check_by_hand(m1, want1, culled1, 'alone, M = 1')
    assert want4['counts'][0] > 0 and want4['counts'][1] == 0
    assert same_bits(m4.top, m1.top) and same_bits(m4.rank[0], m1.rank[0]) and bool((m4.rank[1:] == -1).all())
    assert same_bits(culled4[0], culled1[0]) and same_bits(m4.support_counts, m1.support_counts)
    for k, v in m1.result().items():
        if k != 'surface_support':
            assert same_bits(m4.result()[k], v) if torch.is_tensor(v) else m4.result()[k] == v, k


# ---- 3. one supporting view is the surface test -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', TOLS)
@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_one_supporting_view_equals_the_surface_test_bit_for_bit(key, T):
    views, Js, axes, gsd, *_ = scene_case(key)
    half = np.float32(gsd * np.float32(0.5))       # half the default gsd: holes for the fill
    for g, kw in ((gsd, dict(blend=BLEND_H, feather=8, bands=3)), (half, dict(blend=BLEND_H, feather=8, bands=2, fill=3 * float(half)))):
        old = engine.mosaic_of(views, Js, axes, g, surface=T, **kw)
        m = engine.mosaic_of(views, Js, axes, g, surface=T, support=1, **kw)
        was, got = old.result(), m.result()
        assert [k for k in got if k not in NEW] == list(was) and [k for k in got if k in NEW] == list(NEW)
        for k, v in was.items():
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, (key, T, k)
        assert same_bits(m.top, old.top) and same_bits(m.surface_counts, old.surface_counts) and same_bits(m.acc, old.acc)
        assert same_bits(m.acc_bands, old.acc_bands)
        assert not bool(got['culled_above'].any()) and int(m.support_counts[1]) == 0 and same_bits(got['surface_top'], got['surface'])
        assert torch.equal(got['support'] == 1, got['source'] >= 0) and torch.equal(got['surface_source'] >= 0, got['source'] >= 0)
        if T == 0.005:
            assert int(m.support_counts[0]) > 0
        if 'fill' in kw:
            assert int((got['fill_level'] > 0).sum()) > 0


# ---- 4. the two-sided cull --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', TOLS)
@pytest.mark.parametrize('M', [2, 3])
@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_the_two_sided_cull_equals_the_restatement(key, M, T):
    views, Js, axes, gsd, *_ = scene_case(key)
    want = oracle(key, T, M, whole=True)
    print(f'{key}, M = {M}, T = {T}: culled below {want["counts"][0]}, above {want["counts"][1]} of {want["counts"][2]} samples, in '
          f'{int((want["culled"] > 0).sum())} and {int((want["culled_above"] > 0).sum())} cells')
    if T == 0.005:      # of the restatement: both sides cull, and not everything
        assert want['counts'][0] > 0 and want['counts'][1] > 0 and want['counts'][0] + want['counts'][1] < 0.95 * want['counts'][2]
    if T == 1e6:
        assert want['counts'][:2] == (0, 0)
    m = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, surface=T, support=M, batch=4)
    check_ranks(m, want, (key, M, T))
    got = m.result()
    for k in BEST + BLENDED:
        assert same_bits(got[k], want[k]), (key, M, T, k)
    assert same_bits(m.acc, want['acc'])
    for at in (0, 4):      # the culled copy itself, batch by batch; not counted again
        for J, w in zip(m.culled_images(views[at:at + 4], Js[at:at + 4], at), want['Js'][at:at + 4]):
            assert same_bits(J, w)
    assert tuple(int(x) for x in m.support_counts.cpu()) == want['counts']
    plain = unflagged(key, blend=BLEND_H).result()
    filled = got['source'] >= 0
    assert torch.equal(filled, plain['source'] >= 0) and int(filled.sum()) == int((plain['source'] >= 0).sum())      # the filled set, n_filled
    assert (m.Hm, m.Wm) == tuple(plain['source'].shape)
    assert torch.equal(got['support'] > 0, filled) and bool(torch.isfinite(got['surface'][filled]).all()) and bool(torch.isnan(got['surface'][~filled]).all())
    assert bool((got['culled_above'][~filled] == 0).all()) and bool((got['surface_source'][~filled] == -1).all())
    if T == 1e6:      # nothing culled: every other output byte for byte
        for k, v in plain.items():
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, (key, M, k)


@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_a_tolerance_that_culls_nothing_leaves_the_fill_and_the_bands_alone(key):
    views, Js, axes, gsd, *_ = scene_case(key)
    half = np.float32(gsd * np.float32(0.5))
    kw = dict(blend=BLEND_H, feather=8, bands=2, fill=3 * float(half))
    was = engine.mosaic_of(views, Js, axes, half, **kw).result()
    got = engine.mosaic_of(views, Js, axes, half, surface=1e6, support=3, **kw).result()
    assert [k for k in got if k not in NEW + ('surface', 'culled', 'surface_tol')] == list(was)
    for k, v in was.items():
        assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert int((got['fill_level'] > 0).sum()) > 0 and not bool(got['culled'].any()) and not bool(got['culled_above'].any())


# ---- 5. the fish ------------------------------------------------------------------------------------------------------------------------

def test_a_fish_in_one_view_no_longer_owns_its_cells():
    hv, hJ = crafted.survey()
    views = [engine.DeviceView(depth=v.depth.to(DEV), rgb=v.rgb.to(DEV), K=v.K, R=v.R, t=v.t, name='ABC'[i]) for i, v in enumerate(hv)]
    Js = [J.to(DEV) for J in hJ]
    axes, T, fish = torch.eye(3), crafted.TOL, crafted.FISH_VIEW
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * 3)
    assert float(gsd) == float(np.float32(crafted.GSD))
    want = pref.expected(hv, hJ, axes, gsd, T, 2, H=BLEND_H)
    px, cell = want['cells'][fish]      # the patch, from the restatement alone
    is_fish = np.isin(px, crafted.fish_pixels())
    reached = sorted(set(cell[is_fish].tolist()))
    wholly = set(reached) - set(cell[~is_fish].tolist())
    assert len(wholly) >= 30            # some tens of cells, completely
    patch = torch.zeros(want['Hm'] * want['Wm'], dtype=torch.bool)
    patch[reached] = True
    patch = patch.view(want['Hm'], want['Wm']).to(DEV)
    fish_px = torch.from_numpy(crafted.fish_pixels()).to(DEV)

    old = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, surface=T)
    was = old.result()
    assert bool((was['source'][patch] == fish).all()) and bool(torch.isin(was['pixel'][patch].long(), fish_px).all())
    assert bool((was['culled'][patch] > 0).all()) and not bool(was['culled'][~patch].any())      # the plane's samples there are culled
    assert bool((was['surface'][patch] == crafted.FISH).all())
    colour = torch.tensor(crafted.FISH_COLOUR, device=DEV)
    assert bool((was['J'][patch] == colour).all())

    m = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, surface=T, support=2)
    got = m.result()
    check_ranks(m, want, 'fish')
    for k in BEST + BLENDED:
        assert same_bits(got[k], want[k]), k
    by_fish_view = got['source'] == fish
    assert bool(by_fish_view.any()) and not bool(torch.isin(got['pixel'][by_fish_view].long(), fish_px).any())
    assert not bool((got['J'] == colour).all(dim=-1).any())
    assert bool(((got['surface'][patch] - crafted.PLANE).abs() <= T).all())
    assert torch.equal(got['culled_above'] > 0, patch)
    assert int(m.support_counts[1]) == len(crafted.fish_pixels())
    for k in ('J', 'source', 'surface'):
        assert same_bits(got[k][~patch], was[k][~patch]), k
    assert torch.equal(got['source'] >= 0, was['source'] >= 0)
    n_filled = int((got['source'] >= 0).sum())
    print(f'fish: {len(reached)} of {n_filled} filled cells reached by the patch ({len(wholly)} wholly); with the plain minimum the fish owns '
          f'{int((was["source"][patch] == fish).sum())} of them and {int(was["culled"].sum())} samples of the plane are culled; with two views none, '
          f'{int(got["culled_above"].sum())} samples culled above; {int(((got["support"] < 2) & (got["source"] >= 0)).sum())} filled cells rest on one view')


# ---- 6. argument checks -----------------------------------------------------------------------------------------------------------------

def test_the_entries_check_their_arguments_before_any_launch():
    views, Js, *_ = scene_case('scene')
    m = engine.Mosaic(torch.eye(3), 1.0, DEV)
    arr, n, table, keep = m._images(views[:2], Js[:2])
    lib = _lib.load()
    n_bytes = lib.sucre_mosaic_band_bytes(n, arr)
    buf = torch.full((n_bytes,), 0x5a, dtype=torch.uint8, device=DEV)
    rank = torch.full((4, 4), -1, dtype=torch.int64, device=DEV)
    top = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    sup, src = torch.full((4,), 7, dtype=torch.int32, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV)
    culled, above = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 1.0, 0.0, 0.0, 2, 2
    bad = _lib.MosaicGrid()
    bad.axes, bad.gsd, bad.Hm, bad.Wm = g.axes, 0.0, 2, 2
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    tp, bp, rp, kp, up, op, cp, ap, np_ = (ptr(x) for x in (table, buf, rank, top, sup, src, culled, above, counts))
    support, form, cull = lib.sucre_mosaic_support, lib.sucre_mosaic_support_top, lib.sucre_mosaic_cull_supported
    err = lib.sucre_last_error
    tol, G = C.c_float(0.1), C.byref(g)
    with torch.cuda.device(DEV):
        assert support(None, n, arr, 0, G, 4, 0, rp, 0, sp) == -1 and b'table' in err()
        assert support(tp, 0, arr, 0, G, 4, 0, rp, 0, sp) == -1 and b'n_images' in err()
        assert support(tp, n, arr, -1, G, 4, 0, rp, 0, sp) == -1 and b'ordinals' in err()
        assert support(tp, n, arr, 0, None, 4, 0, rp, 0, sp) == -1 and b'grid' in err()
        assert support(tp, n, arr, 0, C.byref(bad), 4, 0, rp, 0, sp) == -1 and b'gsd' in err()
        for n_levels in (0, 5, -1):
            assert support(tp, n, arr, 0, G, n_levels, 0, rp, 0, sp) == -1 and b'n_levels' in err()
            assert form(G, n_levels, rp, kp, up, op, sp) == -1 and b'n_levels' in err()
        for n_levels, level in ((4, 4), (4, -1), (1, 1), (2, 3)):
            assert support(tp, n, arr, 0, G, n_levels, level, rp, 0, sp) == -1 and b'level=' in err()
        assert support(tp, n, arr, 0, G, 4, 0, None, 0, sp) == -1 and b'rank_dev' in err()
        assert support(tp, n, arr, 0, G, 4, 0, ptr(rank, 4), 0, sp) == -1 and b'aligned' in err()
        assert support(tp, n, arr, 0, G, 4, 0, rp, 2, sp) == -1 and b'flags' in err()
        assert form(None, 4, rp, kp, up, op, sp) == -1 and b'grid' in err()
        assert form(G, 4, None, kp, up, op, sp) == -1 and b'rank_dev' in err()
        assert form(G, 4, ptr(rank, 4), kp, up, op, sp) == -1 and b'rank_dev' in err()
        assert form(G, 4, rp, None, up, op, sp) == -1 and b'top_dev' in err()
        assert form(G, 4, rp, ptr(top, 2), up, op, sp) == -1 and b'top_dev' in err()
        assert form(G, 4, rp, kp, ptr(sup, 2), op, sp) == -1 and b'support_out' in err()
        assert form(G, 4, rp, kp, up, ptr(src, 2), sp) == -1 and b'source_out' in err()
        assert cull(None, n, arr, 0, G, kp, tol, bp, cp, ap, np_, sp) == -1 and b'table' in err()
        assert cull(tp, engine.MAX_VIEWS + 1, arr, 0, G, kp, tol, bp, cp, ap, np_, sp) == -1 and b'n_images' in err()
        assert cull(tp, n, arr, 0, None, kp, tol, bp, cp, ap, np_, sp) == -1 and b'grid' in err()
        assert cull(tp, n, arr, 0, G, None, tol, bp, cp, ap, np_, sp) == -1 and b'top_dev' in err()
        assert cull(tp, n, arr, 0, G, ptr(top, 2), tol, bp, cp, ap, np_, sp) == -1 and b'top_dev' in err()
        for t in (0.0, -0.1, NAN, float('inf')):
            assert cull(tp, n, arr, 0, G, kp, C.c_float(t), bp, cp, ap, np_, sp) == -1 and b'tol' in err()
        assert cull(tp, n, arr, 0, G, kp, tol, None, cp, ap, np_, sp) == -1 and b'J_out' in err()
        assert cull(tp, n, arr, 0, G, kp, tol, ptr(buf, 2), cp, ap, np_, sp) == -1 and b'aligned' in err()
        assert cull(tp, n, arr, 0, G, kp, tol, bp, ptr(culled, 2), ap, np_, sp) == -1 and b'culled_dev' in err()
        assert cull(tp, n, arr, 0, G, kp, tol, bp, cp, ptr(above, 2), np_, sp) == -1 and b'culled_above_dev' in err()
        assert cull(tp, n, arr, 0, G, kp, tol, bp, cp, ap, ptr(counts, 4), sp) == -1 and b'counts_dev' in err()
        assert cull(tp, n, arr, 0, G, kp, tol, ptr(Js[1], 12), cp, ap, np_, sp) == -1 and b'overlaps' in err()
        torch.cuda.synchronize()
    assert bool((buf == 0x5a).all()) and bool((rank == -1).all()) and bool((top == -1).all()) and bool((sup == 7).all()) and bool((src == 7).all())
    assert not bool(culled.any()) and not bool(above.any()) and not bool(counts.any())      # nothing ran


def test_methods_refuse_what_they_cannot_do():
    views, Js, axes, gsd, *_ = scene_case('scene')
    m = engine.Mosaic(axes, gsd, DEV)
    for call in (lambda: m.add_support(views, Js, 0, 0), lambda: m.finish_support()):
        with pytest.raises(ValueError, match=r'begin\(\) comes first'):
            call()
    for bad in (0, 5, -1, 2.5, True, NAN, 'x'):
        with pytest.raises(ValueError, match='supporting views M') as e:
            m.begin(bounds=(0.0, 0.0, 1.0, 1.0), surface=0.1, support=bad)
        assert e.value.field == 'support'
    with pytest.raises(ValueError, match=r'Mosaic.begin: the support decides which top') as e:
        m.begin(bounds=(0.0, 0.0, 1.0, 1.0), support=2)
    assert e.value.field == 'support' and m.key is None and m.rank is None      # refused before anything is allocated
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), surface=0.1)
    assert m.support is None and m.rank is None and not set(NEW) & set(m.result())
    for call in (lambda: m.add_support(views, Js, 0, 0), lambda: m.finish_support()):
        with pytest.raises(ValueError, match='was not given a support'):
            call()
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), surface=0.25, support=3)
    assert m.support == 3 and tuple(m.rank.shape) == (3, m.Hm * m.Wm) and m.result()['surface_support'] == 3
    with pytest.raises(_lib.SucreError, match='level='):
        m.add_support(views, Js, 0, 3)
    old = os.environ.get('SUCRE_MOSAIC_MAX_CELLS')
    os.environ['SUCRE_MOSAIC_MAX_CELLS'] = '3'
    try:
        with pytest.raises(ValueError, match=r'a support of 4 views holds 32 more bytes per cell') as e:
            m.begin(bounds=(0.0, 0.0, 1.0, 1.0), surface=0.25, support=4)
        assert e.value.field == 'grid'
    finally:
        if old is None:
            del os.environ['SUCRE_MOSAIC_MAX_CELLS']
        else:
            os.environ['SUCRE_MOSAIC_MAX_CELLS'] = old


def test_result_holds_the_rows_of_the_table():
    views, Js, axes, gsd, *_ = scene_case('scene')
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    best = [('J', (3,), f32, NAN), ('raw', (3,), u8, 0), ('source', (), i32, -1), ('pixel', (), i32, -1), ('range', (), f32, NAN)]
    blend = [('J_blend', (3,), f32, NAN), ('raw_blend', (3,), u8, 0), ('weight', (), f32, 0), ('samples', (), i32, 0)]
    bands = [('J_multiband', (3,), f32, NAN)]
    surface = [('surface', (), f32, NAN), ('culled', (), i32, 0)]
    new = [('support', (), i32, 0), ('surface_source', (), i32, -1), ('culled_above', (), i32, 0), ('surface_top', (), f32, NAN)]
    for kw, rows, scalars in (({}, best + surface, ['surface_tol']),
                              ({'blend': BLEND_H, 'feather': 8, 'bands': 3}, best + blend + bands + surface, ['feather', 'bands', 'surface_tol'])):
        m = engine.Mosaic(axes, gsd, DEV)
        m.add_bounds(views, Js)
        Hm, Wm = m.begin(surface=0.05, support=2, **kw)
        empty = m.result()          # begun, nothing seen: every cell holds its empty value
        assert list(empty) == [r[0] for r in rows] + scalars + [r[0] for r in new] + ['surface_support']
        for key, tail, dtype, value in rows + new:
            t = empty[key]
            assert (key, tail, dtype) == (key,) + engine.MOSAIC_OUTPUTS[key][1:3]
            assert tuple(t.shape) == (Hm, Wm) + tail and t.dtype == dtype and t.device == torch.device(DEV) and t.is_contiguous(), key
            assert bool(torch.isnan(t).all()) if value != value else bool((t == value).all()), key
        got = engine.mosaic_of(views, Js, axes, gsd, surface=0.05, support=2, fill=0.3, **kw).result()
        filled = [k for k, row in engine.MOSAIC_OUTPUTS.items() if row[0] in ('fill',) + (('blend_fill',) if 'blend' in kw else ())
                  + (('bands_fill',) if 'bands' in kw else ())]
        assert list(got) == [r[0] for r in rows] + scalars + [r[0] for r in new] + ['surface_support'] + filled


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
CLI_M = 2


@pytest.fixture(scope='module')
def support_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_support_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    rest = ['--mosaic-blend', '0.5', '--mosaic-feather', '8', '--mosaic-fill', '0.05', '--mosaic-bands', '2']
    runs = {'plain': rest}
    for T in TOLS:
        runs[f'surface {T}'] = rest + ['--mosaic-surface', str(T)]
        runs[f'one {T}'] = rest + ['--mosaic-surface', str(T), '--mosaic-support', '1']
    runs['two'] = ['--mosaic-blend', '0.5', '--mosaic-surface', str(TOLS[0]), '--mosaic-support', str(CLI_M)]
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


LINE = re.compile(r"^mosaic support of (\d+) views: (\d+) of (\d+) filled cells rest on fewer than (\d+); (\d+) of (\d+) samples \((\S+) %\) stand "
                  r"more than (\S+) m above their cell's supported top, in (\d+) cells$")


@pytest.mark.parametrize('T', TOLS)
def test_cli_with_one_view_writes_the_surface_test_s_files_byte_for_byte(support_run, T):
    from PIL import Image as PILImage
    root, scene, restored, printed, _ = support_run
    without, run = f'surface {T}', f'one {T}'
    before = sorted(p.name for p in (root / without).iterdir())
    assert sorted(p.name for p in (root / run).iterdir()) == sorted(before + ['mosaic_culled_above.png'])
    for name in before:
        if name != 'mosaic.pt':
            assert (root / without / name).read_bytes() == (root / run / name).read_bytes(), (run, name)
    was, got = torch.load(root / without / 'mosaic.pt'), torch.load(root / run / 'mosaic.pt')
    assert set(got) - set(was) == set(NEW) and not set(was) - set(got)
    for k, v in was.items():
        assert same_bits(v, got[k]) if torch.is_tensor(v) else v == got[k], (run, k)
    assert got['surface_support'] == 1 and not bool(got['culled_above'].any()) and same_bits(got['surface_top'], got['surface'])
    assert not np.asarray(PILImage.open(root / run / 'mosaic_culled_above.png')).any()
    lines_was, lines = printed[without].splitlines(), printed[run].splitlines()
    at = next(i for i, line in enumerate(lines_was) if line.startswith('mosaic surface of ')) + 1
    assert lines[:at] == lines_was[:at] and lines[at + 1:] == lines_was[at:] and len(lines) == len(lines_was) + 1
    hit = LINE.match(lines[at])
    assert hit, lines[at]
    n_filled = int((got['source'] >= 0).sum())
    assert hit.groups() == ('1', '0', str(n_filled), '1', '0', hit.group(6), '0.0', f'{T:.6g}', '0')
    assert 'mosaic support' not in printed[without] and 'mosaic support' not in printed['plain']


def test_cli_with_two_views_writes_what_the_engine_computes(support_run):
    from PIL import Image as PILImage
    from sucre_amd import sfm
    root, scene, restored, printed, _ = support_run
    names = [v.name for v in scene.views]
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    T = TOLS[0]
    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, surface=T, support=CLI_M, batch=4)
    got = torch.load(root / 'two' / 'mosaic.pt')
    assert set(NEW) <= set(got) and got['surface_support'] == CLI_M
    for k, v in m.result().items():
        assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert sorted(p.name for p in (root / 'two').iterdir()) == sorted(
        ['mosaic.png', 'mosaic_raw.png', 'mosaic_source.png', 'mosaic.pt', 'mosaic_blend.png', 'mosaic_blend_raw.png', 'mosaic_surface.png',
         'mosaic_culled.png', 'mosaic_culled_above.png'])
    assert np.array_equal(np.asarray(PILImage.open(root / 'two' / 'mosaic_culled_above.png')), sucre.mosaic_culled_picture(got['culled_above'].numpy()))
    assert np.array_equal(np.asarray(PILImage.open(root / 'two' / 'mosaic_surface.png')), sucre.mosaic_surface_picture(got['surface'].numpy()))
    below, above, part = (int(x) for x in m.support_counts.cpu())
    lines = printed['two'].splitlines()
    at = next(i for i, line in enumerate(lines) if line.startswith('mosaic surface of '))
    hit = LINE.match(lines[at + 1])
    assert hit, lines[at + 1]
    filled = got['source'] >= 0
    assert above > 0 and int(got['culled_above'].sum()) == above and int(got['culled'].sum()) == below
    assert hit.groups() == (str(CLI_M), str(int(((got['support'] < CLI_M) & filled).sum())), str(int(filled.sum())), str(CLI_M), str(above), str(part),
                            f'{100.0 * above / part:.1f}', f'{T:.6g}', str(int((got['culled_above'] > 0).sum())))
    assert f'{below} of {part} samples' in lines[at]
    assert got['n_filled'] == torch.load(root / 'plain' / 'mosaic.pt')['n_filled']


def test_cli_refuses_a_lone_flag_and_a_bad_value(support_run):
    root, _, restored, _, base = support_run
    out = ['--output-dir', str(root / 'refused')]
    for extra in (['--mosaic-support', '2'], ['--mosaic', str(restored), '--mosaic-support', '2']):
        with pytest.raises(SystemExit) as e:
            sucre.main(base + out + extra)
        assert e.value.code == '--mosaic-support: only with --mosaic-surface T'
    for bad, shown in (('0', '0'), ('5', '5'), ('1.5', '1.5'), ('nan', 'nan')):
        with pytest.raises(SystemExit) as e:
            sucre.main(base + out + ['--mosaic', str(restored), '--mosaic-surface', '0.05', '--mosaic-support', bad])
        assert e.value.code == f'--mosaic-support: M must be an integer within [1, 4] views, not {shown}'
    assert not (root / 'refused').exists()
