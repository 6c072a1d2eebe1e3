"""GPU tests of the mosaic's per-image gain compensation (sucre_mosaic_gain_span / _apply / _sums, engine.Mosaic, sucre.mosaic,
--mosaic-gains, --mosaic-gain-limit).

The yardstick is tests/mosaic_gains_ref.py, a numpy restatement that shares no code with the engine; test_mosaic_gains_host.py
checks it against plain loops over the definition.  Every comparison with it is EXACT, bit for bit: the span is an integer minimum
and maximum, the sums are integer adds of fixed float32 chains, the solve is float64 with an order-free sum.  The later stages need
no new restatement: a run with the flag must equal a run without it on the images times their gains.
"""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import mosaic_gains_crafted as crafted
import mosaic_gains_ref as gref
from test_gpu_mosaic_support import device_view
from test_gpu_mosaic_surface import MASKS, host_view, masked_image, restored_like, same_bits
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
ROUNDS = 3
GAIN_KEYS = ('gains', 'gain_sums', 'gain_rms', 'gain_overlap', 'gain_rounds', 'gain_limit')
FACTORS = [(0.8, 0.85, 0.9), (1.25, 1.2, 1.1), (1.0, 1.0, 1.0), (0.9, 1.1, 0.95), (1.15, 0.82, 1.05), (1.2, 1.0, 0.8), (0.95, 1.05, 1.25)]
_CACHE = {}


def scene_case(key):
    """(views, Js, axes, gsd, host views, host Js) of ``synth.make_scene(96, 64, 6)`` or ``make_deep_scene(96, 64, 6)``, the stand-in
    restored image of view i times ``FACTORS[i]`` -- made once, never changed."""
    if key not in _CACHE:
        scene = synth.make_scene(96, 64, 6) if key == 'scene' else synth.make_deep_scene(96, 64, 6)
        views = engine.device_views_from_scene(scene, DEV)
        Js = [(restored_like(v, 900 + k) * torch.tensor(FACTORS[k % len(FACTORS)], device=DEV)).contiguous() for k, v in enumerate(views)]
        axes = sucre.mosaic_axes(views)
        gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
        _CACHE[key] = (views, Js, axes, gsd, [host_view(v) for v in views], [J.cpu() for J in Js])
    return _CACHE[key]


def oracle(key, R=ROUNDS, L=2.0):
    ck = (key, 'gains', R, L)
    if ck not in _CACHE:
        _, _, axes, gsd, hv, hJ = scene_case(key)
        _CACHE[ck] = gref.gains(hv, hJ, axes, gsd, R, L)
    return _CACHE[ck]


def check_gains(m, want, what, order=None):
    """``span``, every sum word, the gains, the RMS and the overlap of ``m`` against the restatement's, bit for bit; ``order``: the
    request was that permutation of the restatement's."""
    got = m.result()
    n = len(want['gains'])
    order = list(range(n)) if order is None else list(order)
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']), what
    span = m.span.cpu().numpy().view(np.uint32)
    ws = want['span']
    if order != list(range(n)):      # ordinal i of the request is image order[i] of the restatement; here: reversed
        assert order == list(range(n))[::-1]
        seen = ws[:, 0] != gref.NO_LO
        ws = np.where(seen[:, None], np.stack([n - 1 - ws[:, 1], n - 1 - ws[:, 0]], axis=1), ws).astype(np.uint32)
    assert np.array_equal(span, ws), (what, 'span')
    assert got['gain_sums'].dtype == torch.int64 and tuple(got['gain_sums'].shape) == want['sums'].shape, what
    assert np.array_equal(got['gain_sums'].cpu().numpy(), want['sums'][:, order]), (what, 'sums')
    assert got['gains'].dtype == torch.float32 and same_bits(got['gains'], torch.from_numpy(want['gains'][order].copy())), (what, 'gains')
    assert got['gain_rms'].dtype == torch.float64 and np.array_equal(got['gain_rms'].numpy(), want['rms']), (what, 'rms')
    assert got['gain_overlap'].dtype == torch.int64 and np.array_equal(got['gain_overlap'].cpu().numpy(), want['overlap'][order]), (what, 'overlap')
    assert got['gain_rounds'] == len(want['sums']) - 1 and type(got['gain_rounds']) is int and type(got['gain_limit']) is float


# ---- 1. exactness -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_span_sums_and_gains_equal_the_restatement_in_every_form(key):
    views, Js, axes, gsd, hv, hJ = scene_case(key)
    want = oracle(key)
    shared = want['span'][:, 0] < want['span'][:, 1]
    print(f'{key}: {want["Wm"]} x {want["Hm"]} cells, {int(shared.sum())} shared; overlap {want["overlap"].tolist()}; gains '
          f'{want["gains"].tolist()}; rms {want["rms"].tolist()}')
    # conditions on the restatement, not on the code under test: the case has shared and unshared cells, and gains that moved
    assert shared.any() and (~shared & (want['span'][:, 0] != gref.NO_LO)).any() and bool((want['overlap'] > 0).all())
    assert not np.array_equal(want['gains'], np.ones_like(want['gains']))
    for batch, plain in ((1, False), (5, False), (32, False), (32, True), (4, True)):
        m = engine.mosaic_of(views, Js, axes, gsd, gains=ROUNDS, batch=batch, plain_atomic=plain)
        check_gains(m, want, (key, batch, plain))
        assert same_bits(m.acc_gain, torch.from_numpy(want['acc'])), (key, batch, plain)
    m = engine.mosaic_of(views[::-1], Js[::-1], axes, gsd, gains=ROUNDS, batch=4)       # the same gains per image name
    check_gains(m, want, (key, 'reversed'), order=range(len(views))[::-1])


# ---- 2. every size and mask, launch boundaries, the clamp, a view listed twice ------------------------------------------------------------
SIZES = [(45, 61), (20, 24), (64, 96), (1, 9)]      # H x W: no pixel count is a multiple of 256; 64 x 96 = 24 blocks


def by_hand(views, Js, gsd, R, L=2.0, splits=(), plain=False):
    """begin, splat, span and R rounds by the methods, in one call per phase or cut at ``splits`` (every batch with the ordinal of
    its first image)."""
    cuts = [0, *splits, len(views)]
    batches = [(a, lambda a=a, b=b: (views[a:b], Js[a:b])) for a, b in zip(cuts, cuts[1:])]
    m = engine.Mosaic(torch.eye(3), gsd, DEV)
    m.add_bounds(views, Js)
    m.begin(gains=R, gain_limit=L)
    assert bool((m.span[:, 0] == -1).all()) and not bool(m.span[:, 1].any()) and not bool(m.acc_gain.any())
    for first, load in batches:
        m.splat(*load(), first)
    for first, load in batches:
        m.add_span(*load(), first, plain_atomic=plain)
    for _ in range(R):
        m.gain_pass(batches, plain=plain)
        m.solve_gains()
    m.gain_pass(batches, plain=plain)
    return m


def mixed_request():
    """16 images of four sizes with the four masks around one place, one image far from all others, one with samples at 20.0 and
    +-inf, and image 2 once more."""
    if 'mixed' not in _CACHE:
        views, Js = [], []
        for i, (H, W, kind) in enumerate((H, W, kind) for H, W in SIZES for kind in MASKS):
            depth, J = masked_image(H, W, kind, 8000 + i)
            views.append(device_view(depth, f'{H}x{W} {kind}', tx=0.002 * i, ty=-0.001 * i))
            Js.append(J.to(DEV))
        views.append(device_view(torch.full((7, 13), 1.0), 'far', tx=5.0, ty=5.0))
        Js.append(torch.full((7, 13, 3), 0.5, device=DEV))
        J = torch.full((20, 24, 3), 0.75)
        J[::2, ::3] = torch.tensor([20.0, float('inf'), -float('inf')])
        views.append(device_view(torch.full((20, 24), 1.0), 'clamped'))
        Js.append(J.to(DEV))
        views.append(views[2])
        Js.append(Js[2])
        _CACHE['mixed'] = (views, Js, [host_view(v) for v in views], [J.cpu() for J in Js])
    return _CACHE['mixed']


def test_every_size_and_mask_in_one_call():
    views, Js, hv, hJ = mixed_request()
    gsd, R = 0.05, 2
    want = gref.gains(hv, hJ, torch.eye(3), gsd, R, 2.0)
    far, clamped, twice = len(views) - 3, len(views) - 2, len(views) - 1
    print(f'mixed: {want["Wm"]} x {want["Hm"]} cells; overlap {want["overlap"].tolist()}; gains {want["gains"].tolist()}')
    assert want['overlap'][far] == 0 and want['gains'][far].tolist() == [1.0] * 3                  # overlaps nothing
    assert want['overlap'][clamped] > 0 and int(want['sums'][0, clamped, 4]) >= (8 * 16384) ** 2   # 20.0 entered as 8.0
    shared = want['span'][:, 0] < want['span'][:, 1]
    for i in (2, twice):                                                                          # a view listed twice: its cells are shared
        assert bool(shared[want['samples'][i][1]].all()) and len(want['samples'][i][1]) > 0
    assert bool((want['overlap'][[i for i, v in enumerate(views) if ' none' in v.name]] == 0).all())
    assert bool((want['sums'][:, :, 1:4] <= 0).any())                                             # the path that keeps the old gain
    m = by_hand(views, Js, gsd, R)
    check_gains(m, want, 'mixed')
    assert same_bits(m.acc_gain, torch.from_numpy(want['acc']))
    check_gains(by_hand(views, Js, gsd, R, splits=(3, 4, 17), plain=True), want, 'mixed, four calls, plain')
    # the gained images: J x gain, one float32 multiply, NaN where J holds one; and once more IN PLACE (an image's J is its own block)
    G = m.gain_table
    once = m.gained_images(views, Js, 0)
    for i, (J, got) in enumerate(zip(Js, once)):
        assert got.dtype == torch.float32 and same_bits(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(J * G[i], nan=-7.0)), views[i].name
        assert torch.equal(torch.isnan(got), torch.isnan(J))
    twice_over = m._apply_gains(views, once, 0)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(once, twice_over))
    for i, (J, got) in enumerate(zip(Js, twice_over)):
        assert same_bits(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num((J * G[i]) * G[i], nan=-7.0)), views[i].name
    alone = m.gained_images([views[5]], [Js[5]], 5)[0]                                            # one image: its block starts the buffer
    assert same_bits(torch.nan_to_num(alone, nan=-7.0), torch.nan_to_num(Js[5] * G[5], nan=-7.0))


def test_forty_images_cross_a_launch_and_a_workgroup_s_walk():
    views, Js = [], []
    for i in range(40):
        depth, J = masked_image(8, 8, MASKS[i % 4], 8100 + i)
        views.append(device_view(depth, f'{i}', tx=0.001 * i))
        Js.append(J.abs().to(DEV))
    hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
    want = gref.gains(hv, hJ, torch.eye(3), 0.02, 2, 4.0)
    assert int(want['span'][:, 1].max()) >= 32 and int((want['overlap'] > 0).sum()) >= 20       # the second launch's images share cells
    check_gains(by_hand(views, Js, 0.02, 2, L=4.0), want, 'forty')
    check_gains(by_hand(views, Js, 0.02, 2, L=4.0, splits=(7,)), want, 'forty, split')           # a first_ordinal of 7
    check_gains(by_hand(views, Js, 0.02, 2, L=4.0, splits=(33,), plain=True), want, 'forty, split, plain')


# ---- 3. invariants --------------------------------------------------------------------------------------------------------------------
ALL_ON = dict(blend=0.5, feather=8, bands=3, fill=0.3, surface=0.005, support=2)


@pytest.mark.parametrize('batch', [32, 4])
def test_only_the_restored_colours_change_and_they_are_those_of_the_gained_images(batch):
    views, Js, axes, gsd, *_ = scene_case('deep')
    without = engine.mosaic_of(views, Js, axes, gsd, batch=batch, **ALL_ON)
    was = without.result()
    m = engine.mosaic_of(views, Js, axes, gsd, batch=batch, gains=ROUNDS, **ALL_ON)
    got = m.result()
    assert int(without.support_counts[0]) + int(without.support_counts[1]) > 0                    # the surface test culls here
    assert [k for k in got if k not in GAIN_KEYS] == list(was) and list(got)[-len(GAIN_KEYS):] == list(GAIN_KEYS)
    gains = got['gains']
    assert not bool((gains == 1).all()) and bool((got['gain_overlap'] > 0).all())
    scaled = engine.mosaic_of(views, [J * gains[i] for i, J in enumerate(Js)], axes, gsd, batch=batch, **ALL_ON).result()
    for k, v in was.items():
        if not torch.is_tensor(v):
            assert got[k] == v, k
        elif k.startswith('J'):
            assert same_bits(got[k], scaled[k]), (batch, k)
            assert not same_bits(got[k], v), (batch, k)                                            # and the flag did something
        else:
            assert same_bits(got[k], v) and same_bits(scaled[k], v), (batch, k)
    assert tuple(int(x) for x in m.support_counts.cpu()) == tuple(int(x) for x in without.support_counts.cpu())
    # a limit of 1: every gain is 1.0f and every key keeps its bits
    one = engine.mosaic_of(views, Js, axes, gsd, batch=batch, gains=ROUNDS, gain_limit=1, **ALL_ON).result()
    assert bool((one['gains'] == 1).all()) and one['gain_limit'] == 1.0
    assert same_bits(one['gain_sums'][0], one['gain_sums'][-1]) and same_bits(one['gain_sums'][0], got['gain_sums'][0])
    for k, v in was.items():
        assert same_bits(one[k], v) if torch.is_tensor(v) else one[k] == v, (batch, 'limit 1', k)


def test_without_any_other_option_the_best_view_is_that_of_the_gained_images():
    views, Js, axes, gsd, *_ = scene_case('scene')
    m = engine.mosaic_of(views, Js, axes, gsd, gains=2)
    got = m.result()
    was = engine.mosaic_of(views, Js, axes, gsd).result()
    scaled = engine.mosaic_of(views, [J * got['gains'][i] for i, J in enumerate(Js)], axes, gsd).result()
    assert list(got) == list(was) + list(GAIN_KEYS)
    for k in was:
        assert same_bits(got[k], scaled[k] if k == 'J' else was[k]), k


# ---- 4. the crafted survey ------------------------------------------------------------------------------------------------------------

def test_three_views_of_one_plane_agree_after_one_round():
    """Measured on an MI355X: gain x factor spread 0.5625 -> 0.000174 (bound 2^-10 = 0.000977); RMS disagreement R 0.0736 -> 0,
    G 0.0920 -> 3.5e-05, B 0.0644 -> 5.0e-05 (the restatement's figures, which the device equals to the bit); largest
    |best view - blend| 0.108 -> 3.2e-05."""
    hv, hJ = crafted.survey()
    views = [engine.DeviceView(depth=v.depth.to(DEV), rgb=v.rgb.to(DEV), K=v.K, R=v.R, t=v.t, name='ABC'[i]) for i, v in enumerate(hv)]
    Js = [J.to(DEV) for J in hJ]
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * 3)
    assert float(gsd) == float(np.float32(crafted.GSD))
    m = engine.mosaic_of(views, Js, torch.eye(3), gsd, gains=1, gain_limit=crafted.LIMIT, blend=0.5)
    got = m.result()
    before, after = crafted.spread(torch.ones(3, 3)), crafted.spread(got['gains'].cpu())
    rms = got['gain_rms']
    print(f'crafted: gain x factor spread {before:.6g} -> {after:.6g} (bound {crafted.BOUND:.6g}); RMS disagreement '
          + ' '.join(f'{ch} {float(rms[0, c]):.6g} -> {float(rms[1, c]):.6g}' for c, ch in enumerate('RGB')))
    assert after <= crafted.BOUND
    assert bool((rms[1] < rms[0]).all())
    check_gains(m, gref.gains(hv, hJ, torch.eye(3), gsd, 1, crafted.LIMIT), 'crafted')
    # The seam is gone.  All three views see every cell from one range, so the blend is the plain mean of c k_j g_j over the views
    # and the best view is c k_i g_i of one of them: they differ by at most max_j |k_i g_i - k_j g_j| c <= spread x (k g) x c, with
    # spread <= BOUND, g <= LIMIT, k <= max(FACTORS), c <= max(COLOUR); twice that covers the blend's 2^-20 fixed point.
    plain = engine.mosaic_of(views, Js, torch.eye(3), gsd, blend=0.5).result()
    filled = got['source'] >= 0
    seam_was = float((plain['J'] - plain['J_blend'])[filled].abs().max())
    seam = float((got['J'] - got['J_blend'])[filled].abs().max())
    print(f'crafted: largest |best view - blend| {seam_was:.6g} -> {seam:.6g}')
    assert seam <= 2 * crafted.BOUND * max(crafted.COLOUR) * max(crafted.FACTORS) * crafted.LIMIT < seam_was


# ---- 5. argument checks and refusals ---------------------------------------------------------------------------------------------------

def test_the_entries_check_their_arguments_before_any_launch():
    views, Js, *_ = scene_case('scene')
    m = engine.Mosaic(torch.eye(3), 1.0, DEV)
    arr, n, table, keep = m._images(views[:2], Js[:2])
    lib = _lib.load()
    n_bytes = lib.sucre_mosaic_band_bytes(n, arr)
    buf = torch.full((n_bytes,), 0x5a, dtype=torch.uint8, device=DEV)
    span = torch.tensor([-1, 0], dtype=torch.int32, device=DEV).repeat(4, 1)
    acc = torch.zeros((4, 8), dtype=torch.int64, device=DEV)
    gains = torch.ones((4, 3), dtype=torch.float32, device=DEV)
    sums = torch.zeros((4, 16), dtype=torch.int64, device=DEV)
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 1.0, 0.0, 0.0, 2, 2
    bad = _lib.MosaicGrid()
    bad.axes, bad.gsd, bad.Hm, bad.Wm = g.axes, 0.0, 2, 2
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    tp, bp, pp, ap, gp, up = (ptr(x) for x in (table, buf, span, acc, gains, sums))
    spanf, apply, sumsf = lib.sucre_mosaic_gain_span, lib.sucre_mosaic_gain_apply, lib.sucre_mosaic_gain_sums
    err, G = lib.sucre_last_error, C.byref(g)
    big = (_lib.MosaicImage * 1)()
    C.memmove(big, arr, C.sizeof(big))
    big[0].H, big[0].W = 8193, 8192           # 2^26 + 8192 pixels
    with torch.cuda.device(DEV):
        assert spanf(None, n, arr, 0, G, pp, 0, sp) == -1 and b'table' in err()
        assert spanf(tp, 0, arr, 0, G, pp, 0, sp) == -1 and b'n_images' in err()
        assert spanf(tp, engine.MAX_VIEWS + 1, arr, 0, G, pp, 0, sp) == -1 and b'n_images' in err()
        assert spanf(tp, n, arr, -1, G, pp, 0, sp) == -1 and b'ordinals' in err()
        assert spanf(tp, n, None, 0, G, pp, 0, sp) == -1 and b'images' in err()
        assert spanf(tp, n, arr, 0, None, pp, 0, sp) == -1 and b'grid' in err()
        assert spanf(tp, n, arr, 0, C.byref(bad), pp, 0, sp) == -1 and b'gsd' in err()
        assert spanf(tp, n, arr, 0, G, None, 0, sp) == -1 and b'span_dev' in err()
        assert spanf(tp, n, arr, 0, G, ptr(span, 4), 0, sp) == -1 and b'span_dev' in err()
        assert spanf(tp, n, arr, 0, G, pp, 2, sp) == -1 and b'flags' in err()
        assert apply(None, n, arr, 0, gp, 4, bp, sp) == -1 and b'table' in err()
        assert apply(tp, 0, arr, 0, gp, 4, bp, sp) == -1 and b'n_images' in err()
        assert apply(tp, n, arr, 0, gp, 0, bp, sp) == -1 and b'n_ordinals' in err()
        assert apply(tp, n, arr, 0, gp, engine.MAX_VIEWS + 1, bp, sp) == -1 and b'n_ordinals' in err()
        assert apply(tp, n, arr, 3, gp, 4, bp, sp) == -1 and b'rows of the gain table' in err()
        assert apply(tp, n, arr, 0, None, 4, bp, sp) == -1 and b'gains_dev' in err()
        assert apply(tp, n, arr, 0, ptr(gains, 2), 4, bp, sp) == -1 and b'gains_dev' in err()
        assert apply(tp, n, arr, 0, gp, 4, None, sp) == -1 and b'J_out' in err()
        assert apply(tp, n, arr, 0, gp, 4, ptr(buf, 2), sp) == -1 and b'aligned' in err()
        assert apply(tp, n, arr, 0, gp, 4, ptr(Js[1], 12), sp) == -1 and b'overlaps' in err()
        assert apply(tp, n, arr, 0, gp, 4, ptr(Js[1]), sp) == -1 and b'overlaps' in err()           # image 1's J, but as image 0's block
        assert sumsf(None, n, arr, 0, G, pp, ap, gp, 4, up, 0, sp) == -1 and b'table' in err()
        assert sumsf(tp, n, arr, 0, None, pp, ap, gp, 4, up, 0, sp) == -1 and b'grid' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, gp, 1, up, 0, sp) == -1 and b'rows of the gain table' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, gp, -1, up, 0, sp) == -1 and b'n_ordinals' in err()
        assert sumsf(tp, 1, big, 0, G, pp, ap, gp, 4, up, 0, sp) == -1 and b'2^26' in err() and b'image 0' in err()
        assert sumsf(tp, n, arr, 0, G, None, ap, gp, 4, up, 0, sp) == -1 and b'span_dev' in err()
        assert sumsf(tp, n, arr, 0, G, ptr(span, 4), ap, gp, 4, up, 0, sp) == -1 and b'span_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, None, gp, 4, up, 0, sp) == -1 and b'acc_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ptr(acc, 4), gp, 4, up, 0, sp) == -1 and b'acc_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, None, 4, up, 0, sp) == -1 and b'gains_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, ptr(gains, 2), 4, up, 0, sp) == -1 and b'gains_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, gp, 4, None, 0, sp) == -1 and b'sums_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, gp, 4, ptr(sums, 64), 0, sp) == -1 and b'sums_dev' in err()
        assert sumsf(tp, n, arr, 0, G, pp, ap, gp, 4, up, 2, sp) == -1 and b'flags' in err()
        torch.cuda.synchronize()
    assert bool((buf == 0x5a).all()) and bool((span[:, 0] == -1).all()) and not bool(span[:, 1].any())
    assert not bool(sums.any()) and not bool(acc.any()) and bool((gains == 1).all())              # nothing ran


def test_methods_refuse_what_they_cannot_do():
    views, Js, axes, gsd, *_ = scene_case('scene')
    m = engine.Mosaic(axes, gsd, DEV)
    batches = [(0, lambda: (views, Js))]
    calls = (lambda: m.add_span(views, Js, 0), lambda: m.gain_pass(batches), lambda: m.solve_gains(), lambda: m.gained_images(views, Js, 0),
             lambda: m.add_gain_reference(views, Js, 0), lambda: m.add_gain_sums(views, Js, 0))
    for call in calls:
        with pytest.raises(ValueError, match=r'begin\(\) comes first'):
            call()
    for bad in (0, 65, 2.5, True, NAN, 'x'):
        with pytest.raises(ValueError, match='gain rounds R') as e:
            m.begin(bounds=(0.0, 0.0, 1.0, 1.0), gains=bad)
        assert e.value.field == 'gains'
    with pytest.raises(ValueError, match='gain limit L') as e:
        m.begin(bounds=(0.0, 0.0, 1.0, 1.0), gains=2, gain_limit=17)
    assert e.value.field == 'gain_limit'
    with pytest.raises(ValueError, match=r'Mosaic.begin: the limit clamps the gains') as e:
        m.begin(bounds=(0.0, 0.0, 1.0, 1.0), gain_limit=2)
    assert e.value.field == 'gain_limit' and m.key is None and m.span is None                      # refused before anything is allocated
    m.add_bounds(views, Js)
    m.begin()
    assert m.gains is None and m.span is None and not set(GAIN_KEYS) & set(m.result())
    for call in calls:
        with pytest.raises(ValueError, match='was not given gain rounds'):
            call()
    m.begin(gains=1)
    assert m.gains == 1 and m.gain_limit == 2.0 and tuple(m.span.shape) == (m.Hm * m.Wm, 2) and m.gain_table is None
    empty = m.result()
    assert tuple(empty['gains'].shape) == (0, 3) and tuple(empty['gain_rms'].shape) == (0, 3) and empty['gain_rounds'] == 1
    for call in (lambda: m.add_span(views, Js, 0), lambda: m.gain_pass(batches)):
        with pytest.raises(ValueError, match=r'splat\(\) comes first'):
            call()
    with pytest.raises(ValueError, match='no gain pass has begun'):
        m.gained_images(views, Js, 0)
    m.splat(views, Js, 0)
    m.add_span(views, Js, 0)
    for call in (lambda: m.add_gain_reference(views, Js, 0), lambda: m.add_gain_sums(views, Js, 0), lambda: m.end_gain_pass()):
        with pytest.raises(ValueError, match=r'begin_gain_pass\(\) comes first'):
            call()
    with pytest.raises(ValueError, match='a whole gain pass comes first'):
        m.solve_gains()
    m.begin_gain_pass(len(views) - 1)
    with pytest.raises(ValueError, match='the gain table holds'):
        m.add_gain_reference(views, Js, 0)
    with pytest.raises(ValueError, match='the first pass saw'):
        m.begin_gain_pass(len(views))
    m.begin(gains=1)
    m.splat(views, Js, 0)
    m.add_span(views, Js, 0)
    m.gain_pass(batches)
    m.solve_gains()
    m.gain_pass(batches)
    with pytest.raises(ValueError, match='the 1 rounds and the measuring pass have run'):
        m.gain_pass(batches)
    assert tuple(m.result()['gain_sums'].shape) == (2, len(views), 10)
    m.acc_gain[0, 7] = engine.MOSAIC_MAX_SAMPLES
    with pytest.raises(ValueError, match=r'a cell holds 1048576 samples.*--mosaic-gsd') as e:
        m.check_gain_reference()
    assert e.value.field == 'gains'


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------
REST = ['--mosaic-blend', '0.5', '--mosaic-feather', '8', '--mosaic-fill', '0.05', '--mosaic-bands', '2', '--mosaic-surface', '0.005']


@pytest.fixture(scope='module')
def gains_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_gains_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    runs = {'plain': REST, 'gains': REST + ['--mosaic-gains', '3'], 'limit 1': REST + ['--mosaic-gains', '3', '--mosaic-gain-limit', '1']}
    printed = {}
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        for i, path in enumerate(sorted(restored.glob('*.pt'))):      # the images disagree by known factors
            data = torch.load(path)
            if isinstance(data, dict) and 'J' in data:
                data['J'] = (data['J'] * torch.tensor(FACTORS[i % len(FACTORS)]).to(data['J'].device)).contiguous()
                torch.save(data, path)
        for name, extra in runs.items():
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                sucre.main(base + ['--output-dir', str(root / name), '--mosaic', str(restored)] + extra)
            printed[name] = text.getvalue()
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, scene, restored, printed, base


LINE = re.compile(r'^mosaic gains of (\d+) rounds \(limit (\S+)\): (\d+) of (\d+) images share a cell with another; RMS disagreement in shared '
                  r'cells R (\S+) -> (\S+) G (\S+) -> (\S+) B (\S+) -> (\S+); largest correction (\S+) \(gain R (\S+) G (\S+) B (\S+)\); '
                  r'(\d+) values clipped$')


def test_cli_writes_what_the_engine_computes(gains_run):
    from sucre_amd import sfm
    root, scene, restored, printed, _ = gains_run
    names = [v.name for v in scene.views]
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, feather=8, fill=0.05, bands=2, surface=0.005, gains=3, batch=4)
    got = torch.load(root / 'gains' / 'mosaic.pt')
    was = torch.load(root / 'plain' / 'mosaic.pt')
    assert set(got) - set(was) == set(GAIN_KEYS) and not set(was) - set(got)
    for k, v in m.result().items():
        assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert got['gain_rounds'] == 3 and got['gain_limit'] == 2.0 and tuple(got['gain_sums'].shape) == (4, len(names), 10)
    assert not bool((got['gains'] == 1).all())
    assert sorted(p.name for p in (root / 'gains').iterdir()) == sorted(p.name for p in (root / 'plain').iterdir())
    for p in (root / 'plain').iterdir():      # every file that is no picture of J, and every key that is no J, keeps its bytes
        if 'raw' in p.name or p.name in ('mosaic_source.png', 'mosaic_surface.png', 'mosaic_culled.png', 'mosaic_filled_mask.png'):
            assert p.read_bytes() == (root / 'gains' / p.name).read_bytes(), p.name
    for k, v in was.items():
        if not k.startswith('J'):
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert not same_bits(got['J'], was['J'])
    lines, lines_was = printed['gains'].splitlines(), printed['plain'].splitlines()
    at = next(i for i, line in enumerate(lines) if line.startswith('mosaic surface of ')) + 1
    hit = LINE.match(lines[at])
    assert hit, lines[at]
    assert lines[:at] == lines_was[:at] and len(lines) == len(lines_was) + 1 and 'mosaic gains' not in printed['plain']
    rms, g = got['gain_rms'], got['gains'].double()
    far = int(g.log().abs().max(dim=1).values.argmax())
    assert hit.groups() == ('3', '2', str(int((got['gain_overlap'] > 0).sum())), str(len(names)),
                            *(f'{float(rms[r, c]):.6g}' for c in range(3) for r in (0, 3)), names[far],
                            *(f'{float(g[far, c]):.6g}' for c in range(3)), hit.group(15))
    assert bool((rms[3] < rms[0]).all())      # the survey's images disagree by FACTORS and little else


def test_cli_with_a_limit_of_one_leaves_every_file_byte_identical(gains_run):
    root, _, _, printed, _ = gains_run
    before = sorted(p.name for p in (root / 'plain').iterdir())
    assert sorted(p.name for p in (root / 'limit 1').iterdir()) == before
    for name in before:
        if name != 'mosaic.pt':
            assert (root / 'plain' / name).read_bytes() == (root / 'limit 1' / name).read_bytes(), name
    was, got = torch.load(root / 'plain' / 'mosaic.pt'), torch.load(root / 'limit 1' / 'mosaic.pt')
    assert set(got) - set(was) == set(GAIN_KEYS)
    for k, v in was.items():
        assert same_bits(v, got[k]) if torch.is_tensor(v) else v == got[k], k
    assert bool((got['gains'] == 1).all()) and got['gain_limit'] == 1.0
    hit = LINE.match(next(line for line in printed['limit 1'].splitlines() if line.startswith('mosaic gains of ')))
    assert hit and hit.group(2) == '1' and hit.group(15) == '0' and hit.groups()[11:14] == ('1', '1', '1')


def test_cli_refuses_a_lone_flag_and_a_bad_value(gains_run):
    root, _, restored, _, base = gains_run
    out = ['--output-dir', str(root / 'refused')]
    for extra, code in ((['--mosaic-gain-limit', '2'], '--mosaic-gain-limit: only with --mosaic-gains R'),
                        (['--mosaic', str(restored), '--mosaic-gain-limit', '2'], '--mosaic-gain-limit: only with --mosaic-gains R'),
                        (['--mosaic-gains', '3'], '--mosaic-gains: only with --mosaic DIR')):
        with pytest.raises(SystemExit) as e:
            sucre.main(base + out + extra)
        assert e.value.code == code
    for bad in ('0', '65', '2.5'):
        with pytest.raises(SystemExit) as e:
            sucre.main(base + out + ['--mosaic', str(restored), '--mosaic-gains', bad])
        assert e.value.code == f'--mosaic-gains: R must be an integer within [1, 64] rounds, not {bad}'
    for bad in ('0.5', '17'):
        with pytest.raises(SystemExit) as e:
            sucre.main(base + out + ['--mosaic', str(restored), '--mosaic-gains', '3', '--mosaic-gain-limit', bad])
        assert e.value.code == f'--mosaic-gain-limit: L must be a finite limit within [1, 16] times, not {float(bad)}'
    assert not (root / 'refused').exists()
