"""GPU tests of the multi-band mosaic blend (sucre_mosaic_band_split / _band_combine, engine.Mosaic, sucre.mosaic, --mosaic-bands).

The yardstick is tests/mosaic_bands_ref.py, a numpy restatement that shares no code with the engine (float32 arithmetic on
shifted arrays, the blend's and the feather's own restatements for every band's sums, float64 quotients);
test_mosaic_bands_host.py checks it against plain loops over the definition.  Every comparison is EXACT, bit for bit, NaN
included: the stack is a fixed chain of IEEE operations, the sums are integers, so no schedule, order or split may move a bit.
"""
import contextlib
import ctypes as C
import io
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_bands_ref as mref
import mosaic_blend_ref as bref
import mosaic_feather_ref as fref
import mosaic_fill_ref as fill_ref
import mosaic_ref as ref
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
BEST = ('J', 'raw', 'source', 'pixel', 'range')
BLENDED = ('J_blend', 'raw_blend', 'weight', 'samples')
_CACHE = {}


def host_view(v):
    """What the restatement reads of a DeviceView."""
    return SimpleNamespace(depth=v.depth.cpu(), rgb=v.rgb.cpu(), K=v.K, R=v.R, t=v.t, Kinv=v.Kinv)


def same_bits(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- a. the stack -------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 9), (5, 1), (3, 523), (37, 53)]     # H x W; 523 columns cross two 256-lane segments, every step above 4 is wider than 3 rows
MASKS = ['all', 'none', 'one member', 'one hole', 'checkerboard', 'NaN patch', 'depth hole', 'columns out']
PLAIN_K = torch.tensor([[100.0, 0.0, 10.0], [0.0, 100.0, 10.0], [0.0, 0.0, 1.0]])


def masked_image(H, W, kind, seed):
    """(depth (H,W), J (H,W,3)) float32 CPU tensors with the non-members of ``kind``; J holds +-inf, values beyond +-1024 and -0.0."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand((H, W), generator=g) + 0.5
    J = torch.rand((H, W, 3), generator=g) * 3 - 1
    special = torch.tensor([float('inf'), -float('inf'), 5000.0, -1024.5, -0.0, 1024.0])
    hit = torch.rand((H, W, 3), generator=g) < 0.05
    J[hit] = special[torch.randint(0, len(special), (int(hit.sum()),), generator=g)]
    if H * W > 1:
        J[0, 0] = torch.tensor([float('inf'), -0.0, -2000.0])
    if kind == 'none':
        depth[:] = 0
    elif kind == 'one member':
        keep = depth[H // 2, W // 2].clone()
        depth[:] = -1.0
        depth[H // 2, W // 2] = keep
    elif kind == 'one hole':
        J[H // 2, W // 2, 1] = NAN
    elif kind == 'checkerboard':
        v, u = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
        depth[(v + u) % 2 == 1] = 0
    elif kind == 'NaN patch':
        J[H // 4:H // 4 + max(1, H // 3), W // 4:W // 4 + max(1, W // 3)] = NAN
    elif kind == 'depth hole':
        depth[H // 3:H // 3 + max(1, H // 2), W // 2:W // 2 + max(1, W // 5)] = NAN
    elif kind == 'columns out':
        depth[:, W // 3::4] = 0
    else:
        assert kind == 'all'
    return depth, J


def device_view(depth, name='masked'):
    H, W = depth.shape
    return engine.DeviceView(depth=depth.to(DEV).contiguous(), rgb=torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), K=PLAIN_K,
                             R=torch.eye(3), t=torch.zeros(3, 1), name=name)


def stack_cases():
    """Every size with every mask, 40 images, and the 207 x 333 image with four masks: (views, Js, host depths, host Js) -- made
    once, never changed."""
    if 'stack' not in _CACHE:
        views, Js, depths, hJ = [], [], [], []
        cases = [(H, W, kind) for H, W in SIZES for kind in MASKS] + [(207, 333, kind) for kind in ('all', 'checkerboard', 'NaN patch', 'columns out')]
        for i, (H, W, kind) in enumerate(cases):
            depth, J = masked_image(H, W, kind, 2000 + i)
            member = fref.members(depth.numpy(), J.numpy())
            assert {'all': member.all(), 'none': not member.any(), 'one member': member.sum() == 1}.get(kind, True)
            views.append(device_view(depth, f'{H}x{W} {kind}'))
            Js.append(J.to(DEV))
            depths.append(depth.numpy())
            hJ.append(J.numpy())
        _CACHE['stack'] = (views, Js, depths, hJ)
    return _CACHE['stack']


def stack_oracle(i, K):
    if ('stack', i, K) not in _CACHE:
        _, _, depths, hJ = stack_cases()
        _CACHE[('stack', i, K)] = mref.stack(depths[i], hJ[i], K)
    return _CACHE[('stack', i, K)]


def check_stack(got, i, K, name):
    want = stack_oracle(i, K)
    assert len(got) == K + 1
    for j, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == torch.float32 and tuple(x.shape) == y.shape
        assert same_bits(x, torch.from_numpy(y)), (name, K, j, int((x.cpu().view(torch.int32) != torch.from_numpy(y).view(torch.int32)).sum()))


@pytest.mark.parametrize('K', [1, 3, 6])
def test_the_stack_of_every_size_and_mask_in_one_call_equals_the_restatement(K):
    """40 images of five sizes in one call: two launches, the second one's pixels behind the first one's.  Bit for bit, so NaN
    exactly at the non-members of every band, an infinity clamped, -0.0 kept."""
    views, Js, depths, hJ = stack_cases()
    stacks = engine.Mosaic(torch.eye(3), 1.0, DEV).band_stack(views[:40], Js[:40], K)
    assert len(stacks) == 40
    for i, got in enumerate(stacks):
        check_stack(got, i, K, views[i].name)
        member = fref.members(depths[i], hJ[i])
        for band in got:
            assert np.array_equal(np.isnan(band.cpu().numpy()), np.repeat(~member[:, :, None], 3, axis=2)), views[i].name


@pytest.mark.parametrize('K', [1, 3, 6])
def test_the_stack_of_a_larger_image_of_a_mixed_batch_and_of_one_image_at_a_time(K):
    views, Js, _, _ = stack_cases()
    m = engine.Mosaic(torch.eye(3), 1.0, DEV)
    order = [40, 3, 41, 33, 42, 0, 43, 28]      # 207 x 333 images between small ones: every block starts at a multiple of 256 pixels
    for i, got in zip(order, m.band_stack([views[i] for i in order], [Js[i] for i in order], K)):
        check_stack(got, i, K, views[i].name)
    for i in (0, 12, 30, 39):
        check_stack(m.band_stack([views[i]], [Js[i]], K)[0], i, K, views[i].name)


def test_the_entries_check_their_arguments_before_any_launch():
    views, Js, _, _ = stack_cases()
    m = engine.Mosaic(torch.eye(3), 1.0, DEV)
    arr, n, table, keep = m._images(views[32:34], Js[32:34])
    lib = _lib.load()
    n_bytes = lib.sucre_mosaic_band_bytes(n, arr)
    assert n_bytes == 12 * sum(-(-(e.H * e.W) // 256) * 256 for e in arr)
    assert lib.sucre_mosaic_band_bytes(0, arr) == 0 and b'n_images' in lib.sucre_last_error()
    assert lib.sucre_mosaic_band_bytes(engine.MAX_VIEWS + 1, arr) == 0
    assert lib.sucre_mosaic_band_bytes(n, None) == 0
    bufs = [torch.full((n_bytes,), 0x5a, dtype=torch.uint8, device=DEV) for _ in range(3)]
    a, b, c = (C.c_void_p(x.data_ptr()) for x in bufs)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp = C.c_void_p(table.data_ptr())
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 1.0, 0.0, 0.0, 1, 1
    acc = torch.zeros((7, 1, 8), dtype=torch.int64, device=DEV)
    acc[:, 0, 6:] = 4096
    out = torch.full((1, 1, 3), 7.0, device=DEV)
    ap, op = C.c_void_p(acc.data_ptr()), C.c_void_p(out.data_ptr())
    split, combine = lib.sucre_mosaic_band_split, lib.sucre_mosaic_band_combine
    with torch.cuda.device(DEV):
        for level in (6, -1, 7):
            assert split(tp, n, arr, level, a, b, c, sp) == -1 and b'level' in lib.sucre_last_error()
        assert split(tp, n, arr, 1, None, b, c, sp) == -1 and b'S_in' in lib.sucre_last_error()
        assert split(tp, n, arr, 0, a, b, c, sp) == -1 and b'S_in' in lib.sucre_last_error()
        assert split(tp, n, arr, 0, None, None, c, sp) == -1 and b'S_out' in lib.sucre_last_error()
        assert split(tp, n, arr, 0, None, b, None, sp) == -1 and b'D_out' in lib.sucre_last_error()
        assert split(tp, n, arr, 0, None, C.c_void_p(bufs[1].data_ptr() + 2), c, sp) == -1 and b'aligned' in lib.sucre_last_error()
        for S_in, S_out, D_out in ((a, a, c), (a, b, a), (a, b, b), (a, C.c_void_p(bufs[0].data_ptr() + n_bytes - 4), c)):
            assert split(tp, n, arr, 1, S_in, S_out, D_out, sp) == -1 and b'overlap' in lib.sucre_last_error()
        assert split(tp, n, arr, 0, None, b, b, sp) == -1 and b'overlap' in lib.sucre_last_error()
        assert split(None, n, arr, 0, None, b, c, sp) == -1 and b'table' in lib.sucre_last_error()
        assert split(tp, 0, arr, 0, None, b, c, sp) == -1 and b'n_images' in lib.sucre_last_error()
        for n_bands in (1, 8, 0, -2):
            assert combine(C.byref(g), n_bands, ap, op, sp) == -1 and b'n_bands' in lib.sucre_last_error()
        assert combine(None, 2, ap, op, sp) == -1 and b'grid' in lib.sucre_last_error()
        assert combine(C.byref(g), 2, None, op, sp) == -1 and b'acc_bands_dev' in lib.sucre_last_error()
        assert combine(C.byref(g), 2, ap, None, sp) == -1 and b'J_out' in lib.sucre_last_error()
        assert combine(C.byref(g), 2, C.c_void_p(acc.data_ptr() + 4), op, sp) == -1 and b'aligned' in lib.sucre_last_error()
        torch.cuda.synchronize()
    assert all(bool((x == 0x5a).all()) for x in bufs) and bool((out == 7.0).all())      # nothing ran


# ---- b. the accumulators and the picture --------------------------------------------------------------------------------------------
BLEND_H = 0.5


def restored_like(view, seed):
    """A stand-in for a restored image: random colours, NaN in two patches and in single channels of scattered pixels."""
    H, W = view.depth.shape
    g = torch.Generator().manual_seed(seed)
    J = torch.rand((H, W, 3), generator=g) * 0.98 + 0.01
    for _ in range(2):
        v0, u0 = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
        J[v0:v0 + max(1, H // 6), u0:u0 + max(1, W // 6)] = NAN
    hit = torch.rand((H, W), generator=g) < 0.02
    ch = torch.randint(0, 3, (H, W), generator=g)
    vv, uu = torch.nonzero(hit, as_tuple=True)
    J[vv, uu, ch[vv, uu]] = NAN
    return J.to(DEV)


def scene_case(key):
    """(views, Js, axes, gsd, host views, host Js, best-view reference, per image D2) of the small survey (test_gpu_mosaic.py's)
    or the deep scene, in the request's order or (``key`` ending in ' reversed') reversed -- made once, never changed."""
    if key not in _CACHE:
        if key.endswith(' reversed'):
            views, Js, axes, gsd, hv, hJ, _, near = scene_case(key[:-len(' reversed')])
            views, Js, hv, hJ, near = views[::-1], Js[::-1], hv[::-1], hJ[::-1], near[::-1]
        else:
            scene = synth.make_survey(96, 64, 3, 2) if key == 'survey' else synth.make_deep_scene(96, 64, 6)
            views = engine.device_views_from_scene(scene, DEV)
            Js = [restored_like(v, 300 + k) for k, v in enumerate(views)]
            axes = sucre.mosaic_axes(views)
            gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
            hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
            near = [fref.nearest2(fref.members(v.depth.numpy(), J.numpy())) for v, J in zip(hv, hJ)]
        _CACHE[key] = (views, Js, axes, gsd, hv, hJ, ref.mosaic(hv, hJ, axes, gsd), near)
    return _CACHE[key]


def oracle(key, F, K):
    ck = (key, F, K)
    if ck not in _CACHE:
        views, Js, axes, gsd, hv, hJ, base, near = scene_case(key)
        _CACHE[ck] = mref.multiband(hv, hJ, axes, gsd, BLEND_H, F, K, base=base, near=near)
    return _CACHE[ck]


def blend_oracle(key, F):
    ck = (key, F, 'blend')
    if ck not in _CACHE:
        views, Js, axes, gsd, hv, hJ, base, near = scene_case(key)
        _CACHE[ck] = bref.blend(hv, hJ, axes, gsd, BLEND_H, base=base) if F is None else fref.blend(hv, hJ, axes, gsd, BLEND_H, F, base=base, near=near)
    return _CACHE[ck]


@pytest.mark.parametrize('F', [None, 1, 8])
@pytest.mark.parametrize('K', [1, 4])
@pytest.mark.parametrize('key', ['survey', 'deep'])
def test_the_accumulators_and_the_picture_equal_the_restatement(key, K, F):
    """``acc_bands`` word for word and ``J_multiband``: both forms of the accumulate, batches of 1, 4 and 32 images, a second run,
    and the reversed request against its own restatement.  The residual's words 3..7 are the blend's; ``acc`` is not touched."""
    views, Js, axes, gsd, hv, hJ, base, near = scene_case(key)
    want, blend = oracle(key, F, K), blend_oracle(key, F)
    m = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, bands=K)
    got = m.result()
    least = [int(want['acc_bands'][j, :, 6][want['acc_bands'][K, :, 7] > 0].min()) for j in range(K + 1)]
    print(f'{key}, K = {K}, F = {F}: {base["Wm"]} x {base["Hm"]} cells, plan {m.band_plan}, samples per band '
          f'{[int(want["acc_bands"][j, :, 7].sum()) for j in range(K + 1)]}, smallest weight sums {least}')
    assert (m.Hm, m.Wm) == (base['Hm'], base['Wm']) and got['bands'] == K == m.bands and m.band_plan == mref.plan(BLEND_H, F, K)
    assert tuple(m.acc_bands.shape) == (K + 1, m.Hm * m.Wm, 8) and m.acc_bands.dtype == torch.int64
    assert same_bits(m.acc_bands, want['acc_bands']), int((m.acc_bands.cpu() != want['acc_bands']).sum())
    assert same_bits(got['J_multiband'], want['J_multiband']), int((got['J_multiband'].cpu().view(torch.int32) != want['J_multiband'].view(torch.int32)).sum())
    assert same_bits(m.acc, blend['acc']) and same_bits(m.acc_bands[K, :, 3:], m.acc[:, 3:])
    assert min(least) >= 4 and all(x >= 4096 for x in least if F in (None, 1))
    filled = got['source'] >= 0
    assert bool(torch.isfinite(got['J_multiband'][filled]).all()) and bool(torch.isnan(got['J_multiband'][~filled]).all())
    assert not same_bits(got['J_multiband'], got['J_blend'])
    others = [engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, bands=K, plain_atomic=True),
              engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, bands=K, batch=1),
              engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, bands=K, batch=4),
              engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, bands=K)]
    for other in others:
        assert same_bits(other.acc_bands, m.acc_bands) and same_bits(other.result()['J_multiband'], got['J_multiband'])
        assert same_bits(other.acc, m.acc)
    rv, rJ, *_ = scene_case(key + ' reversed')
    want_r = oracle(key + ' reversed', F, K)
    r = engine.mosaic_of(rv, rJ, axes, gsd, blend=BLEND_H, feather=F, bands=K)
    assert same_bits(r.acc_bands, want_r['acc_bands']) and same_bits(r.result()['J_multiband'], want_r['J_multiband'])


@pytest.mark.parametrize('key', ['survey', 'deep'])
def test_a_map_made_at_the_bands_own_width_gives_the_same_words(key):
    """Every band reads the map made at the user's F; a map of its own, made at F_j <= F, gives the same accumulator."""
    views, Js, axes, gsd, *_ = scene_case(key)
    K, F = 4, 8
    want = oracle(key, F, K)
    m = engine.Mosaic(axes, gsd, DEV)
    m.add_bounds(views, Js)
    m.begin(blend=BLEND_H, feather=F, bands=K)
    assert [f for _, f in m.band_plan] == [1, 1, 2, 4, 8]
    m.splat(views, Js, 0)
    images = m._images(views, Js)
    bufs, first = m._band_buffers(images)
    for j, buf in m._band_levels(images, K, bufs):      # accumulate_bands by hand, with a map of its own for every band
        own, maps = m._feather_pass(images, m.band_plan[j][1])
        assert 1 <= int(max(d.max() for d in maps)) <= m.band_plan[j][1] ** 2      # capped at the band's own width
        m._accumulate_band(images, first, j, buf, 0, 0, own)
    assert same_bits(m.acc_bands, want['acc_bands'])
    assert not bool(m.acc.any()) and not bool(m.feather_counts.any())      # the band passes touch neither


def test_a_constant_survey_stays_constant():
    views, Js, axes, gsd, *_ = scene_case('survey')
    flat = [torch.where(torch.isnan(J), J, torch.full_like(J, 0.5)) for J in Js]
    for F, K in ((None, 4), (8, 6), (1024, 1)):
        got = engine.mosaic_of(views, flat, axes, gsd, blend=BLEND_H, feather=F, bands=K).result()
        filled = got['source'] >= 0
        assert 0 < int(filled.sum()) < filled.numel()
        assert bool((got['J_multiband'][filled] == 0.5).all()) and bool(torch.isnan(got['J_multiband'][~filled]).all())


def test_images_of_several_sizes_in_one_batch_equal_the_restatement():
    """The 37 x 53 and 3 x 523 images of the stack's cases, 16 images in one call and in batches of 5: each image's band block sits
    behind the ones before it, rounded up to whole workgroups, and the accumulate reads it as that image's J."""
    views, Js, _, _ = stack_cases()
    pick = list(range(24, 40))
    views, Js = [views[i] for i in pick], [Js[i] for i in pick]
    hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
    axes, gsd, F, K = torch.eye(3), 0.05, 7, 3
    want = mref.multiband(hv, hJ, axes, gsd, BLEND_H, F, K)
    assert int((want['acc_bands'][K, :, 7] > 1).sum()) > 0
    for batch in (32, 5):
        m = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, bands=K, batch=batch)
        assert same_bits(m.acc_bands, want['acc_bands']) and same_bits(m.result()['J_multiband'], want['J_multiband'])


# ---- c. what the bands leave alone, and what result() holds -------------------------------------------------------------------------

def test_every_other_output_is_what_it_was_and_a_fill_fills_from_the_picture():
    views, Js, axes, gsd, *_ = scene_case('survey')
    gsd = np.float32(gsd * np.float32(0.5))       # half the default gsd: holes
    R = 3 * float(gsd)
    for F in (None, 8):
        was = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, fill=R).result()
        m = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, feather=F, fill=R, bands=4)
        got = m.result()
        assert list(was) == [k for k in got if k not in ('J_multiband', 'bands', 'J_multiband_filled')]
        for k, v in was.items():
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
        host = {k: v.cpu().numpy() for k, v in got.items() if torch.is_tensor(v)}
        assert int((host['source'] < 0).sum()) > 0
        want = fill_ref.fill(host['J_multiband'], host['raw_blend'], host['source'], m.fill_levels)
        assert same_bits(host['J_multiband_filled'], want['J_filled'])
        assert np.array_equal(np.isnan(host['J_multiband_filled']), np.isnan(host['J_blend_filled']))


def test_result_holds_the_rows_of_the_table():
    views, Js, axes, gsd, *_ = scene_case('survey')
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    rows = [('J', (3,), f32, NAN), ('raw', (3,), u8, 0), ('source', (), i32, -1), ('pixel', (), i32, -1), ('range', (), f32, NAN),
            ('J_blend', (3,), f32, NAN), ('raw_blend', (3,), u8, 0), ('weight', (), f32, 0), ('samples', (), i32, 0),
            ('J_multiband', (3,), f32, NAN)]
    filled_rows = [('fill_level', (), i32, None), ('J_filled', (3,), f32, None), ('raw_filled', (3,), u8, None),
                   ('J_blend_filled', (3,), f32, None), ('raw_blend_filled', (3,), u8, None), ('J_multiband_filled', (3,), f32, None)]
    for kw, keys in (({}, [r[0] for r in rows] + ['bands']),
                     ({'feather': 8}, [r[0] for r in rows] + ['feather', 'bands']),
                     ({'fill': 0.3}, [r[0] for r in rows] + ['bands'] + [r[0] for r in filled_rows]),
                     ({'feather': 8, 'fill': 0.3}, [r[0] for r in rows] + ['feather', 'bands'] + [r[0] for r in filled_rows])):
        m = engine.Mosaic(axes, gsd, DEV)
        m.add_bounds(views, Js)
        Hm, Wm = m.begin(blend=BLEND_H, bands=3, feather=kw.get('feather'))
        empty = m.result()          # begun, nothing splatted: every cell holds its empty value
        assert list(empty) == [k for k in keys if k not in [r[0] for r in filled_rows]]
        for key, tail, dtype, value in rows:
            t = empty[key]
            assert tuple(t.shape) == (Hm, Wm) + tail and t.dtype == dtype and t.device == torch.device(DEV), key
            assert bool(torch.isnan(t).all()) if value != value else bool((t == value).all()), key
        assert empty['bands'] == 3 and type(empty['bands']) is int
        assert tuple(m.acc_bands.shape) == (4, Hm * Wm, 8) and not bool(m.acc_bands.any())
        got = engine.mosaic_of(views, Js, axes, gsd, blend=BLEND_H, bands=3, **kw).result()
        assert list(got) == keys
        for key, tail, dtype, _ in rows + (filled_rows if 'fill' in kw else []):
            assert tuple(got[key].shape) == (Hm, Wm) + tail and got[key].dtype == dtype, key


def test_methods_refuse_what_they_cannot_do():
    views, Js, axes, gsd, *_ = scene_case('survey')
    m = engine.Mosaic(axes, gsd, DEV)
    with pytest.raises(ValueError, match='give the blend depth too') as e:
        m.begin(bounds=(0.0, 0.0, 1.0, 1.0), bands=4)
    assert e.value.field == 'bands'
    for bad in (0, 7, 2.5, NAN, True):
        with pytest.raises(ValueError, match='band count K'):
            m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5, bands=bad)
        with pytest.raises(ValueError, match='band count K'):
            m.band_stack(views, Js, bad)
    assert m.key is None and m.acc_bands is None      # refused before anything is allocated
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5)
    assert m.bands is None and 'bands' not in m.result() and 'J_multiband' not in m.result()
    for call in (lambda: m.accumulate_bands(views, Js, 0), m.combine_bands):
        with pytest.raises(ValueError, match='band count'):
            call()
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5, bands=2)
    assert m.bands == 2 and m.result()['bands'] == 2


# ---- d. the frequency property ------------------------------------------------------------------------------------------------------

def test_multiband_has_the_detail_of_the_best_view_and_the_colour_of_the_blend():
    """test_mosaic_bands_host.py's crafted pair on the device: to the bit the restatement's pictures, so its conditions."""
    hv, hJ = mref.frequency_pair()
    views = [engine.DeviceView(depth=v.depth.to(DEV), rgb=v.rgb.to(DEV), K=v.K, R=v.R, t=v.t, name='AB'[i], Kinv=v.Kinv) for i, v in enumerate(hv)]
    Js = [J.to(DEV) for J in hJ]
    axes, gsd = torch.eye(3), mref.PAIR_GSD
    m = engine.mosaic_of(views, Js, axes, gsd, bounds=mref.PAIR_BOUNDS, blend=mref.PAIR_H, bands=mref.PAIR_K)
    got = m.result()
    assert (m.Hm, m.Wm) == mref.PAIR_HW and bool((got['source'] == 0).all()) and bool((got['samples'] == 2).all())
    h, l, ok = mref.frequency_conditions(got['J'].cpu().numpy(), got['J_blend'].cpu().numpy(), got['J_multiband'].cpu().numpy())
    print(f'fine detail: best view {h[0]:.5f}, blend {h[1]:.5f}, multi-band {h[2]:.5f}; colour: {l[0]:.4f}, {l[1]:.4f}, {l[2]:.4f}')
    assert ok[0], h
    assert ok[1], l
    want = mref.multiband(hv, hJ, axes, gsd, mref.PAIR_H, None, mref.PAIR_K, bounds=mref.PAIR_BOUNDS)
    assert same_bits(m.acc_bands, want['acc_bands']) and same_bits(got['J_multiband'], want['J_multiband'])


# ---- e. the command line ------------------------------------------------------------------------------------------------------------
CLI_BLEND, CLI_FEATHER, CLI_FILL, CLI_BANDS = 0.5, 8, 0.05, 4


@pytest.fixture(scope='module')
def bands_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_bands_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    blend = ['--mosaic-blend', str(CLI_BLEND)]
    all_three = blend + ['--mosaic-feather', str(CLI_FEATHER), '--mosaic-fill', str(CLI_FILL)]
    bands = ['--mosaic-bands', str(CLI_BANDS)]
    runs = {'blend': blend, 'bands': blend + bands, 'all': all_three, 'all_bands': all_three + bands}
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
    return root, scene, restored, printed


LINE = re.compile(r'^mosaic multi-band blend of (\d) bands: depths ((?:\S+ )+)m, feathers ((?:\S+ )+)px; RMS difference from the blend '
                  r'R (\S+) G (\S+) B (\S+)$')


def test_cli_writes_the_multiband_picture_and_leaves_every_other_file_alone(bands_run):
    from PIL import Image as PILImage
    from sucre_amd import sfm
    root, scene, restored, printed = bands_run
    names = [v.name for v in scene.views]
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    for run, without, feather, fill in (('bands', 'blend', None, None), ('all_bands', 'all', CLI_FEATHER, CLI_FILL)):
        before = sorted(p.name for p in (root / without).iterdir())
        new = ['mosaic_multiband.png'] + (['mosaic_multiband_filled.png'] if fill else [])
        assert sorted(p.name for p in (root / run).iterdir()) == sorted(before + new)
        for name in before:
            if name != 'mosaic.pt':
                assert (root / without / name).read_bytes() == (root / run / name).read_bytes(), (run, name)
        was, got = torch.load(root / without / 'mosaic.pt'), torch.load(root / run / 'mosaic.pt')
        assert set(got) - set(was) == {'J_multiband', 'bands', 'band_plan'} | ({'J_multiband_filled'} if fill else set()) and not set(was) - set(got)
        for k, v in was.items():
            assert same_bits(v, got[k]) if torch.is_tensor(v) else v == got[k], (run, k)
        plan = engine.mosaic_band_plan(CLI_BLEND, feather, CLI_BANDS)
        assert got['bands'] == CLI_BANDS and type(got['bands']) is int
        assert got['band_plan'] == [(float(h), f) for h, f in plan] and len(got['band_plan']) == CLI_BANDS + 1
        m = engine.mosaic_of(views, Js, axes, gsd, blend=CLI_BLEND, feather=feather, fill=fill, bands=CLI_BANDS)
        for k in ('J_multiband',) + (('J_multiband_filled',) if fill else ()):
            assert same_bits(got[k], m.result()[k]), (run, k)
        for k, png in (('J_multiband', 'mosaic_multiband.png'),) + ((('J_multiband_filled', 'mosaic_multiband_filled.png'),) if fill else ()):
            assert np.array_equal(np.asarray(PILImage.open(root / run / png)), np.asarray(sucre.SUCRe.plot_J(SimpleNamespace(J=got[k], stretch=None))))
        # the lines: those of the run without the flag, with one more after the blend's and the feather's and before the fill's
        lines_was, lines = printed[without].splitlines(), printed[run].splitlines()
        at = len(lines_was) - (1 if fill else 0)
        assert lines[:at] == lines_was[:at] and lines[at + 1:] == lines_was[at:] and len(lines) == len(lines_was) + 1
        hit = LINE.match(lines[at])
        assert hit, lines[at]
        assert int(hit.group(1)) == CLI_BANDS
        assert hit.group(2).split() == [f'{float(h):.6g}' for h, _ in plan]
        assert hit.group(3).split() == ['-' if f is None else str(f) for _, f in plan]
        filled = (got['source'] >= 0)
        d = (got['J_multiband'].double() - got['J_blend'].double())[filled]
        rms = d.pow(2).mean(dim=0).sqrt()
        assert [hit.group(4 + c) for c in range(3)] == [f'{float(rms[c]):.6g}' for c in range(3)] and float(rms.max()) > 0
    assert 'multi-band' not in printed['blend'] and 'multi-band' not in printed['all']
