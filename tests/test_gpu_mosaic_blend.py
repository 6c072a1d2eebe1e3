"""GPU tests of the blended seabed mosaic (sucre_mosaic_accumulate / _normalize, engine.Mosaic, sucre.mosaic, --mosaic-blend).

The yardstick is tests/mosaic_blend_ref.py, a numpy restatement that shares no code with the engine (float32 weights one
operation per line, int64 sums, a float64 quotient); test_mosaic_blend_host.py checks it on a blend computed by hand.  Every
comparison is EXACT: the sums are integers, so neither the order of arrival nor the split into calls may move a bit.
"""
import contextlib
import ctypes as C
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_blend_ref as bref
import mosaic_ref as ref
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BLENDED = ('J_blend', 'raw_blend', 'weight', 'samples')
BEST = ('source', 'pixel', 'range', 'J', 'raw')
_CASES = {}


def restored_like(view, seed):
    """Random float32 in (0, 1) with NaN patches: two rectangles with all channels NaN and about 2 % of the pixels with a NaN in one."""
    H, W = view.depth.shape
    g = torch.Generator().manual_seed(seed)
    J = torch.rand((H, W, 3), generator=g) * 0.98 + 0.01
    for _ in range(2):
        v0, u0 = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
        J[v0:v0 + max(1, H // 6), u0:u0 + max(1, W // 6)] = float('nan')
    hit = torch.rand((H, W), generator=g) < 0.02
    ch = torch.randint(0, 3, (H, W), generator=g)
    vv, uu = torch.nonzero(hit, as_tuple=True)
    J[vv, uu, ch[vv, uu]] = float('nan')
    return J.to(DEV)


def host_view(v):
    """What the oracle reads of a DeviceView."""
    return SimpleNamespace(depth=v.depth.cpu(), rgb=v.rgb.cpu(), K=v.K, R=v.R, t=v.t, Kinv=v.Kinv)


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def views_of(key):
    """(views, Js, axes, default gsd) of a scene -- made once and never changed."""
    if key not in _CASES:
        if key == 'survey':
            scene = synth.make_survey(96, 64, 3, 2)
        elif key == 'deep':
            scene = synth.make_deep_scene(96, 64, 6)
        elif key == 'odd':
            scene = synth.make_scene(333, 207, 1, seed=5)
        else:
            scene = synth.make_survey(24, 16, 11, 3, seed=2)   # 33 views: one more than a launch table holds
        views = engine.device_views_from_scene(scene, DEV)
        Js = [restored_like(v, 300 + k) for k, v in enumerate(views)]
        axes = sucre.mosaic_axes(views)
        gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
        _CASES[key] = (views, Js, axes, gsd)
    return _CASES[key]


def best_view(key, gsd_factor=1.0):
    ck = (key, 'best', gsd_factor)
    if ck not in _CASES:
        views, Js, axes, gsd = views_of(key)
        _CASES[ck] = ref.mosaic([host_view(v) for v in views], [J.cpu() for J in Js], axes, np.float32(gsd * np.float32(gsd_factor)))
    return _CASES[ck]


def oracle(key, H, gsd_factor=1.0):
    ck = (key, 'blend', float(H), gsd_factor)
    if ck not in _CASES:
        views, Js, axes, gsd = views_of(key)
        _CASES[ck] = bref.blend([host_view(v) for v in views], [J.cpu() for J in Js], axes, np.float32(gsd * np.float32(gsd_factor)), H,
                                base=best_view(key, gsd_factor))
    return _CASES[ck]


def quarter_spread(key, gsd_factor=1.0):
    """A quarter of the spread of the winning ranges: deep enough to blend neighbours, shallow enough to give many pixels weight 0."""
    r = best_view(key, gsd_factor)['range'].numpy()
    return float(np.float32(0.25) * (np.nanmax(r) - np.nanmin(r)))


def check_against_oracle(m, want, what):
    got = m.result()
    base = want['base']
    assert (m.Hm, m.Wm) == (base['Hm'], base['Wm']), what
    wq = want['wq']
    print(f'{what}: {base["Wm"]} x {base["Hm"]} cells, {int((want["samples"] > 0).sum())} filled, {int(want["samples"].sum())} samples of '
          f'{len(wq)} pixels, {int(want["samples"].max())} in a cell at most, {int(((wq > 0) & (wq < 4096)).sum())} weights strictly inside')
    assert same_bits(m.acc, want['acc']), (what, 'acc', int((m.acc.cpu() != want['acc']).sum()))
    for k in BLENDED:
        assert same_bits(got[k], want[k]), (what, k, int((got[k].cpu() != want[k]).sum()))
    for k in BEST:
        assert same_bits(got[k], base[k]), (what, k)
    assert not bool(torch.isnan(got['J_blend'][got['samples'] > 0]).any())
    assert torch.equal(got['samples'] > 0, got['source'] >= 0)


def test_dense_collisions_equal_the_oracle_and_leave_the_best_view_alone():
    """Six views, about 17 pixels per cell at the default gsd."""
    views, Js, axes, gsd = views_of('survey')
    H = quarter_spread('survey')
    want = oracle('survey', H)
    filled = want['samples'] > 0
    assert int((want['samples'][filled] > 1).sum()) * 3 >= int(filled.sum())
    assert bool(((want['wq'] > 0) & (want['wq'] < 4096)).any()) and bool((want['wq'] == 0).any())
    m = engine.mosaic_of(views, Js, axes, gsd, blend=H)
    check_against_oracle(m, want, f'survey, default gsd, H = {H:.4f} m')
    plain = engine.mosaic_of(views, Js, axes, gsd)
    assert set(plain.result()) == set(BEST) and plain.acc is None
    assert all(same_bits(plain.result()[k], m.result()[k]) for k in BEST)


def test_fine_grid_equals_the_oracle():
    """A quarter of the default gsd: few collisions, many cells with a single sample."""
    views, Js, axes, gsd = views_of('survey')
    H = quarter_spread('survey', 0.25)
    want = oracle('survey', H, 0.25)
    m = engine.mosaic_of(views, Js, axes, np.float32(gsd * np.float32(0.25)), blend=H)
    check_against_oracle(m, want, 'survey, gsd / 4')
    assert int((want['samples'] == 1).sum()) > 0.3 * int((want['samples'] > 0).sum())


def test_deep_scene_does_not_depend_on_order_run_or_variant():
    """Ranges from 0.7 m to 8 m.  Another request order, a second run and the plain accumulate variant: the same bytes."""
    views, Js, axes, gsd = views_of('deep')
    H = quarter_spread('deep')
    want = oracle('deep', H)
    a = engine.mosaic_of(views, Js, axes, gsd, blend=H)
    check_against_oracle(a, want, f'deep scene, H = {H:.4f} m')
    perm = [4, 0, 6, 2, 5, 1, 3]
    b = engine.mosaic_of([views[i] for i in perm], [Js[i] for i in perm], axes, gsd, blend=H)
    again = engine.mosaic_of(views, Js, axes, gsd, blend=H)
    plain = engine.mosaic_of(views, Js, axes, gsd, blend=H, plain_atomic=True)    # one set of atomics per pixel, in splat and accumulate
    for other in (b, again, plain):
        assert same_bits(other.acc, a.acc)
        assert all(same_bits(other.result()[k], a.result()[k]) for k in BLENDED)


def test_thirty_three_views_in_one_call_and_in_calls_of_five_equal_the_oracle():
    views, Js, axes, gsd = views_of('many')
    assert len(views) == 33
    gsd = np.float32(gsd * np.float32(0.25))
    H = quarter_spread('many', 0.25)
    want = oracle('many', H, 0.25)
    m = engine.mosaic_of(views, Js, axes, gsd, batch=33, blend=H)    # one call per phase: two launches each
    check_against_oracle(m, want, '33 views in one call')
    split = engine.mosaic_of(views, Js, axes, gsd, batch=5, blend=H)
    assert same_bits(split.acc, m.acc) and all(same_bits(split.result()[k], m.result()[k]) for k in BLENDED)


def test_an_odd_sized_image_equals_the_oracle():
    views, Js, axes, gsd = views_of('odd')
    assert tuple(views[0].depth.shape) == (207, 333)
    H = quarter_spread('odd')
    m = engine.mosaic_of(views, Js, axes, gsd, blend=H)
    check_against_oracle(m, oracle('odd', H), '333 x 207')


def test_the_shallowest_blend_is_the_best_view_quantised():
    """H = 1e-6 m: in a cell whose only sample is an untied winner, J_blend is J rounded to 2^-20 -- within 2^-21 of it for
    colours in (0, 1) -- and raw_blend is raw."""
    views, Js, axes, gsd = views_of('survey')
    gsd = np.float32(gsd * np.float32(0.25))
    want = oracle('survey', 1e-6, 0.25)
    m = engine.mosaic_of(views, Js, axes, gsd, blend=1e-6)
    check_against_oracle(m, want, 'survey, gsd / 4, H = 1e-6 m')
    got = {k: v.cpu() for k, v in m.result().items()}
    alone = (got['samples'] == 1) & (want['base']['ties'] == 1)
    assert int(alone.sum()) > 1000
    J = got['J'][alone].numpy()
    rounded = (np.rint(J * np.float32(1048576)).astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(got['J_blend'][alone].numpy(), rounded)
    assert float(np.abs(got['J_blend'][alone].numpy().astype(np.float64) - J.astype(np.float64)).max()) <= 2.0 ** -21
    assert torch.equal(got['raw_blend'][alone], got['raw'][alone])
    assert torch.equal(got['weight'][alone], torch.ones(int(alone.sum())))


def test_the_deepest_blend_is_the_plain_mean():
    """H = 1e6 m: every weight is 4096, J_blend the integer mean of the quantised colours of the cell."""
    views, Js, axes, gsd = views_of('survey')
    want = oracle('survey', 1e6)
    assert bool((want['wq'] == 4096).all())
    m = engine.mosaic_of(views, Js, axes, gsd, blend=1e6)
    check_against_oracle(m, want, 'survey, H = 1e6 m')
    got = {k: v.cpu() for k, v in m.result().items()}
    acc = want['acc'].numpy()
    filled = acc[:, 7] > 0
    assert np.array_equal(acc[:, 6], 4096 * acc[:, 7]) and not (acc[:, 0:6] % 4096).any()
    mean = ((acc[filled, 0:3] // 4096).astype(np.float64) / acc[filled, 7:8].astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(got['J_blend'].reshape(-1, 3)[torch.from_numpy(filled)].numpy(), mean)
    assert torch.equal(got['weight'], got['samples'].float())


TIE_K = torch.tensor([[16.0, 0.0, 8.0], [0.0, 16.0, 4.0], [0.0, 0.0, 1.0]])


def tie_case(J):
    """The 16x8 image of test_gpu_mosaic.py's tie test (dyadic intrinsics, identity pose, depth 1): host view, device view."""
    depth = torch.ones(8, 16)
    rgb = (torch.arange(8 * 16 * 3) % 251).to(torch.uint8).reshape(8, 16, 3)
    host = SimpleNamespace(depth=depth, rgb=rgb, K=TIE_K, R=torch.eye(3), t=torch.zeros(3, 1), Kinv=TIE_K.inverse())
    dev = engine.DeviceView(depth=depth.to(DEV), rgb=rgb.to(DEV), K=TIE_K, R=torch.eye(3), t=torch.zeros(3, 1), name='tie', Kinv=TIE_K.inverse())
    return host, dev


def test_out_of_range_colours_are_clamped_and_make_no_nan():
    J = torch.rand((8, 16, 3), generator=torch.Generator().manual_seed(12)) * 4 - 2
    inf = float('inf')
    J[0, 0, 0], J[0, 1, 1], J[3, 7, 2], J[4, 8, 0], J[2, 2, 1], J[7, 15, 2] = inf, -inf, inf, 1e6, -5000.0, -inf
    host, dev = tie_case(J)
    want = bref.blend([host], [J], torch.eye(3), 4.0, 1.0)
    assert (want['base']['Hm'], want['base']['Wm']) == (1, 1) and int(want['samples'][0, 0]) == 128
    assert not bool(torch.isnan(want['J_blend']).any())
    m = engine.mosaic_of([dev], [J.to(DEV)], torch.eye(3), 4.0, blend=1.0)
    check_against_oracle(m, want, 'one cell with infinities')
    assert bool(torch.isfinite(m.result()['J_blend']).all())


def one_cell_plane(H, W, seed):
    """An H x W view of a plane at depth 1 through a 2^20-pixel focal length: a footprint of a millimetre, one 4 m cell."""
    K = torch.tensor([[2.0 ** 20, 0.0, W / 2], [0.0, 2.0 ** 20, H / 2], [0.0, 0.0, 1.0]])
    Kinv = torch.tensor([[2.0 ** -20, 0.0, -(W / 2) * 2.0 ** -20], [0.0, 2.0 ** -20, -(H / 2) * 2.0 ** -20], [0.0, 0.0, 1.0]])
    g = torch.Generator().manual_seed(seed)
    J = torch.rand((H, W, 3), generator=g)
    rgb = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    view = engine.DeviceView(depth=torch.ones((H, W), device=DEV), rgb=rgb.to(DEV), K=K, R=torch.eye(3), t=torch.zeros(3, 1), name='plane', Kinv=Kinv)
    return view, J, rgb


def test_a_cell_of_2_to_the_20_samples_is_refused_and_one_of_1024_fewer_is_the_exact_mean():
    """The bound of the 64-bit sums.  H = 1e6 m, so every weight is 4096 and the expected values need no geometry."""
    view, J, rgb = one_cell_plane(1024, 1024, 21)
    m = engine.Mosaic(torch.eye(3), 4.0, DEV)
    m.add_bounds([view], [J.to(DEV)])
    assert m.begin(blend=1e6) == (1, 1)
    m.splat([view], [J.to(DEV)], 0)
    m.accumulate([view], [J.to(DEV)], 0)
    with pytest.raises(ValueError, match='1048576 samples') as e:
        m.normalize()
    assert '--mosaic-gsd' in str(e.value)
    assert int(m.acc[0, 7]) == 1 << 20
    view, J, rgb = one_cell_plane(1023, 1024, 22)
    n = 1023 * 1024
    m = engine.mosaic_of([view], [J.to(DEV)], torch.eye(3), 4.0, blend=1e6)
    assert (m.Hm, m.Wm) == (1, 1)
    got = {k: v.cpu() for k, v in m.result().items()}
    Jq = np.rint(J.numpy().reshape(-1, 3) * np.float32(1048576)).astype(np.int64).sum(axis=0)
    R = rgb.numpy().reshape(-1, 3).astype(np.int64).sum(axis=0)
    assert m.acc.cpu().tolist() == [[int(4096 * Jq[0]), int(4096 * Jq[1]), int(4096 * Jq[2]), int(4096 * R[0]), int(4096 * R[1]), int(4096 * R[2]), 4096 * n, n]]
    assert got['samples'].tolist() == [[n]] and got['weight'].tolist() == [[float(n)]]
    assert np.array_equal(got['J_blend'].numpy()[0, 0], ((Jq.astype(np.float64) / np.float64(n)) * 2.0 ** -20).astype(np.float32))
    assert got['raw_blend'].tolist() == [[[int((2 * r + n) // (2 * n)) for r in R]]]


def test_the_two_entries_through_the_c_abi():
    """The tie case of test_gpu_mosaic.py, one cell: the four tied centre pixels all have the full weight.  Bad arguments return
    an error and leave the accumulator untouched."""
    J = torch.rand((8, 16, 3), generator=torch.Generator().manual_seed(9))
    host, dev = tie_case(J)
    H = 0.03125
    want = bref.blend([host], [J], torch.eye(3), 4.0, H)
    assert int((want['wq'] == 4096).sum()) == 4 and int(want['base']['ties'][0, 0]) == 4
    assert 4 < int(want['samples'][0, 0]) < 128 and want['wq'][[55, 56, 71, 72]].tolist() == [4096] * 4
    lib = _lib.load()
    Jd = J.to(DEV)
    im = _lib.MosaicImage()
    im.depth, im.rgb, im.J, im.H, im.W = dev.depth.data_ptr(), dev.rgb.data_ptr(), Jd.data_ptr(), 8, 16
    im.Kinv = (C.c_float * 9)(*TIE_K.inverse().flatten().tolist())
    im.R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    im.t = (C.c_float * 3)(0, 0, 0)
    arr = (_lib.MosaicImage * 1)(im)
    table = torch.empty(lib.sucre_mosaic_table_bytes(1), dtype=torch.uint8, device=DEV)
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    lo_s, lo_t = want['base']['bounds'][:2]
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 4.0, lo_s, lo_t, 1, 1
    key = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    acc = torch.zeros((1, 8), dtype=torch.int64, device=DEV)
    out = {'J_blend': torch.full((1, 1, 3), float('nan'), device=DEV), 'raw_blend': torch.zeros((1, 1, 3), dtype=torch.uint8, device=DEV),
           'weight': torch.zeros((1, 1), device=DEV), 'samples': torch.zeros((1, 1), dtype=torch.int32, device=DEV)}
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp, kp, ap = C.c_void_p(table.data_ptr()), C.c_void_p(key.data_ptr()), C.c_void_p(acc.data_ptr())
    inv_h = C.c_float(float(np.float32(1) / np.float32(H)))
    with torch.cuda.device(DEV):
        _lib.check(lib.sucre_mosaic_splat(tp, 1, arr, 0, C.byref(g), kp, 0, sp))
        for bad in (0.0, float('nan')):
            assert lib.sucre_mosaic_accumulate(tp, 1, arr, 0, C.byref(g), kp, C.c_float(bad), ap, 0, sp) == -1 and b'inv_h' in lib.sucre_last_error()
        assert lib.sucre_mosaic_accumulate(tp, 1, arr, 0, C.byref(g), kp, inv_h, None, 0, sp) == -1 and b'acc_dev' in lib.sucre_last_error()
        assert lib.sucre_mosaic_normalize(C.byref(g), None, *[C.c_void_p(out[k].data_ptr()) for k in BLENDED], sp) == -1
        torch.cuda.synchronize()
        assert not bool(acc.any()) and bool(torch.isnan(out['J_blend']).all())
        for flags in (0, _lib.MOSAIC_PLAIN_ATOMIC):
            acc.zero_()
            _lib.check(lib.sucre_mosaic_accumulate(tp, 1, arr, 0, C.byref(g), kp, inv_h, ap, flags, sp))
            _lib.check(lib.sucre_mosaic_normalize(C.byref(g), ap, *[C.c_void_p(out[k].data_ptr()) for k in BLENDED], sp))
            torch.cuda.synchronize()
            assert same_bits(acc, want['acc']), flags
            for k in BLENDED:
                assert same_bits(out[k], want[k]), (flags, k)


def test_methods_refuse_what_they_cannot_do():
    views, Js, axes, gsd = views_of('survey')
    m = engine.Mosaic(axes, gsd, DEV)
    with pytest.raises(ValueError, match='begin'):
        m.accumulate(views, Js, 0)
    for bad in (0.0, 9e-7, 1.1e6, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='blend depth H'):
            m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=bad)
        assert m.key is None and m.acc is None    # refused before anything is allocated
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='blend'):
        m.accumulate(views, Js, 0)
    with pytest.raises(ValueError, match='blend'):
        m.normalize()
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5)
    assert m.acc.dtype == torch.int64 and tuple(m.acc.shape) == (m.Hm * m.Wm, 8) and not bool(m.acc.any())
    assert float(m.inv_h) == 2.0 and isinstance(m.inv_h, np.float32)
    with pytest.raises(_lib.SucreError, match='ordinals'):
        m.accumulate(views, Js, engine.MAX_VIEWS - 2)
    assert not bool(m.acc.any())    # nothing ran


# ---- the command line: restore a survey with --apply-water, then make its mosaic with and without a blend -------------------------
CLI_BLEND = 0.5    # metres; within [gsd, 100 gsd] of this survey (gsd about 0.08 m) -- see test_the_blend_softens_the_seams


@pytest.fixture(scope='module')
def blend_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_blend_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    torch.save({'lo': torch.tensor([0.1, 0.15, 0.2]), 'hi': torch.tensor([0.8, 0.85, 0.9])}, root / 'stretch.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored, best, blended, fixed = root / 'restored', root / 'mosaic', root / 'mosaic_blend', root / 'mosaic_blend_fixed'
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        printed_best, printed = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(printed_best):
            sucre.main(base + ['--output-dir', str(best), '--mosaic', str(restored)])
        with contextlib.redirect_stdout(printed):
            sucre.main(base + ['--output-dir', str(blended), '--mosaic', str(restored), '--mosaic-blend', str(CLI_BLEND)])
        sucre.main(base + ['--output-dir', str(fixed), '--mosaic', str(restored), '--mosaic-blend', str(CLI_BLEND), '--stretch-from', str(root / 'stretch.pt')])
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, scene, restored, best, blended, fixed, printed_best.getvalue(), printed.getvalue()


def test_cli_writes_six_files_and_leaves_the_best_view_ones_alone(blend_run):
    """The three best-view pictures byte for byte; mosaic.pt gains keys, so there every key of the run without a blend, bit for bit."""
    from PIL import Image as PILImage
    from sucre_amd import sfm
    root, scene, restored, best, blended, fixed, printed_best, printed = blend_run
    names = [v.name for v in scene.views]
    old = ['mosaic.png', 'mosaic.pt', 'mosaic_raw.png', 'mosaic_source.png']
    assert sorted(p.name for p in best.iterdir()) == old
    assert sorted(p.name for p in blended.iterdir()) == sorted(old + ['mosaic_blend.png', 'mosaic_blend_raw.png'])
    for name in ('mosaic.png', 'mosaic_raw.png', 'mosaic_source.png'):
        assert (best / name).read_bytes() == (blended / name).read_bytes(), name
    was, got = torch.load(best / 'mosaic.pt'), torch.load(blended / 'mosaic.pt')
    assert set(got) - set(was) == set(BLENDED) | {'blend'} and not set(was) - set(got)
    for k, v in was.items():
        assert same_bits(v, got[k]) if torch.is_tensor(v) else v == got[k], k
    assert got['blend'] == float(np.float32(CLI_BLEND))
    # the lines: those of the run without a blend, then one more, which matches the tensors
    lines_best, lines = printed_best.splitlines(), printed.splitlines()
    assert lines[:len(lines_best)] == lines_best and len(lines) == len(lines_best) + 1
    samples = got['samples'].long()
    n_filled = int((got['source'] >= 0).sum())
    total, most, several = int(samples.sum()), int(samples.max()), int((samples > 1).sum())
    assert lines[-1] == (f'mosaic blend of depth {got["blend"]:.6g} m: {total} samples, {total / n_filled:.2f} per filled cell on average, '
                         f'{most} at most; {100.0 * several / n_filled:.1f} % of the filled cells blend more than one sample')
    assert total > 10 * n_filled
    # the same blend from sucre.mosaic() called directly, and from the engine on the restored files
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    with contextlib.redirect_stdout(io.StringIO()):
        direct = sucre.mosaic(names, model, restored, root / 'direct', blend=CLI_BLEND)
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    m = engine.mosaic_of(views, Js, axes, gsd, blend=CLI_BLEND)
    for k in BEST + BLENDED:
        assert same_bits(got[k], direct[k]) and same_bits(got[k], m.result()[k]), k
    assert direct['blend'] == got['blend']
    # the pictures: J_blend through the function that makes mosaic.png, the raw blend as it is
    assert np.array_equal(np.asarray(PILImage.open(blended / 'mosaic_blend_raw.png')), got['raw_blend'].numpy())
    sucre_like = SimpleNamespace(J=got['J_blend'], stretch=None)
    assert np.array_equal(np.asarray(PILImage.open(blended / 'mosaic_blend.png')), np.asarray(sucre.SUCRe.plot_J(sucre_like)))
    # --stretch-from goes to both pictures of J
    fixed_got = torch.load(fixed / 'mosaic.pt')
    lo, hi = sucre.read_stretch_file(root / 'stretch.pt')
    assert np.array_equal(np.asarray(PILImage.open(fixed / 'mosaic_blend.png')), sucre.stretch_picture(fixed_got['J_blend'].numpy(), lo, hi))
    assert np.array_equal(np.asarray(PILImage.open(fixed / 'mosaic.png')), sucre.stretch_picture(fixed_got['J'].numpy(), lo, hi))
    assert same_bits(fixed_got['J_blend'], got['J_blend'])


def seam_steps(J, source):
    """Mean |difference of J| over horizontally adjacent filled cells won by different images (float64)."""
    J, source = J.double().numpy(), source.numpy()
    seam = (source[:, :-1] >= 0) & (source[:, 1:] >= 0) & (source[:, :-1] != source[:, 1:])
    return float(np.abs(J[:, 1:][seam] - J[:, :-1][seam]).mean()), int(seam.sum())


def test_the_blend_softens_the_seams(blend_run):
    """What it is for: across the seams of the best-view mosaic -- neighbouring cells won by different images -- the blended colours
    step less than the best-view ones.  For the CPU reference on this survey (123 seam pairs, best view 0.037448): blended 0.036555,
    0.036873, 0.036572, 0.036498, 0.036476 at H = 1, 3, 10, 30, 100 gsd and 0.036657 at the 0.5 m used here."""
    root, scene, restored, best, blended, fixed, _, _ = blend_run
    got = torch.load(blended / 'mosaic.pt')
    gsd = got['gsd']
    assert gsd <= CLI_BLEND <= 100 * gsd
    best_step, n = seam_steps(got['J'], got['source'])
    blend_step, _ = seam_steps(got['J_blend'], got['source'])
    print(f'{n} seam pairs: mean |dJ| {best_step:.6f} best view, {blend_step:.6f} blended (H = {CLI_BLEND} m, gsd {gsd:.4f} m)')
    assert n > 100
    assert blend_step < best_step
