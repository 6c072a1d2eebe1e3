"""GPU tests of the seabed mosaic (sucre_mosaic_*, engine.Mosaic, sucre.mosaic, --mosaic).

The yardstick is tests/mosaic_ref.py, a CPU float32 restatement that shares no code with the engine (geometry by the
reference's formulas, the winner by a lexicographic sort).  Everything is compared EXACTLY: the bounds, the grid size and the
bytes of all five outputs.  test_mosaic_host.py checks that oracle on mosaics computed by hand.
"""
import contextlib
import ctypes as C
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_ref as ref
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_CASES = {}


def restored_like(view, seed, device=DEV):
    """Random float32 in (0, 1) with NaN patches: two rectangles with all channels NaN and about 2 % of the pixels with a NaN in one.
    (``device``: where the image goes; test_mosaic_variants_host.py makes the same images on the CPU.)"""
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
    return J.to(device)


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
            scene = synth.make_scene(333, 207, 1, seed=5)   # the size of baseline_odd's fixture: no multiple of anything
        else:
            scene = synth.make_survey(24, 16, 11, 3, seed=2)   # 33 views: one more than a launch table holds
        views = engine.device_views_from_scene(scene, DEV)
        Js = [restored_like(v, 300 + k) for k, v in enumerate(views)]
        axes = sucre.mosaic_axes(views)
        gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
        _CASES[key] = (views, Js, axes, gsd)
    return _CASES[key]


def oracle(key, gsd_factor=1.0, bounds=None):
    ck = (key, 'oracle', gsd_factor, bounds)
    if ck not in _CASES:
        views, Js, axes, gsd = views_of(key)
        _CASES[ck] = ref.mosaic([host_view(v) for v in views], [J.cpu() for J in Js], axes, np.float32(gsd * np.float32(gsd_factor)), bounds=bounds)
    return _CASES[ck]


def check_against_oracle(m, want, what):
    got = m.result()
    filled = int((want['source'] >= 0).sum())
    print(f'{what}: {want["Wm"]} x {want["Hm"]} cells, {filled} filled, {int(want["ties"].max())} pixels share the winning range bits at most')
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']), what
    for k in ('source', 'pixel', 'range', 'J', 'raw'):
        assert same_bits(got[k], want[k]), (what, k, int((got[k].cpu() != want[k]).sum()))


def test_survey_on_a_coarse_grid_equals_the_oracle():
    """Six views, about 17 pixels per cell: dense collisions at a tiny size."""
    views, Js, axes, gsd = views_of('survey')
    assert sum(int((v.depth > 0).sum()) for v in views) == 36475
    want = oracle('survey')
    m = engine.mosaic_of(views, Js, axes, gsd)
    assert m.bounds() == want['bounds']
    assert 50 <= want['Wm'] <= 75 and 28 <= want['Hm'] <= 45
    check_against_oracle(m, want, 'survey, default gsd')
    assert int((want['source'] >= 0).sum()) > 0.9 * want['Hm'] * want['Wm']
    assert len(set(want['source'].flatten().tolist()) - {-1}) == 6


def test_survey_on_a_fine_grid_equals_the_oracle():
    """A quarter of the default gsd: few collisions, many empty cells."""
    views, Js, axes, gsd = views_of('survey')
    want = oracle('survey', 0.25)
    m = engine.mosaic_of(views, Js, axes, np.float32(gsd * np.float32(0.25)))
    assert m.bounds() == want['bounds']
    check_against_oracle(m, want, 'survey, gsd / 4')
    assert int((want['source'] < 0).sum()) > 0.3 * want['Hm'] * want['Wm']


def test_deep_scene_does_not_depend_on_the_request_order():
    """Ranges from 0.7 m to 8 m.  The same images in another order: the same range and colour in every cell, the ordinals permuted."""
    views, Js, axes, gsd = views_of('deep')
    want = oracle('deep')
    a = engine.mosaic_of(views, Js, axes, gsd)
    check_against_oracle(a, want, 'deep scene')
    perm = [4, 0, 6, 2, 5, 1, 3]
    b = engine.mosaic_of([views[i] for i in perm], [Js[i] for i in perm], axes, gsd)
    ra, rb = a.result(), b.result()
    assert b.bounds() == a.bounds() and (b.Hm, b.Wm) == (a.Hm, a.Wm)
    assert same_bits(ra['range'], rb['range']) and same_bits(ra['J'], rb['J']) and same_bits(ra['raw'], rb['raw']) and same_bits(ra['pixel'], rb['pixel'])
    back = torch.tensor(perm + [-1], dtype=torch.int32, device=DEV)    # ordinal in b -> ordinal in a; -1 stays -1
    assert torch.equal(back[rb['source'].long()], ra['source'])
    lo, hi = float(np.nanmin(want['range'].numpy())), float(np.nanmax(want['range'].numpy()))
    print(f'deep scene: winning ranges {lo:.3f} .. {hi:.3f} m')


def test_the_same_view_twice_goes_to_the_earlier_ordinal():
    views, Js, axes, gsd = views_of('survey')
    m = engine.mosaic_of([views[2], views[2]], [Js[2], Js[2]], axes, gsd)
    source = m.result()['source']
    assert int((source >= 0).sum()) > 100 and bool((source[source >= 0] == 0).all())
    alone = engine.mosaic_of([views[2]], [Js[2]], axes, gsd)
    assert all(same_bits(m.result()[k], alone.result()[k]) for k in ('source', 'pixel', 'range', 'J', 'raw'))


def abi_mosaic(images, axes, gsd, bounds, plain=False):
    """The four phases through the C ABI, as a caller without the Python class would run them; returns the five outputs and the bounds."""
    lib = _lib.load()
    n = len(images)
    arr = (_lib.MosaicImage * n)(*images)
    table = torch.empty(lib.sucre_mosaic_table_bytes(n), dtype=torch.uint8, device=DEV)
    words = torch.tensor([-1, -1, 0, 0], dtype=torch.int32, device=DEV)
    axes_c = (C.c_float * 9)(*axes)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp = C.c_void_p(table.data_ptr())
    with torch.cuda.device(DEV):
        _lib.check(lib.sucre_mosaic_bounds(tp, n, arr, axes_c, C.c_void_p(words.data_ptr()), sp))
        k = words.cpu().numpy().view(np.uint32)
        found = tuple(np.where(k & 0x80000000, k & 0x7fffffff, ~k).astype(np.uint32).view(np.float32).tolist())
        lo_s, lo_t, hi_s, hi_t = bounds if bounds is not None else found
        g = _lib.MosaicGrid()
        g.axes, g.gsd, g.lo_s, g.lo_t = axes_c, gsd, lo_s, lo_t
        g.Wm, g.Hm = engine.mosaic_cells(lo_s, hi_s, gsd), engine.mosaic_cells(lo_t, hi_t, gsd)
        key = torch.full((g.Hm * g.Wm,), -1, dtype=torch.int64, device=DEV)
        pix = torch.full((g.Hm * g.Wm,), -1, dtype=torch.int32, device=DEV)
        out = {'J': torch.full((g.Hm, g.Wm, 3), float('nan'), device=DEV), 'raw': torch.zeros((g.Hm, g.Wm, 3), dtype=torch.uint8, device=DEV),
               'source': torch.full((g.Hm, g.Wm), -1, dtype=torch.int32, device=DEV), 'pixel': torch.full((g.Hm, g.Wm), -1, dtype=torch.int32, device=DEV),
               'range': torch.full((g.Hm, g.Wm), float('nan'), device=DEV)}
        kp, pp = C.c_void_p(key.data_ptr()), C.c_void_p(pix.data_ptr())
        _lib.check(lib.sucre_mosaic_splat(tp, n, arr, 0, C.byref(g), kp, _lib.MOSAIC_PLAIN_ATOMIC if plain else 0, sp))
        _lib.check(lib.sucre_mosaic_resolve(tp, n, arr, 0, C.byref(g), kp, pp, sp))
        _lib.check(lib.sucre_mosaic_gather(tp, n, arr, 0, C.byref(g), kp, pp, *[C.c_void_p(out[k].data_ptr()) for k in ('J', 'raw', 'source', 'pixel', 'range')], sp))
        torch.cuda.synchronize()
    return out, found, key


def test_pixel_tie_goes_to_the_lower_index_through_the_c_abi():
    """One 16x8 image, dyadic intrinsics, identity pose, depth 1, one cell: the four centre pixels 55, 56, 71, 72 have bit-equal
    ranges (checked here, on the CPU, through the oracle) and the lowest index wins."""
    K = torch.tensor([[16.0, 0.0, 8.0], [0.0, 16.0, 4.0], [0.0, 0.0, 1.0]])
    depth = torch.ones(8, 16)
    rgb = (torch.arange(8 * 16 * 3) % 251).to(torch.uint8).reshape(8, 16, 3)
    J = torch.rand((8, 16, 3), generator=torch.Generator().manual_seed(9))
    view = SimpleNamespace(depth=depth, rgb=rgb, K=K, R=torch.eye(3), t=torch.zeros(3, 1))
    want = ref.mosaic([view], [J], torch.eye(3), 4.0)
    p, z, _, _ = ref.pixels(view, J, torch.eye(3))
    zb = z.view(torch.int32)
    assert len({int(zb[i]) for i in (55, 56, 71, 72)}) == 1 and int(want['ties'][0, 0]) == 4 and (want['Hm'], want['Wm']) == (1, 1)
    assert want['pixel'].tolist() == [[55]]
    d, c, Jd = depth.to(DEV), rgb.to(DEV), J.to(DEV)
    im = _lib.MosaicImage()
    im.depth, im.rgb, im.J, im.H, im.W = d.data_ptr(), c.data_ptr(), Jd.data_ptr(), 8, 16
    im.Kinv = (C.c_float * 9)(*K.inverse().flatten().tolist())
    im.R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    im.t = (C.c_float * 3)(0, 0, 0)
    for plain in (False, True):
        out, found, key = abi_mosaic([im], [1, 0, 0, 0, 1, 0, 0, 0, 1], 4.0, None, plain=plain)
        assert found == want['bounds']
        assert out['pixel'].cpu().tolist() == [[55]] and out['source'].cpu().tolist() == [[0]]
        assert int(key.cpu()[0]) == int(zb[55]) << 32    # bits(z) << 32 | ordinal 0: below 2^63, a valid int64
        for k in ('source', 'pixel', 'range', 'J', 'raw'):
            assert same_bits(out[k], want[k]), k


def test_range_is_the_minimum_over_the_single_view_mosaics():
    views, Js, axes, gsd = views_of('survey')
    m = engine.mosaic_of(views, Js, axes, gsd)
    bounds = m.bounds()
    ranges = []
    for v, J in zip(views, Js):
        one = engine.mosaic_of([v], [J], axes, gsd, bounds=bounds)
        assert (one.Hm, one.Wm) == (m.Hm, m.Wm)
        ranges.append(one.result()['range'])
    stacked = torch.stack(ranges)
    lowest = torch.where(torch.isnan(stacked), torch.full_like(stacked, float('inf')), stacked).min(dim=0).values
    lowest = torch.where(torch.isinf(lowest), torch.full_like(lowest, float('nan')), lowest)
    assert same_bits(lowest, m.result()['range'])


def test_an_odd_sized_image_equals_the_oracle():
    views, Js, axes, gsd = views_of('odd')
    assert tuple(views[0].depth.shape) == (207, 333)
    want = oracle('odd')
    m = engine.mosaic_of(views, Js, axes, gsd)
    assert m.bounds() == want['bounds']
    check_against_oracle(m, want, '333 x 207, two views')


def test_thirty_three_views_in_one_call_equal_the_oracle():
    views, Js, axes, gsd = views_of('many')
    assert len(views) == 33
    gsd = np.float32(gsd * np.float32(0.25))    # fine enough for every one of the 33 views to win cells
    want = oracle('many', 0.25)
    m = engine.mosaic_of(views, Js, axes, gsd, batch=33)    # one call per phase: two launches each
    assert m.bounds() == want['bounds']
    check_against_oracle(m, want, '33 views in one call')
    assert set(want['source'].flatten().tolist()) == set(range(-1, 33))
    split = engine.mosaic_of(views, Js, axes, gsd, batch=5)   # the same in calls of five: the ordinals come from first_ordinal
    assert all(same_bits(m.result()[k], split.result()[k]) for k in ('source', 'pixel', 'range', 'J', 'raw'))


def test_two_runs_and_both_splat_variants_give_the_same_bytes():
    views, Js, axes, gsd = views_of('survey')
    a = engine.mosaic_of(views, Js, axes, gsd)
    b = engine.mosaic_of(views, Js, axes, gsd)
    c = engine.mosaic_of(views, Js, axes, gsd, plain_atomic=True)
    for other in (b, c):
        assert other.bounds() == a.bounds() and same_bits(other.key, a.key) and same_bits(other.pix, a.pix)
        assert all(same_bits(a.result()[k], other.result()[k]) for k in ('source', 'pixel', 'range', 'J', 'raw'))


def test_caller_given_bounds_drop_what_lies_outside_as_the_oracle_does():
    views, Js, axes, gsd = views_of('survey')
    lo_s, lo_t, hi_s, hi_t = oracle('survey')['bounds']
    half = (lo_s, lo_t, float(np.float32(0.5 * (lo_s + hi_s))), hi_t)
    want = oracle('survey', 1.0, half)
    m = engine.mosaic_of(views, Js, axes, gsd, bounds=half)
    check_against_oracle(m, want, 'survey cut in half')
    full = oracle('survey')
    assert want['Wm'] < 0.6 * full['Wm'] and want['Hm'] == full['Hm']
    assert same_bits(want['pixel'][:, :want['Wm'] - 1], full['pixel'][:, :want['Wm'] - 1])


def test_bad_arguments_are_refused_without_a_launch(monkeypatch):
    """Argument checks only: nothing here reaches the device."""
    views, Js, axes, gsd = views_of('survey')
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='gsd'):
            engine.Mosaic(axes, bad, DEV)
    with pytest.raises(ValueError, match='axes'):
        engine.Mosaic(torch.zeros(2, 3), gsd, DEV)
    m = engine.Mosaic(axes, gsd, DEV)
    with pytest.raises(ValueError, match='begin'):
        m.splat(views, Js, 0)
    with pytest.raises(ValueError, match='1..4096'):
        m.add_bounds([views[0]] * (engine.MAX_VIEWS + 1), [Js[0]] * (engine.MAX_VIEWS + 1))
    with pytest.raises(ValueError, match='restored images'):
        m.add_bounds(views, Js[:2])
    with pytest.raises(ValueError, match='float32'):
        m.add_bounds(views[:1], [Js[0][:, :5]])
    with pytest.raises(ValueError, match='uint8'):
        m.add_bounds([views[0].as_float_colour()], Js[:1])
    with pytest.raises(ValueError, match='no pixel takes part'):
        m.begin()
    monkeypatch.setenv('SUCRE_MOSAIC_MAX_CELLS', '1000')
    with pytest.raises(ValueError, match='--mosaic-gsd') as e:
        m.begin(bounds=(0.0, 0.0, 100.0, 100.0))
    assert 'SUCRE_MOSAIC_MAX_CELLS' in str(e.value) and m.key is None
    monkeypatch.delenv('SUCRE_MOSAIC_MAX_CELLS')
    with pytest.raises(ValueError, match='--mosaic-gsd'):
        engine.Mosaic(axes, 1e-6, DEV).begin(bounds=(0.0, 0.0, 100.0, 100.0))    # 10^16 cells: refused before anything is allocated
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0))
    with pytest.raises(_lib.SucreError, match='ordinals'):
        m.splat(views, Js, engine.MAX_VIEWS - 2)
    assert bool((m.key == -1).all())    # nothing ran


# ---- the command line: restore a survey with --apply-water, then make its mosaic ------------------------------------------------
@pytest.fixture(scope='module')
def mosaic_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    torch.save({'lo': torch.tensor([0.1, 0.15, 0.2]), 'hi': torch.tensor([0.8, 0.85, 0.9])}, root / 'stretch.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored, out, fixed = root / 'restored', root / 'mosaic', root / 'mosaic_fixed'
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            sucre.main(base + ['--output-dir', str(out), '--mosaic', str(restored), '--num-iter', '3'])
        sucre.main(base + ['--output-dir', str(fixed), '--mosaic', str(restored), '--mosaic-gsd', '0.1', '--stretch-from', str(root / 'stretch.pt')])
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, scene, restored, out, fixed, printed.getvalue()


def test_cli_writes_the_four_files_and_the_engines_bits(mosaic_run):
    from PIL import Image as PILImage
    from sucre_amd import sfm
    root, scene, restored, out, fixed, printed = mosaic_run
    names = [v.name for v in scene.views]
    assert sorted(p.name for p in out.iterdir()) == ['mosaic.png', 'mosaic.pt', 'mosaic_raw.png', 'mosaic_source.png']
    assert '--mosaic' in printed and 'ignored' in printed and 'Solve least squares' not in printed and 'ground sample distance' in printed
    got = torch.load(out / 'mosaic.pt')
    assert all(k in got for k in ('J', 'raw', 'source', 'pixel', 'range', 'axes', 'gsd', 'lo', 'images', 'n_filled', 'per_image'))
    Hm, Wm = got['source'].shape
    n_filled = int((got['source'] >= 0).sum())
    assert f'mosaic of 6 images: {Wm} x {Hm} cells of {got["gsd"]:.6g} m, {n_filled} filled (' in printed and f'{Hm * Wm - n_filled} empty; largest share img_' in printed
    assert got['images'] == names and got['n_filled'] == n_filled and int(got['per_image'].sum()) == n_filled
    assert torch.equal(got['per_image'], torch.bincount(got['source'][got['source'] >= 0].long(), minlength=6))
    # the same mosaic from sucre.mosaic() called directly, and from the engine on the restored files
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    with contextlib.redirect_stdout(io.StringIO()):
        direct = sucre.mosaic(names, model, restored, root / 'direct')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    m = engine.mosaic_of(views, Js, axes, gsd)
    assert got['gsd'] == float(gsd) and torch.equal(got['axes'], axes) and tuple(got['lo'].tolist()) == m.bounds()[:2]
    for k in ('J', 'raw', 'source', 'pixel', 'range'):
        assert same_bits(got[k], direct[k]) and same_bits(got[k], m.result()[k]), k
    # restored colours of a survey restored with its true water: the mosaic holds them, and the pictures show it
    assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic_raw.png')), got['raw'].numpy())
    assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic_source.png')), sucre.mosaic_source_picture(got['source'].numpy()))
    sucre_like = SimpleNamespace(J=got['J'], stretch=None)
    assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic.png')), np.asarray(sucre.SUCRe.plot_J(sucre_like)))


def test_cli_with_a_fixed_stretch_and_a_given_gsd(mosaic_run):
    from PIL import Image as PILImage
    root, scene, restored, out, fixed, _ = mosaic_run
    got = torch.load(fixed / 'mosaic.pt')
    assert got['gsd'] == float(np.float32(0.1)) and got['source'].shape != torch.load(out / 'mosaic.pt')['source'].shape
    lo, hi = sucre.read_stretch_file(root / 'stretch.pt')
    assert np.array_equal(np.asarray(PILImage.open(fixed / 'mosaic.png')), sucre.stretch_picture(got['J'].numpy(), lo, hi))


def test_restored_images_that_do_not_fit_the_cache_are_read_again_per_phase_with_the_same_bits(mosaic_run, monkeypatch):
    """A cache budget of one and a half images: every phase reads every file again (the LRU cache drops what it just held)."""
    from sucre_amd import sfm
    root, scene, restored, out, fixed, _ = mosaic_run
    names = [v.name for v in scene.views]
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    monkeypatch.setenv('SUCRE_CONSISTENCY_CACHE_GB', str(1.5 * 96 * 64 * 12 / 2 ** 30))
    reads = []
    real = sucre._read_restored
    monkeypatch.setattr(sucre, '_read_restored', lambda path, image, **kw: (reads.append((path.name, kw.get('lazy', False))), real(path, image, **kw))[1])
    with contextlib.redirect_stdout(io.StringIO()):
        small = sucre.mosaic(names, model, restored, root / 'small_cache')
    full_reads = [n for n, lazy in reads if not lazy]
    assert len(full_reads) > 2 * len(names)    # bounds, splat, resolve, gather: more than one pass over the files
    got = torch.load(out / 'mosaic.pt')
    for k in ('J', 'raw', 'source', 'pixel', 'range'):
        assert same_bits(got[k], small[k]), k
