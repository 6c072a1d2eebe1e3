"""GPU tests of the feathered mosaic blend (sucre_mosaic_feather / _accumulate_feathered, engine.Mosaic, sucre.mosaic,
--mosaic-feather).

The yardstick is tests/mosaic_feather_ref.py, a numpy restatement that shares no code with the engine (a brute-force distance
map, float32 weights one operation per line, int64 sums); test_mosaic_feather_host.py checks it against the separable form.
Every comparison is EXACT: the map is integer, the sums are integers, so no schedule, order or split may move a bit.
"""
import contextlib
import ctypes as C
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_feather_ref as fref
import mosaic_fill_ref as fill_ref
import mosaic_ref as ref
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
BLENDED = ('J_blend', 'raw_blend', 'weight', 'samples')
BEST = ('source', 'pixel', 'range', 'J', 'raw')
_CACHE = {}


def host_view(v):
    """What the restatement reads of a DeviceView."""
    return SimpleNamespace(depth=v.depth.cpu(), rgb=v.rgb.cpu(), K=v.K, R=v.R, t=v.t, Kinv=v.Kinv)


def same_bits(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))

# ---- a. the map ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (67, 45), (5, 300), (300, 5), (523, 3)]     # W x H; 300 and 523 columns cross a 256-lane segment
MASKS = ['all', 'none', 'middle', 'corners', 'column and row', 'random holes', 'NaN in one channel', 'bad depths']
MAP_WIDTHS = [1, 2, 7, 64, 1024]
PLAIN_K = torch.tensor([[100.0, 0.0, 10.0], [0.0, 100.0, 10.0], [0.0, 0.0, 1.0]])


def masked_image(W, H, kind, seed):
    """(depth (H,W), J (H,W,3)) float32 CPU tensors with the non-members of ``kind``."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand((H, W), generator=g) + 0.5
    J = torch.rand((H, W, 3), generator=g)
    if kind == 'none':
        depth[:] = 0
    elif kind == 'middle':
        J[H // 2, W // 2] = NAN
    elif kind == 'corners':
        for v, u in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            depth[v, u] = 0
    elif kind == 'column and row':
        J[:, W // 2] = NAN
        depth[H // 2, :] = 0
    elif kind == 'random holes':
        depth[torch.rand((H, W), generator=g) < 0.3] = 0
    elif kind == 'NaN in one channel':
        hit = torch.rand((H, W), generator=g) < 0.2
        ch = torch.randint(0, 3, (H, W), generator=g)
        vv, uu = torch.nonzero(hit, as_tuple=True)
        J[vv, uu, ch[vv, uu]] = NAN
    elif kind == 'bad depths':
        r = torch.rand((H, W), generator=g)
        depth[r < 0.1] = 0
        depth[(r >= 0.1) & (r < 0.2)] = -1.5
        depth[(r >= 0.2) & (r < 0.3)] = NAN
    else:
        assert kind == 'all'
    return depth, J


def device_view(depth, name='masked', K=PLAIN_K, Kinv=None):
    H, W = depth.shape
    return engine.DeviceView(depth=depth.to(DEV).contiguous(), rgb=torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), K=K,
                             R=torch.eye(3), t=torch.zeros(3, 1), name=name, Kinv=Kinv)


def map_cases():
    """Every size with every mask, 40 images: (views, Js, per image the uncapped brute-force D2) -- made once, never changed."""
    if 'maps' not in _CACHE:
        views, Js, near = [], [], []
        for i, (W, H) in enumerate(SIZES):
            for k, kind in enumerate(MASKS):
                depth, J = masked_image(W, H, kind, 1000 + 10 * i + k)
                member = fref.members(depth.numpy(), J.numpy())
                if kind == 'all':
                    assert member.all()
                elif kind == 'none':
                    assert not member.any()
                views.append(device_view(depth, f'{W}x{H} {kind}'))
                Js.append(J.to(DEV))
                near.append(fref.nearest2(member))
        _CACHE['maps'] = (views, Js, near)
    return _CACHE['maps']


@pytest.mark.parametrize('F', MAP_WIDTHS)
def test_the_map_of_every_size_and_mask_in_one_call_equals_the_brute_force(F):
    """40 images of five sizes in one call: two launches, the second one's words behind the first one's."""
    views, Js, near = map_cases()
    assert len(views) == 40
    maps = engine.Mosaic(torch.eye(3), 1.0, DEV).feather_map(views, Js, F)
    assert len(maps) == 40
    for v, got, D2 in zip(views, maps, near):
        assert got.dtype == torch.int32 and tuple(got.shape) == tuple(v.depth.shape)
        want = np.minimum(D2, F * F)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (v.name, F, int((got.cpu().numpy() != want).sum()))


def test_the_map_of_33_images_and_of_one_image_at_a_time():
    views, Js, near = map_cases()
    m = engine.Mosaic(torch.eye(3), 1.0, DEV)
    order = list(range(7, 40))      # 33 images: one more than a launch holds
    maps = m.feather_map([views[i] for i in order], [Js[i] for i in order], 7)
    for i, got in zip(order, maps):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), np.minimum(near[i], 49)), views[i].name
    for i in (0, 9, 19, 29, 37):
        alone = m.feather_map([views[i]], [Js[i]], 1024)[0]
        assert np.array_equal(alone.cpu().numpy().astype(np.int64), np.minimum(near[i], 1024 * 1024)), views[i].name


def test_the_entries_check_their_arguments_before_any_launch():
    views, Js, near = map_cases()
    m = engine.Mosaic(torch.eye(3), 1.0, DEV)
    arr, n, table, keep = m._images(views[8:10], Js[8:10])
    lib = _lib.load()
    n_bytes = lib.sucre_mosaic_feather_bytes(n, arr)
    px = sum(-(-(e.H * e.W) // 256) * 256 for e in arr)
    assert n_bytes == 6 * px
    assert lib.sucre_mosaic_feather_bytes(0, arr) == 0 and b'n_images' in lib.sucre_last_error()
    assert lib.sucre_mosaic_feather_bytes(engine.MAX_VIEWS + 1, arr) == 0
    buf = torch.full((n_bytes,), 0x5a, dtype=torch.uint8, device=DEV)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp, bp = C.c_void_p(table.data_ptr()), C.c_void_p(buf.data_ptr())
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 1.0, 0.0, 0.0, 1, 1
    key = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    acc = torch.zeros((1, 8), dtype=torch.int64, device=DEV)
    kp, ap = C.c_void_p(key.data_ptr()), C.c_void_p(acc.data_ptr())
    with torch.cuda.device(DEV):
        for bad in (0, 1025, -1):
            assert lib.sucre_mosaic_feather(tp, n, arr, bad, bp, sp) == -1 and b'feather_px' in lib.sucre_last_error()
            assert lib.sucre_mosaic_accumulate_feathered(tp, n, arr, 0, C.byref(g), kp, C.c_float(2.0), bad, bp, ap, 0, sp) == -1
            assert b'feather_px' in lib.sucre_last_error()
        assert lib.sucre_mosaic_feather(tp, n, arr, 8, None, sp) == -1 and b'feather_dev' in lib.sucre_last_error()
        assert lib.sucre_mosaic_accumulate_feathered(tp, n, arr, 0, C.byref(g), kp, C.c_float(2.0), 8, None, ap, 0, sp) == -1
        assert b'feather_dev' in lib.sucre_last_error()
        assert lib.sucre_mosaic_feather(tp, 0, arr, 8, bp, sp) == -1 and b'n_images' in lib.sucre_last_error()
        assert lib.sucre_mosaic_feather(tp, engine.MAX_VIEWS + 1, arr, 8, bp, sp) == -1
        assert lib.sucre_mosaic_accumulate_feathered(tp, n, arr, 0, C.byref(g), kp, C.c_float(2.0), 8, bp, ap, 2, sp) == -1
        assert b'flags' in lib.sucre_last_error()
        torch.cuda.synchronize()
    assert bool((buf == 0x5a).all()) and not bool(acc.any())      # nothing ran


# ---- b, c. the accumulator and the outputs ------------------------------------------------------------------------------------------
WIDTHS, DEPTHS = [1, 8, 1024], [0.05, 0.5, 1e6]


def scene_case(key):
    """(views, Js, axes, gsd, host views, host Js, best-view reference, per image D2) of a scene with a NaN patch punched into two
    of its restored images -- made once, never changed."""
    if key not in _CACHE:
        scene = synth.make_scene(96, 64, 6) if key == 'scene' else synth.make_deep_scene(96, 64, 6)
        views = engine.device_views_from_scene(scene, DEV)
        g = torch.Generator().manual_seed(41 if key == 'scene' else 42)
        Js = []
        for k, v in enumerate(views):
            H, W = v.depth.shape
            J = torch.rand((H, W, 3), generator=g) * 0.98 + 0.01
            if k in (1, 4):
                J[10 + k:30 + k, 25:60] = NAN
            Js.append(J.to(DEV))
        axes = sucre.mosaic_axes(views)
        gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
        hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
        base = ref.mosaic(hv, hJ, axes, gsd)
        near = [fref.nearest2(fref.members(v.depth.numpy(), J.numpy())) for v, J in zip(hv, hJ)]
        _CACHE[key] = (views, Js, axes, gsd, hv, hJ, base, near)
    return _CACHE[key]


def oracle(key, H, F):
    ck = (key, float(H), F)
    if ck not in _CACHE:
        views, Js, axes, gsd, hv, hJ, base, near = scene_case(key)
        _CACHE[ck] = fref.blend(hv, hJ, axes, gsd, H, F, base=base, near=near)
    return _CACHE[ck]


@pytest.mark.parametrize('H', DEPTHS)
@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('key', ['scene', 'deep'])
def test_the_accumulator_and_the_outputs_equal_the_restatement(key, F, H):
    """Both kernel forms, batches of 1, 4 and 32 images and the reversed request: one ``acc``, to the bit; the four blended outputs
    equal the restatement's, the five best-view ones the unfeathered run's; F = 1 is the unfeathered blend."""
    views, Js, axes, gsd, hv, hJ, base, near = scene_case(key)
    want = oracle(key, H, F)
    wq = want['wq']
    m = engine.mosaic_of(views, Js, axes, gsd, blend=H, feather=F)
    got = m.result()
    print(f'{key}, F = {F}, H = {H}: {base["Wm"]} x {base["Hm"]} cells, {int(want["samples"].sum())} samples of {len(wq)} pixels, '
          f'{int(((wq > 0) & (wq < 4096)).sum())} weights strictly inside, smallest weight sum {int(want["acc"][:, 6][want["acc"][:, 7] > 0].min())}')
    assert (m.Hm, m.Wm) == (base['Hm'], base['Wm']) and got['feather'] == F and m.feather == F
    assert same_bits(m.acc, want['acc']), int((m.acc.cpu() != want['acc']).sum())
    for k in BLENDED:
        assert same_bits(got[k], want[k]), (k, int((got[k].cpu() != want[k]).sum()))
    unfeathered = engine.mosaic_of(views, Js, axes, gsd, blend=H)
    assert set(got) == set(unfeathered.result()) | {'feather'}
    for k in BEST:
        assert same_bits(got[k], base[k]) and same_bits(got[k], unfeathered.result()[k]), k
    filled = got['source'] >= 0
    assert bool((got['samples'][filled] >= 1).all()) and not bool(got['samples'][~filled].any())
    assert not bool(torch.isnan(got['J_blend'][filled]).any())
    if F == 1:
        assert same_bits(m.acc, unfeathered.acc)
        assert all(same_bits(got[k], unfeathered.result()[k]) for k in BLENDED)
    else:
        assert not same_bits(m.acc, unfeathered.acc)
    others = [engine.mosaic_of(views, Js, axes, gsd, blend=H, feather=F, plain_atomic=True),
              engine.mosaic_of(views, Js, axes, gsd, blend=H, feather=F, batch=1),
              engine.mosaic_of(views, Js, axes, gsd, blend=H, feather=F, batch=4),
              engine.mosaic_of(views[::-1], Js[::-1], axes, gsd, blend=H, feather=F)]
    for other in others:
        assert same_bits(other.acc, m.acc)
        assert all(same_bits(other.result()[k], got[k]) for k in BLENDED)
    near_edge, part = (int(x) for x in m.feather_counts.cpu())
    assert part == sum(int((d > 0).sum()) for d in near) and near_edge == sum(int(((d > 0) & (d < F * F)).sum()) for d in near)


def test_images_of_several_sizes_in_one_batch_equal_the_restatement():
    """Every mask of the 67 x 45, 300 x 5 and 523 x 3 images of the map's cases, 24 images in one call: each image's words sit
    behind the ones before it, rounded up to whole workgroups."""
    views, Js, near = map_cases()
    pick = list(range(8, 16)) + list(range(24, 40))
    views, Js, near = [views[i] for i in pick], [Js[i] for i in pick], [near[i] for i in pick]
    hv, hJ = [host_view(v) for v in views], [J.cpu() for J in Js]
    axes, gsd, H, F = torch.eye(3), 0.05, 0.5, 7
    want = fref.blend(hv, hJ, axes, gsd, H, F, near=near)
    assert int((want['samples'] > 1).sum()) > 0 and bool(((want['wq'] > 0) & (want['wq'] < 4096)).any())
    for batch in (32, 5):
        m = engine.mosaic_of(views, Js, axes, gsd, blend=H, feather=F, batch=batch)
        assert same_bits(m.acc, want['acc']) and all(same_bits(m.result()[k], want[k]) for k in BLENDED)
        near_edge, part = (int(x) for x in m.feather_counts.cpu())
        assert part == sum(int((d > 0).sum()) for d in near) and near_edge == sum(int(((d > 0) & (d < F * F)).sum()) for d in near)


def test_a_fill_fills_from_the_feathered_blend():
    views, Js, axes, gsd, hv, hJ, base, near = scene_case('scene')
    gsd = np.float32(gsd * np.float32(0.5))       # half the default gsd: holes
    R = 3 * float(gsd)
    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, feather=8, fill=R)
    plain = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, feather=8)
    L = m.fill_levels
    host = {k: v.cpu().numpy() for k, v in m.result().items() if torch.is_tensor(v)}
    assert int((host['source'] < 0).sum()) > 0
    for k in BEST + BLENDED:
        assert same_bits(m.result()[k], plain.result()[k]), k
    want = fill_ref.fill(host['J_blend'], host['raw_blend'], host['source'], L)
    assert same_bits(host['J_blend_filled'], want['J_filled']) and same_bits(host['raw_blend_filled'], want['raw_filled'])
    want = fill_ref.fill(host['J'], host['raw'], host['source'], L)
    assert all(same_bits(host[k], want[k]) for k in ('J_filled', 'raw_filled', 'fill_level'))


def test_methods_refuse_what_they_cannot_do():
    views, Js, axes, gsd, *_ = scene_case('scene')
    m = engine.Mosaic(axes, gsd, DEV)
    with pytest.raises(ValueError, match='blend'):
        m.begin(bounds=(0.0, 0.0, 1.0, 1.0), feather=8)
    for bad in (0, 1025, 2.5, NAN):
        with pytest.raises(ValueError, match='feather width F'):
            m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5, feather=bad)
        with pytest.raises(ValueError, match='feather width F'):
            m.feather_map(views, Js, bad)
    assert m.key is None and m.acc is None      # refused before anything is allocated
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5, feather=8)
    assert m.feather == 8 and m.result()['feather'] == 8
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0), blend=0.5)
    assert m.feather is None and 'feather' not in m.result()


# ---- d. the seam property -----------------------------------------------------------------------------------------------------------

def test_the_feather_takes_the_step_out_of_a_footprint_edge():
    """test_mosaic_feather_host.py's crafted pair on the device: A covers the grid with J = 0.2, B its left half with 0.8."""
    hv, hJ = fref.seam_pair()
    views = [engine.DeviceView(depth=v.depth.to(DEV), rgb=v.rgb.to(DEV), K=v.K, R=v.R, t=v.t, name='AB'[i], Kinv=v.Kinv) for i, v in enumerate(hv)]
    Js = [J.to(DEV) for J in hJ]
    axes, gsd, F = torch.eye(3), fref.SEAM_GSD, fref.SEAM_F
    plain = engine.mosaic_of(views, Js, axes, gsd, blend=0.5)
    assert (plain.Hm, plain.Wm) == fref.SEAM_HW
    step_plain = fref.largest_row_step(plain.result()['J_blend'].cpu().numpy())
    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, feather=F)
    step = fref.largest_row_step(m.result()['J_blend'].cpu().numpy())
    print(f'largest step along a row: {step_plain:.6f} unfeathered, {step:.6f} at F = {F}; bound {fref.seam_bound():.6f}')
    assert abs(step_plain - 0.3) <= 2.0 ** -19
    assert step <= fref.seam_bound()
    want = fref.blend(hv, hJ, axes, gsd, 0.5, F)
    assert same_bits(m.acc, want['acc']) and all(same_bits(m.result()[k], want[k]) for k in BLENDED)


# ---- e. the command line ------------------------------------------------------------------------------------------------------------
CLI_BLEND, CLI_FEATHER, CLI_FILL = 0.5, 8, 0.05


@pytest.fixture(scope='module')
def feather_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_feather_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    blend = ['--mosaic-blend', str(CLI_BLEND)]
    runs = {'blend': blend, 'feather': blend + ['--mosaic-feather', str(CLI_FEATHER)],
            'feather_filled': blend + ['--mosaic-feather', str(CLI_FEATHER), '--mosaic-fill', str(CLI_FILL)]}
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


def test_cli_writes_the_feathered_blend_and_leaves_the_best_view_files_alone(feather_run):
    from sucre_amd import sfm
    root, scene, restored, printed = feather_run
    names = [v.name for v in scene.views]
    old = ['mosaic.png', 'mosaic.pt', 'mosaic_raw.png', 'mosaic_source.png', 'mosaic_blend.png', 'mosaic_blend_raw.png']
    filled = ['mosaic_filled.png', 'mosaic_filled_mask.png', 'mosaic_raw_filled.png', 'mosaic_blend_filled.png', 'mosaic_blend_raw_filled.png']
    assert sorted(p.name for p in (root / 'feather').iterdir()) == sorted(old)
    assert sorted(p.name for p in (root / 'feather_filled').iterdir()) == sorted(old + filled)
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    was = torch.load(root / 'blend' / 'mosaic.pt')
    for run, fill in (('feather', None), ('feather_filled', CLI_FILL)):
        for name in ('mosaic.png', 'mosaic_raw.png', 'mosaic_source.png'):
            assert (root / 'blend' / name).read_bytes() == (root / run / name).read_bytes(), (run, name)
        got = torch.load(root / run / 'mosaic.pt')
        m = engine.mosaic_of(views, Js, axes, gsd, blend=CLI_BLEND, feather=CLI_FEATHER, fill=fill)
        want = m.result()
        extra = {'axes', 'gsd', 'lo', 'images', 'n_filled', 'per_image', 'blend'} | ({'fill', 'fill_levels'} if fill else set())
        assert set(got) == set(want) | extra
        assert got['feather'] == CLI_FEATHER == want['feather'] and 'feather' not in was
        for k, v in want.items():
            if torch.is_tensor(v):
                assert same_bits(got[k], v), (run, k)
        for k in BEST:
            assert same_bits(got[k], was[k]), (run, k)
        assert not same_bits(got['J_blend'], was['J_blend'])
        # the lines: those of the run with the blend alone -- the blend's own, the last of them, now counts the feathered samples
        # (a weight may round to nothing at an edge) --, then the feather's, then the fill's
        lines_was, lines = printed['blend'].splitlines(), printed[run].splitlines()
        assert lines[:len(lines_was) - 1] == lines_was[:-1] and len(lines) == len(lines_was) + (2 if fill else 1)
        samples = got['samples'].long()
        n_filled = int((got['source'] >= 0).sum())
        total, most, several = int(samples.sum()), int(samples.max()), int((samples > 1).sum())
        assert lines_was[-1].startswith('mosaic blend of depth') and total <= int(was['samples'].long().sum())
        assert lines[len(lines_was) - 1] == (f'mosaic blend of depth {got["blend"]:.6g} m: {total} samples, {total / n_filled:.2f} per filled cell on '
                                             f'average, {most} at most; {100.0 * several / n_filled:.1f} % of the filled cells blend more than one sample')
        maps = m.feather_map(views, Js, CLI_FEATHER)
        part = sum(int((d > 0).sum()) for d in maps)
        near = sum(int(((d > 0) & (d < CLI_FEATHER ** 2)).sum()) for d in maps)
        smallest = float(got['weight'][got['samples'] > 0].min())
        assert lines[len(lines_was)] == (f'mosaic feather of {CLI_FEATHER} px: {100.0 * near / part:.1f} % of the samples within {CLI_FEATHER} px of an edge; '
                                         f'smallest weight sum in a filled cell {smallest:.6g}')
        assert 0 < near < part and smallest >= 4 / 4096
        if fill:
            assert lines[-1].startswith(f'mosaic fill of {CLI_FILL:.6g} m')
    assert 'mosaic feather' not in printed['blend']
