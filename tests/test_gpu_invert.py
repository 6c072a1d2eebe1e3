"""GPU tests of the single-view inversion (sucre_invert_images, engine.invert_images, SUCRe.invert, --apply-water).

The yardstick is the engine's own closed form: with one observation per pixel -- the image matched against itself --
SUCRe.update_J (sucre.py:66-77) is J = (I - l B (1 - e^(-gamma z))) a / a^2, a = l e^(-beta z), and ``invert_images`` must return
the very bits ``Restoration.update_J`` leaves after ``match(view, [view])``.  That comparison is complete only where the two-way
match of the image with itself keeps every pixel with depth > 0, so every scene is first checked for that ON THE ORACLE ALONE
(``case``): a condition on the case, no pixel may be left out.

Against the oracle the bar is the project's crafted-test rule: max |J_engine - J64| <= 8 max |J_oracle - J64| with a floor of
2^-22, J64 a float64 evaluation of the formula written here, the right-hand side measured in the test and printed.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from oracle import oracle
from sucre_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WATER = [.094, .121, .119, .321, .073, .072, .140, .137, .142]           # fitted values, away from the 0.1 start
LIGHT = WATER + [0.02, -0.03, 0.01, 0.05, -0.04, 0.03] + [0.9, 0.1, -0.05, 1.1]   # a non-zero twist, sigma not the identity

_CASES = {}


def case(key):
    """(scene, target view on the device, the same with float32 colours off the 1/255 grid, self samples) -- made once and
    never changed, after the oracle alone has shown that the target's self-match maps every depth > 0 pixel to itself."""
    if key not in _CASES:
        from test_gpu_trim import float_images
        make, index = {'75x52': (lambda: synth.make_scene(75, 52, 5, seed=11, far_views=1), None),
                       '47x33': (lambda: synth.make_scene(47, 33, 2, seed=5), None),
                       '48x32': (lambda: synth.make_scene(48, 32, 2, seed=3), None),
                       # cameras 0.75 .. 4 m above the seabed, half of them oblique: a low one and a tilted one
                       'deep-near': (lambda: synth.make_deep_scene(96, 64, 8, seed=0), 1),
                       'deep-far': (lambda: synth.make_deep_scene(96, 64, 8, seed=0), 0)}[key]
        scene = make()
        index = scene.target if index is None else index
        tgt = scene.views[index]
        cam, d = helpers.oracle_cam(scene, tgt), tgt.depth_f32().numpy()
        m = oracle.match_view(d, cam, d, cam)
        assert len(m) == int((d > 0).sum()) > 0 and np.array_equal(m.u1, m.u2) and np.array_equal(m.v1, m.v2), key
        assert int((d <= 0).sum()) > 0, 'the scenes hold invalid pixels too'
        samples = [(m.u1, m.v1, oracle.unproject(cam, m.u2, m.v2, m.d), oracle.gather_rgb(tgt.rgb_u8.numpy(), m.u2, m.v2))]
        view = engine.device_views_from_scene(scene, DEV)[index]
        frgb = float_images(scene)[index]
        fview = engine.DeviceView(depth=view.depth, rgb=frgb.to(DEV), K=scene.K, R=tgt.R, t=tgt.t, name=tgt.name)
        _CASES[key] = (scene, view, fview, samples)
    return _CASES[key]


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def closed_form(view, params, **kw):
    """The engine's own update_J on a store that holds only the self-match."""
    H, W = view.depth.shape
    r = engine.Restoration(H, W, 1, device=DEV, **kw)
    r.match(view, [view])
    r.fit_init(view, params0=params)
    r.update_J()
    return r.J()


VARIANTS = {'plain': (False, False), 'light': (True, False), 'float': (False, True), 'light-float': (True, True)}


# ---- 1. bitwise against the engine's own closed form ----------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('key', ['75x52', '47x33', '48x32'])
def test_bits_of_the_engines_closed_form(key, variant):
    light, fcolour = VARIANTS[variant]
    scene, view, fview, _ = case(key)
    v, p = (fview if fcolour else view), (LIGHT if light else WATER)
    want = closed_form(v, p, light=light, float_colour=fcolour)
    got = engine.invert_images([v], p, light=light)[0]
    assert got.dtype == torch.float32 and got.shape == (scene.height, scene.width, 3)
    nan = torch.isnan(got).any(dim=2)
    assert torch.equal(nan, view.depth <= 0) and torch.equal(torch.isnan(got).all(dim=2), nan)
    assert same_bits(got, want)
    assert bool((got[~nan] != v.rgb[~nan].float() / (1 if fcolour else 255)).any()), 'the inversion moves the colours'


def test_bits_on_deep_ranges_with_the_plain_float32_store():
    """Ranges from 0.7 m to 9 m (synth.make_deep_scene), the store kept as float32 words."""
    spans = []
    for key in ('deep-near', 'deep-far'):
        scene, view, _, samples = case(key)
        z = np.linalg.norm(samples[0][2].astype(np.float64), axis=0)
        spans += [z.min(), z.max()]
        assert same_bits(engine.invert_images([view], WATER)[0], closed_form(view, WATER, obs_format='f32plain')), key
    assert min(spans) < 0.8 and max(spans) > 8.0, spans


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['75x52', '47x33', '48x32', 'deep-near', 'deep-far'])
def test_against_the_oracle(key):
    scene, view, _, samples = case(key)
    H, W = scene.height, scene.width
    u, v, cP, I = samples[0]
    Jo = oracle.update_J(H, W, samples, np.asarray(WATER, np.float32))
    p = np.asarray(WATER, np.float32).astype(np.float64)
    z = np.sqrt((cP.astype(np.float64) ** 2).sum(axis=0))
    a = np.exp(-p[3:6, None] * z)
    b = p[0:3, None] * (1.0 - np.exp(-p[6:9, None] * z))
    J64 = np.full((H, W, 3), np.nan)
    J64[v, u] = (((I.astype(np.float64) - b) * a) / (a * a)).T
    got = engine.invert_images([view], WATER)[0].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(J64)) and np.array_equal(np.isnan(Jo[v, u]), np.isnan(J64[v, u]))
    ok = ~np.isnan(J64)
    e_oracle = np.abs(Jo.astype(np.float64) - J64)[ok].max()
    e_engine = np.abs(got.astype(np.float64) - J64)[ok].max()
    bar = max(8 * e_oracle, 2.0 ** -22)
    print(f'{key}: max|J_engine - J64| = {e_engine:.3e}, max|J_oracle - J64| = {e_oracle:.3e}, bar = {bar:.3e}')
    assert e_engine <= bar, (key, e_engine, e_oracle)


# ---- 3. launch shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_three_sizes_in_one_launch(variant):
    light, fcolour = VARIANTS[variant]
    views = [case(k)[2 if fcolour else 1] for k in ('75x52', '47x33', '48x32')]
    p = LIGHT if light else WATER
    together = engine.invert_images(views, p, light=light)
    assert len(together) == 3
    for v, J in zip(views, together):
        assert same_bits(J, engine.invert_images([v], p, light=light)[0]), tuple(v.depth.shape)


def test_forty_images_in_one_launch():
    """More images than one set launch of the table carries (32), of three sizes: each equals its launch alone."""
    base = []
    for key in ('75x52', '47x33', '48x32'):
        base += engine.device_views_from_scene(case(key)[0], DEV)
    views = [base[i % len(base)] for i in range(40)]
    assert len({tuple(v.depth.shape) for v in views}) == 3
    alone = [engine.invert_images([v], WATER)[0] for v in base]
    together = engine.invert_images(views, WATER)
    assert len(together) == 40
    for i, J in enumerate(together):
        assert same_bits(J, alone[i % len(base)]), i


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_dirty_table_and_outputs_and_two_runs(variant):
    """Straight on the C ABI: the table and the outputs filled with 0xFF first give the same bits, and so do two runs."""
    light, fcolour = VARIANTS[variant]
    views = [case(k)[2 if fcolour else 1] for k in ('75x52', '47x33')]
    p = LIGHT if light else WATER
    lib = _lib.load()
    flags = (_lib.INVERT_LIGHT if light else 0) | (_lib.INVERT_FLOAT_COLOUR if fcolour else 0)
    pc = (engine.C.c_float * len(p))(*p)

    def run(fill):
        table = torch.empty(lib.sucre_invert_bytes(2), dtype=torch.uint8, device=DEV)
        outs = [torch.empty(tuple(v.depth.shape) + (3,), dtype=torch.float32, device=DEV) for v in views]
        if fill is not None:
            table.fill_(fill)
            for o in outs:
                o.view(torch.uint8).fill_(fill)
        arr = (_lib.InvertImage * 2)()
        for e, v, o in zip(arr, views, outs):
            e.depth, e.rgb, e.J, e.H, e.W, e.Kinv = v.depth.data_ptr(), v.rgb.data_ptr(), o.data_ptr(), v.depth.shape[0], v.depth.shape[1], v.to_struct().Kinv
        with torch.cuda.device(DEV):
            _lib.check(lib.sucre_invert_images(engine.C.c_void_p(table.data_ptr()), 2, arr, pc, flags, engine._stream_ptr()))
        torch.cuda.synchronize()
        return outs

    first, again, dirty = run(None), run(None), run(0xFF)
    for a, b, c, v in zip(first, again, dirty, views):
        assert same_bits(a, b) and same_bits(a, c)
        assert same_bits(a, engine.invert_images([v], p, light=light)[0])


# ---- 4. SUCRe.invert and 5. the command line --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disk_scene(tmp_path_factory):
    from test_gpu_api import write_scene
    root = tmp_path_factory.mktemp('invert_scene')
    scene = synth.make_scene(96, 64, 4, seed=21, far_views=1)
    write_scene(scene, root)
    for light, p in ((False, WATER), (True, LIGHT)):
        w = {'B': torch.tensor(p[0:3]).view(3, 1), 'beta': torch.tensor(p[3:6]).view(3, 1), 'gamma': torch.tensor(p[6:9]).view(3, 1)}
        if light:
            w.update(cam2light=torch.tensor(p[9:15]), sigma=torch.tensor(p[15:19]).view(2, 2))
        torch.save({**w, 'images': scene.names}, root / ('light.pt' if light else 'w.pt'))   # (an extra key, as shared_water.pt has)
    return root, scene


def model_of(root, scale=1.0):
    from sucre_amd import sfm
    return sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth', image_scale=scale)


def _base(root):
    return ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model')]


@pytest.mark.parametrize('closed', [False, True], ids=['J-parameter', 'closed-form'])
def test_module_invert(disk_scene, closed):
    from sucre_amd import sucre
    root, scene = disk_scene
    image = model_of(root)[scene.names[scene.target]]
    s = sucre.SUCRe(image=image, use_closed_form=closed).to(DEV)
    with torch.no_grad():
        for name, lo in (('B', 0), ('beta', 3), ('gamma', 6)):
            getattr(s, name).copy_(torch.tensor(WATER[lo:lo + 3]).view(3, 1))
    assert s.invert() is s
    want = engine.invert_images([image.device_view(DEV)], WATER)[0]
    assert same_bits(s.J.detach(), want)
    assert isinstance(s.J, torch.nn.Parameter) is (not closed)
    lit = sucre.SUCRe(image=image, light_model=True, use_closed_form=True).to(DEV)
    with torch.no_grad():
        lit.load_state_dict(torch.load(root / 'light.pt'), strict=False)
    assert same_bits(lit.invert().J, engine.invert_images([image.device_view(DEV)], LIGHT, light=True)[0])


def test_cli_apply_water(disk_scene, tmp_path, monkeypatch, capsys):
    from PIL import Image as PILImage
    from sucre_amd import loader, sucre
    root, scene = disk_scene
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    decoded = []
    for fn in ('_imread_rgb_u8', '_imread_depth_u16'):
        real = getattr(loader, fn)
        monkeypatch.setattr(loader, fn, lambda path, real=real: (decoded.append(Path(path).name), real(path))[1])
    out = tmp_path / 'survey'
    sucre.main(_base(root) + ['--output-dir', str(out), '--apply-water', str(root / 'w.pt'), '--image-ids', '1', '4', '--num-iter', '7'])
    printed = capsys.readouterr().out
    assert '--apply-water' in printed and 'ignored' in printed and 'Solve least squares' not in printed
    model = model_of(root)
    names = [model.images[i].name for i in range(1, 4)]
    stems = [Path(n).stem for n in names]
    # the decoder ran once per target and never for another image
    assert sorted(decoded) == sorted(names + [f'depth_{s}.png' for s in stems]), decoded
    assert sorted(p.name for p in out.iterdir()) == sorted([f'{s}_rgb.png' for s in stems] + [f'{s}.pt' for s in stems])
    for name, stem in zip(names, stems):
        got = torch.load(out / f'{stem}.pt')
        assert list(got) == ['B', 'beta', 'gamma', 'J']
        assert torch.equal(torch.cat([got[k].flatten() for k in ('B', 'beta', 'gamma')]), torch.tensor(WATER))
        J = engine.invert_images([model[name].device_view(DEV)], WATER)[0]
        assert same_bits(got['J'], J)
        s = sucre.SUCRe(image=model[name], use_closed_form=True)
        s.J = J
        assert np.array_equal(np.asarray(PILImage.open(out / f'{stem}_rgb.png')), np.asarray(s.plot_J()))
        # a run of its own gives the same bits
        single = tmp_path / 'single'
        sucre.main(_base(root) + ['--output-dir', str(single), '--apply-water', str(root / 'w.pt'), '--image-name', name])
        assert same_bits(torch.load(single / f'{stem}.pt')['J'], got['J'])
        assert (single / f'{stem}_rgb.png').read_bytes() == (out / f'{stem}_rgb.png').read_bytes()


def test_cli_apply_water_light_model_and_image_scale(disk_scene, tmp_path, monkeypatch):
    from sucre_amd import sucre
    root, scene = disk_scene
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    name = scene.names[scene.target]
    stem = Path(name).stem
    lit = tmp_path / 'light'
    sucre.main(_base(root) + ['--output-dir', str(lit), '--apply-water', str(root / 'light.pt'), '--image-name', name, '--light-model'])
    assert sorted(p.name for p in lit.iterdir()) == sorted([f'{stem}_rgb.png', f'{stem}_vignetting.png', f'{stem}.pt'])
    got = torch.load(lit / f'{stem}.pt')
    assert list(got) == ['B', 'beta', 'gamma', 'cam2light', 'sigma', 'J']
    assert same_bits(got['J'], engine.invert_images([model_of(root)[name].device_view(DEV)], LIGHT, light=True)[0])
    # a 9-parameter file does not do for the light model
    with pytest.raises(SystemExit) as e:
        sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'no'), '--apply-water', str(root / 'w.pt'), '--image-name', name, '--light-model'])
    assert "'cam2light'" in str(e.value.code) and not (tmp_path / 'no').exists()
    # --image-scale: float32 colours
    half = tmp_path / 'half'
    sucre.main(_base(root) + ['--output-dir', str(half), '--apply-water', str(root / 'w.pt'), '--image-name', name, '--image-scale', '0.5'])
    view = model_of(root, 0.5)[name].device_view(DEV)
    assert view.rgb.dtype == torch.float32 and tuple(view.depth.shape) == (32, 48)
    got = torch.load(half / f'{stem}.pt')['J']
    assert got.shape == (32, 48, 3) and same_bits(got, engine.invert_images([view], WATER)[0])
    assert (half / f'{stem}_rgb.png').exists()
