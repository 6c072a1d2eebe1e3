"""GPU tests of the uncertainty pass (sucre_fit_uncertainty*, engine.Restoration.uncertainty, --save-uncertainty) against the
cancellation-free float64 restatement of tests/uncertainty_ref.py, fed from the oracle's match lists at the engine's own float32
J() and params(), in every variant of the kernel.

Bars (the same for every case; each test prints its worst |d| / bar).
  count, N, P                exact (integers).
  H per channel              || D (H_dev - H_ref) D ||_F / || D H_ref D ||_F <= 1e-9 with D = diag(H_ref)^-1/2: the same one-pass
                             float64 sums agree with the restatement to 2.6e-12 on the CPU (tests/test_uncertainty_host.py), so
                             400x margin; a float32 step anywhere misses it by five orders.
  SSR                        1e-9 relative.
  jterms                     2^-23 relative: one float32 rounding and a factor of two.
  J_se                       1e-6 relative.
  two calls                  identical bits.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import crafted
import uncertainty_ref as uref
from sucre_amd import engine, synth
from test_gpu_residuals import fitted, scene_observations

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BAR_H, BAR_SSR, BAR_JT, BAR_JSE = 1e-9, 1e-9, 2.0 ** -23, 1e-6


def flat(obs, W, min_cover=1e-6, u16mm=False):
    """px, z, I of the kept views of ``scene_observations``' list."""
    samples = [(u1, v1, cP, I) for cover, u1, v1, cP, I in obs if cover > min_cover]
    return uref.flatten(samples, W, u16mm=u16mm)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


def check(label, r, px, z, I):
    """The common bars.  Returns (the device's arrays on the host, the reference, engine.water_uncertainty's dict)."""
    H, W = r.H, r.W
    dev = r.uncertainty()
    again = r.uncertainty()
    count, jterms, sums = [t.cpu().numpy() for t in dev]
    assert count.dtype == np.int32 and count.shape == (H, W) and jterms.dtype == np.float32 and jterms.shape == (H, W, 3, 4)
    assert sums.dtype == np.float64 and sums.shape == (24,)
    for x, y in zip(dev, again):
        assert _same_bits(x, y), (label, 'two calls differ')
    ref = uref.restatement(px, z, I, r.J().cpu().numpy(), r.params().cpu().numpy()[:9], H, W)
    assert np.array_equal(count, ref['count']), (label, 'count')
    assert sums[0] == ref['N'] and sums[1] == ref['P'] and sums[2] == 0, (label, sums[:3], ref['N'], ref['P'])
    Hd, SSRd = uref.normal_of(sums)
    seen = ref['count'] > 0
    assert np.all(jterms[~seen] == 0), (label, 'jterms where nothing is observed')
    ratios = {'H': uref.scaled_distance(Hd, ref['H']) / BAR_H, 'SSR': float(np.abs(SSRd / ref['SSR'] - 1).max()) / BAR_SSR,
              'jterms': float(np.abs(jterms[seen].astype(np.float64) / ref['jterms'][seen] - 1).max()) / BAR_JT}
    res = engine.water_uncertainty(dev[2])
    if ref['N'] - ref['P'] - 3 > 0:
        assert res['well_posed'].all(), (label, res)
        J_se = engine.j_standard_error(dev[1], dev[0], res)
        assert J_se.is_cuda and J_se.dtype == torch.float32 and J_se.shape == (H, W, 3)
        J_se = J_se.cpu().numpy()
        assert np.array_equal(np.isnan(J_se).any(axis=-1), ~seen) and np.array_equal(np.isnan(J_se).all(axis=-1), ~seen), (label, 'NaN pattern')
        ratios['J_se'] = float(np.abs(J_se[seen] / ref['J_se'][seen] - 1).max()) / BAR_JSE
        ratios['se'] = float(np.abs(res['se'] / ref['se'] - 1).max()) / BAR_JSE
    print(f'{label}: worst |d|/bar ' + ', '.join(f'{k} {v:.3g}' for k, v in ratios.items())
          + f' (N {ref["N"]}, P {ref["P"]}, counts {ref["count"].min()}..{ref["count"].max()}; se red {res["se"][0]}, cond {res["cond"]})')
    for k, v in ratios.items():
        assert v <= 1.0, (label, k, v)
    return (count, jterms, sums), ref, res


@pytest.fixture(scope='module')
def scene75():
    """5x4 tiles, partial in both directions; 7 views, the target is view 3; view 5 (far) sees nothing and is not kept."""
    scene = synth.make_scene(75, 52, 5, seed=11, far_views=1)
    return scene, scene_observations(scene)


def test_plain_partial_tiles_and_a_view_that_is_not_kept(scene75):
    scene, obs = scene75
    r = fitted(scene, 20)
    keep = r.view_keep().cpu().numpy() != 0
    assert not keep[5] and keep.sum() == 6
    (count, _, sums), ref, res = check('plain 75x52, 20 iterations', r, *flat(obs, scene.width))
    assert int(sums[0]) == r.n_obs() and (count == 0).any()
    # the issue's finding on this one-altitude survey: B and gamma are all but undetermined, and almost perfectly anticorrelated
    assert res['corr'][0, 0, 2] < -0.95


def test_tile_count_that_is_no_multiple_of_four():
    """40 x 24 pixels = 3 x 2 tiles: the last workgroup of the pass has two waves without a tile."""
    scene = synth.make_scene(40, 24, 3, seed=7)
    assert (scene.width + 15) // 16 * ((scene.height + 15) // 16) == 6
    check('plain 40x24, 6 tiles', fitted(scene, 20), *flat(scene_observations(scene), scene.width))


def test_min_cover_drops_a_view(scene75):
    scene, obs = scene75
    r = fitted(scene, 20, min_cover=0.7)
    assert (r.view_keep().cpu().numpy() != 0).tolist() == [True, False, True, True, True, False, True]
    (_, _, sums), _, _ = check('plain 75x52 min_cover 0.7', r, *flat(obs, scene.width, min_cover=0.7))
    assert int(sums[0]) == r.n_obs()


def test_closed_form(scene75):
    scene, obs = scene75
    check('closed form', fitted(scene, 20, closed=True), *flat(obs, scene.width))


def test_u16mm_reads_the_quantised_ranges(scene75):
    scene, obs = scene75
    r = fitted(scene, 20, obs_format='u16mm')
    J, params = r.J().cpu().numpy(), r.params().cpu().numpy()
    # on the CPU first: the unquantised ranges give another H, by more than 100x the bar -- otherwise this case proves nothing
    exact = uref.restatement(*flat(obs, scene.width), J, params, scene.height, scene.width)
    quant = uref.restatement(*flat(obs, scene.width, u16mm=True), J, params, scene.height, scene.width)
    apart = uref.scaled_distance(exact['H'], quant['H'])
    print(f'u16mm: H of the unquantised ranges is {apart:.2e} from H of the quantised ones ({apart / BAR_H:.0f} bars)')
    assert apart > 100 * BAR_H
    check('u16mm', r, *flat(obs, scene.width, u16mm=True))


def test_f32plain_store(scene75):
    scene, obs = scene75
    check('f32plain', fitted(scene, 20, obs_format='f32plain'), *flat(obs, scene.width))


def test_float_colours(scene75):
    scene, obs = scene75
    check('float colours', fitted(scene, 20, float_views=True, float_colour=True), *flat(obs, scene.width))


def test_deep_scene():
    scene = synth.make_deep_scene(96, 64, 6, seed=5)
    _, _, res = check('deep 96x64', fitted(scene, 20), *flat(scene_observations(scene), scene.width))
    assert (res['cond'] < 1e6).all()


def test_light_model_is_refused(scene75):
    scene, _ = scene75
    r = fitted(scene, 2, light=True)
    with pytest.raises(NotImplementedError, match='light model'):
        r.uncertainty()


# ---- imported stores ----------------------------------------------------------------------------------------------------------
def _imported(g, rgb, T=10):
    ls = crafted.ListSet(g, rgb=rgb)
    tgt = crafted.target_view(g.H, g.W)
    r = engine.Restoration(g.H, g.W, g.n_views, device=DEV)
    r.import_matches(tgt, crafted.device_lists(ls, 'cuda'), min_cover=g.min_cover)
    J0 = (0.2 + 0.6 * np.random.default_rng(11).random((g.H, g.W, 3))).astype(np.float32)
    r.fit_init(tgt, np.full(9, 0.1, np.float32), J0=torch.from_numpy(J0).cuda())
    r.fit(T)
    ok = g.obs_kept
    return r, (g.px[ok], g.z[ok], ls.I()[ok])


def test_imported_store_with_empty_pixels_and_single_observations():
    g = crafted.CASE['ragged40x24'].geometry()
    cm = g.count_map()
    assert (cm == 0).any() and (cm == 1).any() and cm.max() == 8
    r, lists = _imported(g, crafted.random_colours(g))
    (count, jterms, _), ref, _ = check('imported 40x24, counts 0..8', r, *lists)
    assert np.array_equal(count, cm)


def test_one_observation_per_pixel_is_not_well_posed():
    """Every observation is spent on its pixel's own J: dof = N - P - 3 = -3.  (H is rounding noise around 0 here -- what is left of d
    once J is eliminated is nothing --, so it is not compared.)"""
    g = crafted.CASE['eq1'].geometry()
    r, (px, z, I) = _imported(g, crafted.random_colours(g))
    dev = r.uncertainty()
    count, jterms, sums = [t.cpu().numpy() for t in dev]
    ref = uref.restatement(px, z, I, r.J().cpu().numpy(), r.params().cpu().numpy()[:9], g.H, g.W)
    assert (count == 1).all() and sums[0] == sums[1] == 256 and sums[2] == 0
    assert float(np.abs(jterms.astype(np.float64) / ref['jterms'] - 1).max()) <= BAR_JT
    _, SSR = uref.normal_of(sums)
    assert float(np.abs(SSR / ref['SSR'] - 1).max()) <= BAR_SSR
    res = engine.water_uncertainty(dev[2])
    assert res['dof'] == -3 and not res['well_posed'].any() and np.isnan(res['se']).all() and np.isnan(res['cov']).all()
    assert bool(torch.isnan(engine.j_standard_error(dev[1], dev[0], res)).all())


def test_after_a_trim_round_the_survivors_are_counted(scene75):
    scene, obs = scene75
    views = engine.device_views_from_scene(scene, DEV)
    r = fitted(scene, 20)
    before = r.n_obs()
    dropped, _, _ = r.trim_outliers(2.0)
    r.fit_init(views[scene.target])
    r.fit(20)
    count, jterms, sums = r.uncertainty()
    n_dropped = int(dropped.sum().cpu())
    assert 0 < n_dropped < before and int(sums[0].cpu()) == r.n_obs() == before - n_dropped
    rc, _, stats = r.residuals()
    assert torch.equal(count, rc) and int(sums[1].cpu()) == int((rc > 0).sum().cpu())
    ssr = np.array([float(sums[3 + 7 * c + 6].cpu()) for c in range(3)])
    assert np.allclose(ssr, stats[:, 1:].sum(dim=0).cpu().numpy(), rtol=1e-4, atol=0)    # (the residual pass sums in float32)
    assert engine.water_uncertainty(sums)['well_posed'].all()


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disk_scene(tmp_path_factory):
    from test_gpu_api import write_scene
    root = tmp_path_factory.mktemp('uncertainty_scene')
    scene = synth.make_scene(64, 48, 4, seed=21)
    write_scene(scene, root)
    return root, scene


def _base(root):
    return ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'), '--num-iter', '10']


KEYS = {'B_se', 'beta_se', 'gamma_se', 'cov', 'corr', 'cond', 's2', 'dof', 'n_obs', 'n_pixels', 'normal', 'sums', 'well_posed', 'J_se', 'count'}


def _check_record(q, H, W, pooled=False):
    assert set(q) == KEYS
    for k in ('B_se', 'beta_se', 'gamma_se'):
        assert q[k].dtype == torch.float64 and q[k].shape == (3, 1)
    for k, shape in (('cov', (3, 3, 3)), ('corr', (3, 3, 3)), ('normal', (3, 3, 3)), ('cond', (3,)), ('s2', (3,)), ('sums', (24,))):
        assert q[k].dtype == torch.float64 and q[k].shape == shape, k
    assert q['well_posed'].dtype == torch.bool and q['well_posed'].shape == (3,)
    assert q['J_se'].dtype == torch.float32 and q['J_se'].shape == (H, W, 3)
    assert q['count'].dtype == torch.int32 and q['count'].shape == (H, W)
    assert all(isinstance(q[k], int) for k in ('dof', 'n_obs', 'n_pixels'))
    assert int(q['count'].sum()) == int(q['sums'][0]) and int((q['count'] > 0).sum()) == int(q['sums'][1])
    if not pooled:   # (with a shared fit n_obs, n_pixels and dof are those of the pool; sums and count stay the image's own)
        assert q['n_obs'] == int(q['sums'][0]) and q['n_pixels'] == int(q['sums'][1])


def test_cli_save_uncertainty_files(disk_scene, tmp_path, capsys):
    from PIL import Image as PILImage
    from sucre_amd import sucre
    root, scene = disk_scene
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path), '--image-name', name, '--save-uncertainty'])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith(f'{name}: standard errors B ± ')]
    assert len(line) == 1 and ', beta ± ' in line[0] and ', gamma ± ' in line[0] and '; strongest correlation ' in line[0]
    assert '; median sigma_J R ' in line[0]
    q = torch.load(tmp_path / f'{stem}_uncertainty.pt')
    _check_record(q, 48, 64)
    assert q['dof'] == q['n_obs'] - q['n_pixels'] - 3 and bool(q['well_posed'].all())
    assert torch.equal(q['B_se'][:, 0], q['cov'][:, 0, 0].sqrt()) and torch.equal(q['gamma_se'][:, 0], q['cov'][:, 2, 2].sqrt())
    res = engine.water_uncertainty(q['sums'])
    assert np.array_equal(res['cov'], q['cov'].numpy())
    png = np.asarray(PILImage.open(tmp_path / f'{stem}_uncertainty.png'))
    assert png.dtype == np.uint8 and png.shape == (48, 64)
    assert np.array_equal(png, sucre.uncertainty_image(q['J_se'].numpy())) and np.all(png[q['count'].numpy() == 0] == 0)
    assert (tmp_path / f'{stem}.pt').exists() and (tmp_path / f'{stem}_rgb.png').exists()


def test_cli_shared_water_pools_the_sums(disk_scene, tmp_path, capsys):
    from sucre_amd import sucre
    root, scene = disk_scene
    sucre.main(_base(root) + ['--output-dir', str(tmp_path), '--image-ids', '1', '4', '--shared-water', '--save-uncertainty'])
    out = capsys.readouterr().out
    assert 'shared water: standard errors B ± ' in out
    pooled = torch.load(tmp_path / 'shared_water_uncertainty.pt')
    assert len(pooled['images']) == 3 and pooled['image_sums'].shape == (3, 24)
    total = torch.zeros(24, dtype=torch.float64)
    for name, own in zip(pooled['images'], pooled['image_sums']):
        q = torch.load(tmp_path / f'{Path(name).stem}_uncertainty.pt')
        _check_record(q, 48, 64, pooled=True)
        assert torch.equal(q['sums'], own)
        assert torch.equal(q['cov'], pooled['cov'])          # every image's J_se is made from the pooled covariance
        total = total + own                                    # in request order
    assert torch.equal(pooled['sums'], total)
    assert pooled['n_pixels'] == int(pooled['image_sums'][:, 1].sum()) and pooled['n_obs'] == int(pooled['image_sums'][:, 0].sum())
    assert pooled['dof'] == pooled['n_obs'] - pooled['n_pixels'] - 3


def test_cli_survey_in_batch_launches_equals_single_runs(disk_scene, tmp_path, monkeypatch):
    from sucre_amd import sucre
    root, scene = disk_scene
    monkeypatch.setenv('SUCRE_IMAGES_IN_FLIGHT', '2')
    monkeypatch.setenv('SUCRE_FIT_BATCH', 'auto')
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'survey'), '--image-ids', '1', '4', '--save-uncertainty'])
    got = sorted((tmp_path / 'survey').glob('*_uncertainty.pt'))
    assert len(got) == 3
    for p in got:
        name = p.name.replace('_uncertainty.pt', '.png')
        assert name in scene.names
        sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'single'), '--image-name', name, '--save-uncertainty'])
        a, b = torch.load(p), torch.load(tmp_path / 'single' / p.name)
        _check_record(a, 48, 64)
        for k in ('sums', 'count', 'J_se', 'cov'):
            assert _same_bits(a[k], b[k]), (p.name, k)
