"""GPU tests of the residual pass (sucre_fit_residuals*, engine.Restoration.residuals, --save-quality): per-pixel and per-view
sums of r^2 against a float64 restatement of the model, in every variant of the kernel.

The reference for the sums is computed HERE, in float64 numpy, from the oracle's match lists: sucre.py:52-64 (l, z) and
sucre.py:79-82 (forward), evaluated at the engine's own float32 J() and params() cast to float64.

Bars.  count and the per-view numbers of observations are integers: exact.  A sum of n squared residuals with reference value S
may differ by   |d| <= 2 delta sqrt(n S) + n delta^2 + 1e-5 S:   an error delta in each modelled intensity moves sum r^2 by at
most sum 2 |r| delta + n delta^2 (Cauchy-Schwarz on the first term); delta = 1e-6 for the plain model (the argument product,
v_exp_f32 and two FMAs on values <= 1 round to about 3e-7: a factor of three is left), 2e-6 with the light model (about twice
as many rounded steps: lP, the quotient, the quadratic form, a second exponential); 1e-5 S covers the float32 accumulation.
A pass that read unquantised ranges from a u16mm store would miss this bar by more than an order of magnitude per pixel.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from oracle import oracle
from sucre_amd import engine, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


# ---- the float64 reference ------------------------------------------------------------------------------------------------
def scene_observations(scene):
    """Per view, in engine order (= scene order): (cover, u1, v1, cP (3,n) float32, I (3,n) float32) from the oracle."""
    per_view, _ = helpers.oracle_scene_samples(scene)
    obs = []
    for (name, _, m), view in zip(per_view, scene.views):
        cP = oracle.unproject(helpers.oracle_cam(scene, view), m.u2, m.v2, m.d)
        I = oracle.gather_rgb(view.rgb_u8.numpy(), m.u2, m.v2)
        obs.append((len(m) / (scene.width * scene.height), m.u1.astype(np.int64), m.v1.astype(np.int64), cP, I))
    return obs


def reference_sums(obs, H, W, J, params, min_cover=1e-6, u16mm=False, light=False):
    """(count (H,W) int64, ssr (H,W,3) float64, view_stats (n_views,4) float64, kept (n_views,) bool)."""
    J64, p = J.astype(np.float64), params.astype(np.float64)
    B, beta, gamma = p[0:3], p[3:6], p[6:9]
    count, ssr = np.zeros((H, W), np.int64), np.zeros((H, W, 3), np.float64)
    stats, kept = np.zeros((len(obs), 4), np.float64), np.zeros(len(obs), bool)
    if light:   # sucre.py:54-61 with se3.exp (se3.py:22-27), float64
        from sucre_amd import se3
        R, t = [x.numpy() for x in se3.exp(torch.tensor(p[9:15], dtype=torch.float64))]
        sigma = p[15:19].reshape(2, 2)
        Minv = np.linalg.inv(sigma.T @ sigma)
    for k, (cover, u1, v1, cP, I) in enumerate(obs):
        kept[k] = cover > min_cover          # sfm.py:136
        if not kept[k]:
            continue
        z32 = np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2])   # the float32 range the store holds (sucre.py:53)
        if u16mm:   # what the fit of a u16mm store reads
            z32 = np.clip(np.rint(z32 * np.float32(1000.0)), np.float32(1.0), np.float32(65535.0)) * np.float32(0.001)
            assert z32.dtype == np.float32
        z, l = z32.astype(np.float64), 1.0
        if light:
            lP = R @ cP.astype(np.float64) + t
            lp = lP[:2] / lP[2]
            l = np.exp(-(lp * (Minv @ lp)).sum(axis=0) / 2)[:, None]
            z = z + np.linalg.norm(lP, axis=0)
        z = z[:, None]
        Ihat = l * (J64[v1, u1] * np.exp(-beta * z) + B * (1 - np.exp(-gamma * z)))   # sucre.py:79-82
        r2 = (I.T.astype(np.float64) - Ihat) ** 2                                       # sucre.py:144
        np.add.at(count, (v1, u1), 1)
        np.add.at(ssr, (v1, u1), r2)
        stats[k] = [len(u1), *r2.sum(axis=0)]
    return count, ssr, stats, kept


def bar(n, S, delta):
    return 2 * delta * np.sqrt(n * S) + n * delta ** 2 + 1e-5 * S


def check_against_reference(label, r, obs, min_cover=1e-6, u16mm=False, light=False):
    delta = 2e-6 if light else 1e-6
    count, ssr, stats = [t.cpu().numpy() for t in r.residuals()]
    H, W = r.H, r.W
    assert count.dtype == np.int32 and count.shape == (H, W) and ssr.dtype == np.float32 and ssr.shape == (H, W, 3)
    assert stats.dtype == np.float64 and stats.shape == (r.n_views, 4)
    rc, rs, rv, kept = reference_sums(obs, H, W, r.J().cpu().numpy(), r.params().cpu().numpy(), min_cover, u16mm, light)
    assert np.array_equal(r.view_keep().cpu().numpy() != 0, kept), label
    assert np.array_equal(count, rc), (label, 'count')
    assert np.array_equal(stats[:, 0], rv[:, 0]), (label, 'observations per view')
    assert np.all(ssr[rc == 0] == 0) and np.all(stats[~kept] == 0), (label, 'zeros where nothing is observed / kept')
    assert np.isfinite(ssr).all() and np.isfinite(stats).all(), label
    pix = np.abs(ssr.astype(np.float64) - rs) / np.maximum(bar(rc[..., None], rs, delta), 1e-300)
    view = np.abs(stats[:, 1:] - rv[:, 1:]) / np.maximum(bar(rv[:, :1], rv[:, 1:], delta), 1e-300)
    pix[rc == 0] = 0.0; view[~kept] = 0.0
    print(f'{label}: worst |d|/bar per pixel {pix.max():.3f}, per view {view.max():.3f} '
          f'({int(rc.sum())} observations, counts {rc.min()}..{rc.max()}, {int((rc == 0).sum())} empty pixels)')
    assert pix.max() <= 1.0, (label, 'per-pixel ssr', pix.max())
    assert view.max() <= 1.0, (label, 'per-view sums', view.max())
    return count, ssr, stats, (rc, rs, rv, kept)


def fitted(scene, T, min_cover=1e-6, closed=False, float_views=False, **kw):
    views = engine.device_views_from_scene(scene, DEV)
    if float_views:
        views = [v.as_float_colour() for v in views]
    r = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
    r.match(views[scene.target], views, min_cover=min_cover)
    r.fit_init(views[scene.target])
    r.fit(T, use_closed_form=closed)
    return r


@pytest.fixture(scope='module')
def scene75():
    """5x4 tiles, partial in both directions; 7 views, the target is view 3; view 5 (far) sees nothing."""
    scene = synth.make_scene(75, 52, 5, seed=11, far_views=1)
    return scene, scene_observations(scene)


@pytest.fixture(scope='module')
def scene71():
    """71 views, all kept: per-pixel counts above one 64-bit mask word."""
    scene = synth.make_scene(48, 32, 70, seed=3)
    return scene, scene_observations(scene)


# ---- 1. plain ---------------------------------------------------------------------------------------------------------------
def test_plain_maps_and_table_exclude_views_below_min_cover(scene75):
    scene, obs = scene75
    r = fitted(scene, 20, min_cover=0.7)
    count, ssr, stats, (rc, rs, rv, kept) = check_against_reference('plain 75x52 min_cover 0.7', r, obs, min_cover=0.7)
    assert kept.tolist() == [True, False, True, True, True, False, True]
    counts = r.view_counts().cpu().numpy()
    assert counts[1] > 0 and counts[5] == 0          # view 1 has chunks in the dense store, but is not kept
    assert np.all(stats[1] == 0) and np.all(stats[5] == 0)
    assert int(count.sum()) == int(counts[kept].sum()) == r.n_obs()
    assert (rc == 0).sum() > 0 and count.max() == 5


def test_plain_71_views(scene71):
    scene, obs = scene71
    r = fitted(scene, 5)
    count, _, _, (rc, _, _, kept) = check_against_reference('plain 48x32 x 71 views', r, obs)
    assert kept.all() and count.max() > 64


def test_plain_more_tiles_than_threads_of_the_view_sums():
    """272 x 250 pixels = 17 x 16 = 272 tiles: residual_view_sum_kernel's threads take tiles t, t + 256, ... -- sixteen of them go
    round twice --, and the scratch index view * n_tiles + tile runs past 256 tiles per view."""
    scene = synth.make_scene(272, 250, 3, seed=4)
    r = fitted(scene, 5)
    assert (scene.width + 15) // 16 * ((scene.height + 15) // 16) == 272
    count, _, stats, (rc, _, _, kept) = check_against_reference('plain 272x250 x 4 views, 272 tiles', r, scene_observations(scene))
    assert kept.all() and (rc == 0).sum() > 0


# ---- 2. the sum of the residuals is the next logged cost --------------------------------------------------------------------
@pytest.mark.parametrize('light', [False, True], ids=['plain', 'light'])
def test_sum_equals_the_next_logged_cost(scene75, light):
    scene, _ = scene75
    r = fitted(scene, 10, light=light)
    _, _, stats = r.residuals()
    total = float(stats[:, 1:].sum().cpu())
    cost = float(r.fit(1)[0, 0].cpu())    # sucre.py:144-150: the cost logged by an iteration is measured before its step
    print(f'sum of residuals vs next cost ({"light" if light else "plain"}): {total:.9e} vs {cost:.9e}, rel {abs(total / cost - 1):.2e}')
    assert abs(total / cost - 1) <= 2e-5


# ---- 3. the other variants --------------------------------------------------------------------------------------------------
def test_closed_form(scene75):
    scene, obs = scene75
    check_against_reference('closed form', fitted(scene, 10, closed=True), obs)


def test_u16mm_reads_the_quantised_ranges(scene75):
    scene, obs = scene75
    r = fitted(scene, 10, obs_format='u16mm')
    check_against_reference('u16mm', r, obs, u16mm=True)


def test_float_colours(scene75):
    scene, obs = scene75
    check_against_reference('float colours', fitted(scene, 10, float_views=True, float_colour=True), obs)


def test_light_model(scene75):
    scene, obs = scene75
    r = fitted(scene, 10, light=True)
    check_against_reference('light model', r, obs, light=True)


def test_light_model_on_float_colours(scene75):
    scene, obs = scene75
    r = fitted(scene, 10, float_views=True, light=True, float_colour=True)
    check_against_reference('light model, float colours', r, obs, light=True)


def test_imported_store(scene75):
    """A workspace filled by import_matches (no view table, no match kernel) gives the same sums."""
    scene, obs = scene75
    views = engine.device_views_from_scene(scene, DEV)
    lists = []
    for cover, u1, v1, cP, I in obs:
        z = np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2])
        lists.append((torch.tensor(u1, dtype=torch.int16), torch.tensor(v1, dtype=torch.int16), torch.tensor(z),
                      torch.tensor(np.rint(I.T * 255).astype(np.uint8))))
    r = engine.Restoration(scene.height, scene.width, len(lists), device=DEV)
    r.import_matches(views[scene.target], lists, min_cover=1e-6)
    r.fit_init(views[scene.target])
    r.fit(10)
    check_against_reference('imported lists', r, obs)


# ---- 4. a pure read, and reproducible ---------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


@pytest.mark.parametrize('light', [False, True], ids=['plain', 'light'])
def test_pure_read_and_reproducible(scene75, light):
    scene, _ = scene75
    a = fitted(scene, 10, light=light)
    first = a.residuals()
    second = a.residuals()
    for x, y in zip(first, second):
        assert _same_bits(x, y)
    ta = a.fit(10)
    b = fitted(scene, 10, light=light)
    tb = b.fit(10)
    assert a.steps_done == b.steps_done == 20
    assert _same_bits(a.J(), b.J()) and _same_bits(a.params(), b.params()) and _same_bits(ta, tb)


def test_module_residuals_leaves_the_optimiser_alone(scene75):
    """SUCRe.residuals: the module's parameters go to the engine, as in update_J; Adam's state and step count stay."""
    from sucre_amd import loader, sucre
    scene, obs = scene75
    r = fitted(scene, 10)
    model = sucre.SUCRe.__new__(sucre.SUCRe)
    torch.nn.Module.__init__(model)
    model.light_model, model.use_closed_form = False, False
    p = r.params().clone()
    model.B, model.beta, model.gamma = [torch.nn.Parameter((p[i:i + 3] * 1.25).view(3, 1)) for i in (0, 3, 6)]
    md = loader.MatchesData(restoration=r)
    before = r.ws.clone()
    count, ssr, stats = model.residuals(md)
    assert r.steps_done == 10 and torch.allclose(r.params(), p * 1.25)
    r.params().copy_(p)
    assert torch.equal(r.ws, before)             # nothing but the nine parameters was written
    rc, rs, rv, _ = reference_sums(obs, r.H, r.W, r.J().cpu().numpy(), (p * 1.25).cpu().numpy())
    assert np.array_equal(count.cpu().numpy(), rc)
    assert np.all(np.abs(stats.cpu().numpy()[:, 1:] - rv[:, 1:]) <= bar(rv[:, :1], rv[:, 1:], 1e-6))


# ---- 5. it finds the bad view -----------------------------------------------------------------------------------------------
def test_finds_the_view_with_a_colour_cast(scene75):
    import copy
    scene, _ = scene75
    bad = copy.copy(scene)
    bad.views = list(scene.views)
    v0 = copy.copy(scene.views[0])
    rgb = v0.rgb_u8.clone()
    rgb[..., 0] = torch.clamp(rgb[..., 0].to(torch.int32) + 40, max=255).to(torch.uint8)
    v0.rgb_u8 = rgb
    bad.views[0] = v0
    r = fitted(bad, 20)
    stats = r.residuals()[2].cpu().numpy()
    kept = (r.view_keep().cpu().numpy() != 0) & (stats[:, 0] > 0)
    red = np.where(kept, np.sqrt(stats[:, 1] / np.maximum(stats[:, 0], 1)), -1.0)
    others = red[kept & (np.arange(len(red)) != 0)]
    print(f'red RMS per view {red}, view 0 / median of the others = {red[0] / np.median(others):.2f}')
    assert kept[0] and int(red.argmax()) == 0
    assert red[0] >= 2 * np.median(others)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disk_scene(tmp_path_factory):
    from test_gpu_api import scene_as_loaded, write_scene
    from sucre_amd import sfm
    root = tmp_path_factory.mktemp('quality_scene')
    scene = synth.make_scene(96, 64, 4, seed=21, far_views=1)
    write_scene(scene, root)
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    return root, scene, scene_as_loaded(scene, model)


def _base(root):
    return ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'), '--num-iter', '10']


QUALITY_FILES = ('_quality.pt', '_coverage.png', '_residual.png')


def test_cli_save_quality_files(disk_scene, tmp_path, capsys):
    from PIL import Image as PILImage
    from sucre_amd import sucre
    root, scene, loaded = disk_scene
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'off'), '--image-name', name])
    assert (tmp_path / 'off' / f'{stem}.pt').exists()
    assert not [p for p in (tmp_path / 'off').iterdir() if p.name.endswith(QUALITY_FILES)]
    capsys.readouterr()
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'on'), '--image-name', name, '--save-quality'])
    out = capsys.readouterr().out
    assert f'{name}: residual RMS R ' in out and 'worst kept view' in out
    q = torch.load(tmp_path / 'on' / f'{stem}_quality.pt')
    assert set(q) == {'count', 'ssr', 'views', 'view_kept', 'view_n', 'view_ssr'}
    n = len(q['views'])
    assert q['count'].dtype == torch.int32 and q['count'].shape == (64, 96)
    assert q['ssr'].dtype == torch.float32 and q['ssr'].shape == (64, 96, 3)
    assert q['view_kept'].dtype == torch.bool and q['view_kept'].shape == (n,)
    assert q['view_n'].dtype == torch.int64 and q['view_n'].shape == (n,)
    assert q['view_ssr'].dtype == torch.float64 and q['view_ssr'].shape == (n, 3)
    # the matched views in engine order, and the oracle's match counts for the kept ones
    per_view, _ = helpers.oracle_scene_samples(loaded)
    assert all(isinstance(v, str) for v in q['views']) and set(q['views']) <= set(scene.names)
    kept_names = [v for v, k in zip(q['views'], q['view_kept'].tolist()) if k]
    assert kept_names == [nm for nm, k, _ in per_view if k]
    assert [int(x) for x, k in zip(q['view_n'], q['view_kept'].tolist()) if k] == [len(m) for _, k, m in per_view if k]
    assert int(q['count'].sum()) == int(q['view_n'].sum())
    # the two pictures are the stated mappings of the tensors
    cov = np.asarray(PILImage.open(tmp_path / 'on' / f'{stem}_coverage.png'))
    res = np.asarray(PILImage.open(tmp_path / 'on' / f'{stem}_residual.png'))
    assert cov.dtype == np.uint8 and cov.shape == (64, 96) and res.dtype == np.uint8 and res.shape == (64, 96)
    count = q['count'].numpy().astype(np.int64)
    assert np.array_equal(cov, np.uint8(255 * count // int(q['view_kept'].sum())))
    rms = np.sqrt(np.where(count > 0, q['ssr'].numpy().astype(np.float64).sum(-1) / np.maximum(3 * count, 1), 0.0))
    assert np.array_equal(res, np.uint8(255 * np.minimum(1.0, rms / 0.25))) and np.all(res[count == 0] == 0)
    # the other outputs are the bits of a run without the flag
    a, b = torch.load(tmp_path / 'off' / f'{stem}.pt'), torch.load(tmp_path / 'on' / f'{stem}.pt')
    for k in a:
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), k


@pytest.mark.parametrize('fit_batch', ['1', 'auto'], ids=['two-in-flight', 'one-launch-per-iteration'])
def test_cli_survey_quality_equals_single_runs(disk_scene, tmp_path, monkeypatch, fit_batch):
    from sucre_amd import sucre
    root, scene, loaded = disk_scene
    monkeypatch.setenv('SUCRE_IMAGES_IN_FLIGHT', '2')
    monkeypatch.setenv('SUCRE_FIT_BATCH', fit_batch)
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'survey'), '--image-ids', '1', '4', '--save-quality'])
    got = sorted((tmp_path / 'survey').glob('*_quality.pt'))
    assert len(got) == 3
    for p in got:
        name = p.name.replace('_quality.pt', '.png')
        assert name in scene.names
        sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'single'), '--image-name', name, '--save-quality'])
        a, b = torch.load(p), torch.load(tmp_path / 'single' / p.name)
        assert a['views'] == b['views']
        for k in ('count', 'ssr', 'view_kept', 'view_n', 'view_ssr'):
            assert _same_bits(a[k], b[k]), (p.name, k)


def test_cli_shared_water_save_quality(disk_scene, tmp_path):
    from sucre_amd import sucre
    root, scene, loaded = disk_scene
    sucre.main(_base(root) + ['--output-dir', str(tmp_path), '--image-ids', '1', '3', '--shared-water', '--save-quality'])
    assert (tmp_path / 'shared_water.pt').exists()
    stems = [p.name[:-len('_quality.pt')] for p in sorted(tmp_path.glob('*_quality.pt'))]
    assert len(stems) == 2
    for stem in stems:
        for suffix in QUALITY_FILES:
            assert (tmp_path / f'{stem}{suffix}').exists(), (stem, suffix)
        q = torch.load(tmp_path / f'{stem}_quality.pt')
        assert int(q['count'].sum()) == int(q['view_n'].sum()) > 0 and bool(torch.isfinite(q['ssr']).all())
