"""GPU tests of the per-view gains in the store variants, rule branches and command-line modes tests/test_gpu_gains.py does not
reach.

Everything is that file's: the scenes, the float64 reference (reference_table), the bars of the estimate (check_estimate:
delta = 1e-6, 2e-6 with the light model), the numpy restatements of the apply rule (test_gains_host.apply_u8, apply_f32: bit for
bit) and the refit contract (bit for bit a plain run on a store into which the corrected colours were imported).  "Rerun on the
kept file" is held to the bars of test_gpu_trim_variants.test_cli_kept_matches_hold_the_survivors.  No bar is new here.

What is new is WHERE they are applied:
  * the apply with real inverses (INV: ties, clamps, a view that is not kept, an empty view) on the light store (the camera
    points must keep their bits), the u16mm store, and the light store on float32 colours (two extension sets: the gains go to
    the SECOND one, read back through export_view_colour; a launcher that picked the first would scale the camera points);
  * the refit contract in the light, light + float32 colour, u16mm, closed-form and light closed-form variants, with a view
    that holds observations and is not kept, and on a store that was itself imported;
  * the estimate's rule branches ON THE DEVICE: a NaN J under some observations of every view (selected out of both sums,
    still counted), a quotient that is not positive, a sum of squares that overflows float32, a channel with nothing finite;
  * the estimate on an imported light store, and behind a closed-form light fit;
  * --view-gains with --light-model, --use-closed-form, --image-scale and SUCRE_OBS_FORMAT=u16mm, --gain-rounds 2 against the
    API round by round, and --keep-matches: the kept file's colours (MatchesFile.save replays the rule on the host) against the
    colours the corrected STORE holds;
  * MatchesData.iter on a store whose gains were divided out: I is the store's, in every colour variant.
"""
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from sucre_amd import _lib, engine
from test_gains_host import apply_f32, apply_u8, gains_from_sums
from test_gpu_gains import (CLI_ITER, DEV, INV, _api_rounds, _base, _same_bits, check_estimate, device_views, disk_scene,   # noqa: F401
                            fitted, float_scene_of, reference_table, scene_of)
from test_gpu_gains import lists_of as plain_lists_of

pytestmark = pytest.mark.gpu

PX = 75 * 52
KEPT_07 = [True, False, True, True, True, False, True]
FLT_MAX = float(np.finfo(np.float32).max)


def lists_of(obs, inv=None, float_colour=False, light=False):
    """test_gpu_gains.lists_of, with the oracle's camera points along for a light restoration: the fifth element, or the first
    three of six planes in front of the float32 colours."""
    lists = plain_lists_of(obs, inv, float_colour)
    if not light:
        return lists
    out = []
    for o, item in zip(obs, lists):
        cP = torch.tensor(np.ascontiguousarray(o['cP'], np.float32))
        out.append(item[:3] + (None, torch.cat([cP, item[4]]).contiguous()) if float_colour else item + (cP,))
    return out


def imported(scene, lists, min_cover=1e-6, **kw):
    views = device_views(scene)
    r = engine.Restoration(scene.height, scene.width, len(lists), device=DEV, **kw)
    r.import_matches(views[scene.target], lists, min_cover=min_cover)
    assert r._views_dev is None          # no view table: nothing was matched
    return r, views


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the apply with real inverses, in the missing variants -----------------------------------------------------------------
def precondition_07(obs):
    """On the oracle's lists: min_cover = 0.7 keeps [T, F, T, T, T, F, T]; view 1 holds observations, view 5 none."""
    assert [len(o['u1']) / PX > 0.7 for o in obs] == KEPT_07 and len(obs[1]['u1']) > 0 and len(obs[5]['u1']) == 0


def check_u8_apply(r, obs, before, clipped, ext_before=None):
    """The uint8 rule of test_apply_uint8_is_the_numpy_rule on every view of ``r``; with ``ext_before`` the extension planes
    (camera points) of every view keep their bits."""
    kept = r.view_keep().cpu().numpy() != 0
    assert kept.tolist() == KEPT_07 and clipped.dtype == np.int64
    ties = 0
    for k in range(r.n_views):
        z0, rgb0 = before[k]
        z1, rgb1 = [t.cpu().numpy() for t in r.export_view(k)]
        assert np.array_equal(bits(z0), bits(z1)), (k, 'ranges')
        assert (z0 > 0).sum() == len(obs[k]['u1'])
        if ext_before is not None:
            assert np.array_equal(bits(ext_before[k]), bits(r.export_view_ext(k).cpu().numpy())), (k, 'camera points')
        if not kept[k]:
            assert np.array_equal(rgb0, rgb1) and clipped[k] == 0, (k, 'a view that is not kept')
            continue
        at = z0 > 0
        want, n_clip = apply_u8(rgb0[at], INV[k])
        assert np.array_equal(rgb1[at], want), (k, 'colours')
        assert np.array_equal(rgb1[~at], rgb0[~at]), (k, 'empty slots')
        assert clipped[k] == n_clip, (k, 'clipped')
        half = rgb0[at].astype(np.float32) * INV[k][None, :]
        ties += int((half - np.floor(half) == 0.5).sum())
    # properties of the scene and of INV, as in test_apply_uint8_is_the_numpy_rule
    assert 0 < clipped[2] < (before[2][0] > 0).sum() and clipped[4] > 0 and clipped[3] == 0 and ties > 100


def test_apply_light_store_keeps_the_camera_points():
    """uint8 colours next to one extension set, the camera points: the colours follow the uint8 rule, the points keep their bits."""
    scene, obs = scene_of('clean75')
    precondition_07(obs)
    r, views = fitted(scene, 5, min_cover=0.7, light=True)
    before = [tuple(t.cpu().numpy() for t in r.export_view(k)) for k in range(r.n_views)]
    points = [r.export_view_ext(k).cpu().numpy() for k in range(r.n_views)]
    assert all(np.any(p != 0) for k, p in enumerate(points) if len(obs[k]['u1']))
    counts, keep, n_obs = r.view_counts().clone(), r.view_keep().clone(), r.n_obs()
    clipped = r.apply_view_gains(torch.tensor(INV, device=DEV)).cpu().numpy()
    assert r.steps_done == 0
    assert _same_bits(r.view_counts(), counts) and _same_bits(r.view_keep(), keep) and r.n_obs() == n_obs
    check_u8_apply(r, obs, before, clipped, ext_before=points)
    r.fit_init(views[scene.target])
    assert not _same_bits(r.fit(5), r.trace_first)


def test_apply_u16mm_store_and_its_format():
    scene, obs = scene_of('clean75')
    precondition_07(obs)
    r, views = fitted(scene, 5, min_cover=0.7, obs_format='u16mm')
    assert int(r.store_format()[0]) == _lib.STORE_U16MM
    before = [tuple(t.cpu().numpy() for t in r.export_view(k)) for k in range(r.n_views)]
    counts, keep, n_obs = r.view_counts().clone(), r.view_keep().clone(), r.n_obs()
    clipped = r.apply_view_gains(torch.tensor(INV, device=DEV)).cpu().numpy()
    assert _same_bits(r.view_counts(), counts) and _same_bits(r.view_keep(), keep) and r.n_obs() == n_obs
    check_u8_apply(r, obs, before, clipped)
    assert int(r.store_format()[0]) == _lib.STORE_U16MM          # the refinalise decides the format again, the same way
    r.fit_init(views[scene.target])
    assert not _same_bits(r.fit(5), r.trace_first)


def test_apply_light_float_colours_goes_to_the_second_plane_set():
    """Camera points in the first extension set, float32 colours in the second: one float32 multiply on the second, not a bit of
    the first or of the uint8 colour words changes."""
    scene, obs, frgb = float_scene_of('clean75')
    precondition_07(obs)
    r, _ = fitted(scene, 5, min_cover=0.7, frgb=frgb, light=True, float_colour=True)
    assert r.both
    n = r.n_views
    before = [tuple(t.cpu().numpy() for t in r.export_view(k)) for k in range(n)]
    points = [r.export_view_ext(k).cpu().numpy() for k in range(n)]
    colours = [r.export_view_colour(k).cpu().numpy() for k in range(n)]
    kept = r.view_keep().cpu().numpy() != 0
    assert kept.tolist() == KEPT_07
    clipped = r.apply_view_gains(torch.tensor(INV, device=DEV)).cpu().numpy()
    assert np.all(clipped == 0)
    top = 0.0
    for k in range(n):
        z0, rgb0 = before[k]
        z1, rgb1 = [t.cpu().numpy() for t in r.export_view(k)]
        I0, I1 = colours[k], r.export_view_colour(k).cpu().numpy()
        top = max(top, float(I1.max()))
        assert np.array_equal(bits(z0), bits(z1)), (k, 'ranges')
        assert np.array_equal(rgb0, rgb1), (k, 'uint8 colour words')
        assert np.array_equal(bits(points[k]), bits(r.export_view_ext(k).cpu().numpy())), (k, 'camera points')
        at = z0 > 0
        assert at.sum() == len(obs[k]['u1'])
        want = apply_f32(I0[:, at].T, INV[k] if kept[k] else np.ones(3, np.float32)).T
        assert np.array_equal(bits(I1[:, at]), bits(want)), (k, 'colours')
        assert np.array_equal(bits(I1[:, ~at]), bits(I0[:, ~at])), (k, 'empty slots')
        if at.any():   # the two sets before the apply: the oracle's points' range is the stored one, the colours are the pictures' pixels
            o = obs[k]
            assert np.array_equal(I0[:, o['v1'], o['u1']].T, o['I'])
            assert np.any(points[k][:, o['v1'], o['u1']] != I0[:, o['v1'], o['u1']])
    assert top > 1.0      # no clamp


# ---- 2. the refit is a plain run on the corrected store, in the missing variants ----------------------------------------------
REFIT = {'light': dict(light=True), 'light-float': dict(light=True, float_colour=True), 'u16mm': dict(obs_format='u16mm'),
         'closed': dict(), 'light-closed': dict(light=True), 'not-kept': dict()}


def refit_and_compare(case, a, target, scene, obs, T, kw, closed=False, min_cover=1e-6):
    """``a`` holds its first fit (``a.trace_first``): estimate, apply, fit anew; ``b`` imports the oracle's lists with the colours
    taken through the numpy rule (inv = 1 for a view that is not kept) and fits; the two are the same bits."""
    _, inv, _ = a.view_gains()
    inv_host = inv.cpu().numpy()
    a.apply_view_gains(inv)
    a.fit_init(target)
    ta = a.fit(T, use_closed_form=closed)
    kept = a.view_keep().cpu().numpy() != 0
    assert np.all(inv_host[~kept] == 1.0) and np.any(inv_host[kept] != 1.0), case
    b = engine.Restoration(scene.height, scene.width, len(obs), device=DEV, **kw)
    lists = lists_of(obs, np.where(kept[:, None], inv_host, np.float32(1.0)), float_colour=bool(kw.get('float_colour')),
                     light=bool(kw.get('light')))
    b.import_matches(target, lists, min_cover=min_cover)
    b.fit_init(target)
    tb = b.fit(T, use_closed_form=closed)
    for name, x, y in (('J', a.J(), b.J()), ('params', a.params(), b.params()), ('trace', ta, tb),
                       ('view_counts', a.view_counts(), b.view_counts()), ('view_keep', a.view_keep(), b.view_keep())):
        assert _same_bits(x, y), (case, name)
    assert a.n_obs() == b.n_obs() > 0 and bool(torch.isfinite(ta).all()), case
    assert not _same_bits(ta, a.trace_first), case
    return a, b


@pytest.mark.parametrize('case', list(REFIT))
def test_refit_equals_a_plain_run_on_the_corrected_colours(case):
    T = 20
    kw = REFIT[case]
    closed = case.endswith('closed')
    min_cover = 0.7 if case == 'not-kept' else 1e-6
    if kw.get('float_colour'):
        scene, obs, frgb = float_scene_of('bad75')
    else:
        (scene, obs), frgb = scene_of('bad75'), None
    a, views = fitted(scene, T, min_cover=min_cover, closed=closed, frgb=frgb, **kw)
    if case == 'not-kept':   # bad75 changes colours only: the match lists, hence the kept views, are clean75's
        precondition_07(obs)
        assert (a.view_keep().cpu().numpy() != 0).tolist() == KEPT_07 and int(a.view_counts()[1]) == len(obs[1]['u1'])
    a, b = refit_and_compare(case, a, views[scene.target], scene, obs, T, kw, closed=closed, min_cover=min_cover)
    if case == 'u16mm':
        assert int(a.store_format()[0]) == _lib.STORE_U16MM == int(b.store_format()[0])
    if case == 'not-kept':
        assert int(b.view_counts()[1]) == len(obs[1]['u1']) and (b.view_keep().cpu().numpy() != 0).tolist() == KEPT_07


def test_refit_of_a_store_that_was_itself_imported():
    """``a`` is filled by import_matches (no view table): estimate, apply and refit work on it as on a matched store."""
    T = 20
    scene, obs = scene_of('bad75')
    a, views = imported(scene, lists_of(obs))
    a.fit_init(views[scene.target])
    a.trace_first = a.fit(T)
    refit_and_compare('imported-start', a, views[scene.target], scene, obs, T, {})
    assert a._views_dev is None


# ---- 3. the estimate's rule branches, on the device ---------------------------------------------------------------------------
NAN_ROWS = slice(16, 32)       # of 52
BETA_B = 0.01
PARAMS0 = np.array([0.1, 0.0, 0.1, 0.1, 0.1, BETA_B, 0.1, 0.1, 0.1])      # B_G = 0; a small beta_B keeps 3e19 e^(-beta z) large
HUGE = 3e19


def test_estimate_rule_branches_on_the_device():
    """No fit step: fit_init sets J and the parameters, view_gains runs at them.
    R: J = NaN on rows 16 .. 31 -- those terms are selected out of both sums and still counted.
    G: B = 0 and J < 0 -- Ihat < 0, S_IIhat < 0, the quotient is not positive: g = 1.
    B (second call): J = 3e19 -- Ihat is finite in float32, Ihat^2 is not: S_IhatIhat = +inf, g = 1.
    Third call: J = NaN in every pixel of R -- both sums are exactly 0 with n > 0: g = 1."""
    scene, obs = scene_of('bad75')
    views = device_views(scene)
    target = views[scene.target]
    r = engine.Restoration(scene.height, scene.width, len(views), device=DEV)
    r.match(target, views, min_cover=1e-6)
    kept = np.array([o['cover'] > 1e-6 for o in obs])
    # the case, on the oracle's lists: every kept view has observations under the NaN block and outside it
    under = [int(((o['v1'] >= NAN_ROWS.start) & (o['v1'] < NAN_ROWS.stop)).sum()) for o in obs]
    print(f'observations under the NaN rows per view: {under} of {[len(o["u1"]) for o in obs]}')
    assert sum(under) > 0 and all(0 < u < len(o['u1']) for u, o, k in zip(under, obs, kept) if k) and kept.sum() >= 2
    # ... and over the scene's ranges (3e19 e^(-beta_B z) + B)^2 >= (3e19 e^(-beta_B z))^2 > FLT_MAX >= 3e19 + B
    z_max = max(float(o['z'].max()) for o, k in zip(obs, kept) if k)
    assert (HUGE * np.exp(-BETA_B * z_max)) ** 2 > FLT_MAX and HUGE + 1.0 < FLT_MAX

    J0 = (scene.views[scene.target].rgb_u8.to(torch.float64) / 255).to(torch.float32)
    J0[NAN_ROWS, :, 0] = float('nan')
    J0[:, :, 1] = -(J0[:, :, 1] + 0.25)
    r.fit_init(target, params0=PARAMS0, J0=J0)
    gains, inv, sums, kept_dev = check_estimate('NaN rows in R, negative G', r, obs)      # the usual bars; sums[:, 0] counts every observation
    assert np.array_equal(kept_dev, kept)
    assert np.all(sums[kept, 0] > 0)
    # R: what the NaN rows hide is missing from the sums -- less than the same view would give with J finite everywhere
    assert np.all(sums[kept, 4] > 0) and not np.any(gains[kept, 0] == 1.0)
    # G
    assert np.all(sums[kept, 2] < 0) and np.all(sums[kept, 5] > 0)
    assert np.all(gains[:, 1] == 1.0) and np.all(inv[:, 1] == 1.0)
    # B is ordinary in this call
    assert not np.any(gains[kept, 2] == 1.0)

    J1 = J0.clone()
    J1[:, :, 2] = HUGE
    r.fit_init(target, params0=PARAMS0, J0=J1)
    gains2, inv2, sums2 = [t.cpu().numpy() for t in r.view_gains()]
    assert np.all(sums2[~kept] == 0)
    assert np.array_equal(sums2[:, [0, 1, 2, 4, 5]], sums[:, [0, 1, 2, 4, 5]]), 'R and G do not see B'
    assert np.all(np.isposinf(sums2[kept, 6])), 'float32 FMA sums of Ihat^2 overflow'
    assert np.all(np.isfinite(sums2[kept, 3])) and np.all(sums2[kept, 3] > 0)
    assert np.all(gains2[:, 2] == 1.0) and np.all(inv2[:, 2] == 1.0)
    g_ref, inv_ref = gains_from_sums(sums2, kept)
    assert np.array_equal(gains2, g_ref) and np.array_equal(inv2, inv_ref)
    assert np.array_equal(gains2[:, :2], gains[:, :2])

    J2 = J0.clone()
    J2[:, :, 0] = float('nan')
    r.fit_init(target, params0=PARAMS0, J0=J2)
    gains3, inv3, sums3 = [t.cpu().numpy() for t in r.view_gains()]
    assert np.all(sums3[:, 1] == 0) and np.all(sums3[:, 4] == 0) and np.all(sums3[kept, 0] > 0)
    assert np.array_equal(sums3[:, 0], sums[:, 0])
    assert np.all(gains3[:, 0] == 1.0) and np.all(inv3[:, 0] == 1.0)
    g_ref, inv_ref = gains_from_sums(sums3, kept)
    assert np.array_equal(gains3, g_ref) and np.array_equal(inv3, inv_ref)
    assert np.array_equal(sums3[:, [2, 3, 5, 6]], sums[:, [2, 3, 5, 6]])


# ---- 4. the estimate on an imported light store, and behind a closed-form light fit -------------------------------------------
@pytest.mark.parametrize('case', ['imported-light', 'imported-light-closed', 'light-closed'])
def test_estimate_light_variants(case):
    scene, obs = scene_of('bad75')
    closed = case.endswith('closed')
    if case.startswith('imported'):   # the camera points are the fifth element of each list, z = ||cP||
        r, views = imported(scene, lists_of(obs, light=True), light=True)
        r.fit_init(views[scene.target])
        r.fit(10, use_closed_form=closed)
    else:
        r, _ = fitted(scene, 10, closed=True, light=True)
    gains, _, _, kept = check_estimate(case, r, obs, light=True)
    assert not np.any(gains[kept] == 1.0)


# ---- 5. the command line ------------------------------------------------------------------------------------------------------
CLI_MODES = {'light-model': (['--light-model'], dict(light=True)), 'closed-form': (['--use-closed-form'], dict(closed=True)),
             'light-closed-form': (['--light-model', '--use-closed-form'], dict(light=True, closed=True)),
             'image-scale': (['--image-scale', '0.5'], dict(scale=0.5)),
             'light-image-scale': (['--light-model', '--image-scale', '0.5'], dict(light=True, scale=0.5)),
             'u16mm': ([], dict(u16mm=True))}


def api_rounds(root, name, out_dir, rounds, light=False, closed=False, scale=1.0, limit=2.0, u16mm=False):
    """test_gpu_gains._api_rounds in the mode the flags stand for: the command line's own start (model at its scale, matches,
    initial values), then the engine calls.  (``u16mm``: the caller has set SUCRE_OBS_FORMAT, the knob both paths read.)"""
    from sucre_amd import sfm, sucre
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth', image_scale=scale)
    out_dir.mkdir(parents=True, exist_ok=True)
    job = sucre._restore_submit(model[name], model, out_dir, light, closed, 0.000001, list(model.images.values()), 0.05, CLI_ITER, None,
                                False, 0, DEV)
    resto = sucre._adam_begin(job.sucre, job.matches_data)
    assert resto.light == light and resto.float_colour == (scale != 1.0) and resto.obs_format == ('u16mm' if u16mm else 'f32')
    resto.fit(CLI_ITER, use_closed_form=closed)
    records = []
    for _ in range(rounds):
        gains, inv, sums = resto.view_gains(limit)
        records.append((gains.cpu(), sums.cpu(), resto.apply_view_gains(inv).cpu()))
        sucre._adam_begin(job.sucre, job.matches_data)
        resto.fit(CLI_ITER, use_closed_form=closed)
    sucre._pull_results(job.sucre, resto)
    return job, records, resto


def same_as_api(out_dir, stem, job, records):
    g = torch.load(out_dir / f'{stem}_gains.pt')
    assert g['gains'].shape[0] == len(records)
    gain = torch.ones_like(records[0][0])
    for i, (gains, sums, view_clipped) in enumerate(records):
        assert _same_bits(g['gains'][i], gains) and _same_bits(g['sums'][i], sums) and _same_bits(g['view_clipped'][i], view_clipped), i
        gain = gain * gains
    assert _same_bits(g['gain'], gain)
    got = torch.load(out_dir / f'{stem}.pt')
    want = {**job.sucre.cpu().state_dict(), 'J': job.sucre.J.detach().cpu()}
    assert set(got) == set(want)
    for key in got:
        assert _same_bits(got[key], want[key].detach()), key
    return g


@pytest.mark.parametrize('mode', list(CLI_MODES))
def test_cli_view_gains_in_the_other_modes(disk_scene, tmp_path, monkeypatch, mode):
    """As test_cli_view_gains_files for the plain mode: <stem>_gains.pt and <stem>.pt are the engine path's bits (match, fit,
    view_gains, apply_view_gains, fit_init, fit) on the scene as the command line loads it, with the same flags."""
    from sucre_amd import sucre
    root, scene, loaded, scaled = disk_scene
    extra, kw = CLI_MODES[mode]
    if kw.get('u16mm'):
        monkeypatch.setenv('SUCRE_OBS_FORMAT', 'u16mm')
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'cli'), '--image-name', name, '--view-gains'] + extra)
    job, records, _ = api_rounds(root, name, tmp_path / 'api', 1, **kw)
    g = same_as_api(tmp_path / 'cli', stem, job, records)
    n = len(g['views'])
    assert g['gains'].shape == (1, n, 3) and g['sums'].shape == (1, n, 7) and int(g['sums'][0, :, 0].sum()) > 0
    assert not torch.all(g['gain'] == 1.0)


def test_cli_two_rounds_equal_the_api_round_by_round(disk_scene, tmp_path):
    from sucre_amd import sucre
    root, scene, loaded, scaled = disk_scene
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'two'), '--image-name', name, '--view-gains', '--gain-rounds', '2'])
    job, records = _api_rounds(root, name, tmp_path / 'api', 2)
    g = same_as_api(tmp_path / 'two', stem, job, records)
    assert g['gains'].shape[0] == 2 and _same_bits(g['gain'], g['gains'][0] * g['gains'][1])
    assert not _same_bits(g['gains'][0], g['gains'][1])


def store_colours(resto, k, v1, u1):
    """(3, n) float32: view k's colours as the store holds them, in the form MatchesFile.save writes."""
    if resto.both:
        return resto.export_view_colour(k)[:, v1, u1].cpu().numpy()
    if resto.float_colour:
        return resto.export_view_ext(k)[:, v1, u1].cpu().numpy()
    rgb = resto.export_view(k)[1][v1, u1]
    return (rgb.to(torch.float64) / 255).to(torch.float32).T.cpu().numpy()


KEEP_MODES = {'plain': [], 'light-model': ['--light-model'], 'image-scale': ['--image-scale', '0.5'],
              'light-image-scale': ['--light-model', '--image-scale', '0.5']}


@pytest.mark.parametrize('mode', list(KEEP_MODES))
def test_cli_kept_matches_hold_the_store_s_corrected_colours(disk_scene, tmp_path, capsys, mode):
    """--keep-matches --view-gains: MatchesFile.save does not read the store, it replays the rule on the views' pixels on the
    host.  The file's colours must be the bits the corrected store holds after the same two rounds; and a plain run on the file
    restores the image of the run with gains (the bars of test_cli_kept_matches_hold_the_survivors)."""
    from sucre_amd import h5bridge, sucre
    root, scene, loaded, scaled = disk_scene
    extra = KEEP_MODES[mode]
    light, scale = '--light-model' in extra, 0.5 if '--image-scale' in extra else 1.0
    name = scene.names[scene.target]
    stem = Path(name).stem
    first, again = tmp_path / 'first', tmp_path / 'again'
    capsys.readouterr()
    sucre.main(_base(root) + ['--output-dir', str(first), '--image-name', name, '--view-gains', '--gain-rounds', '2', '--keep-matches'] + extra)
    out = capsys.readouterr().out
    assert 'Compute' in out and 'colours with the view gains divided out' in out
    kept = [f for f in first.iterdir() if f.suffix in ('.h5', '.npz')]
    assert len(kept) == 1
    groups = h5bridge.read_groups(kept[0]) if kept[0].suffix == '.h5' else h5bridge.read_npz_groups(kept[0])
    # the store of an API-path restoration taken through the same rounds
    job, records, resto = api_rounds(root, name, tmp_path / 'api', 2, light=light, scale=scale)
    same_as_api(first, stem, job, records)
    keep = resto.view_keep().cpu().numpy() != 0
    names = [im.name for im in job.matches_data.image_list]
    assert set(groups) == {n for n, k in zip(names, keep) if k}
    changed = 0
    for k, view_name in enumerate(names):
        if not keep[k]:
            continue
        g = groups[view_name]
        v1, u1 = torch.tensor(g['v1'].astype(np.int64), device=DEV), torch.tensor(g['u1'].astype(np.int64), device=DEV)
        assert len(g['u1']) == int(resto.view_counts()[k]) == int((resto.export_view(k)[0] > 0).sum())
        want = store_colours(resto, k, v1, u1)
        I = np.asarray(g['I'], np.float32)
        assert I.shape == want.shape and np.array_equal(bits(I), bits(want)), (view_name, 'kept colours')
        view = job.matches_data.image_list[k].device_view(DEV)
        own = view.rgb[torch.tensor(g['v2'].astype(np.int64), device=DEV), torch.tensor(g['u2'].astype(np.int64), device=DEV)]
        own = (own if own.dtype == torch.float32 else (own.to(torch.float64) / 255).to(torch.float32)).T.cpu().numpy()
        changed += int((bits(own) != bits(I)).sum())
    assert changed > 0, 'the gains changed no colour: the comparison would hold for uncorrected colours too'
    # a plain run on the kept file
    again.mkdir()
    shutil.copy(kept[0], again / kept[0].name)
    capsys.readouterr()          # (what the API path printed)
    sucre.main(_base(root) + ['--output-dir', str(again), '--image-name', name, '--keep-matches'] + extra)
    txt = capsys.readouterr().out
    assert 'Compute' not in txt and 'is not reused' not in txt and 'Total of' in txt
    assert not (again / f'{stem}_gains.pt').exists()
    a, b = torch.load(first / f'{stem}.pt'), torch.load(again / f'{stem}.pt')
    assert set(a) == set(b)
    assert np.array_equal(np.isnan(a['J'].numpy()), np.isnan(b['J'].numpy()))
    assert helpers.rms_per_channel(b['J'].numpy(), a['J'].numpy()).max() < (3e-5 if light else 1e-6)
    for k in a:
        if k != 'J':
            assert torch.allclose(a[k], b[k], atol=(2e-3 if k in ('cam2light', 'sigma') else 1e-4) if light else 2e-6), k


# ---- 6. MatchesData.iter on a corrected store ---------------------------------------------------------------------------------
class FloatPixels:
    """A synthetic view whose colour image is a float32 picture off the 1/255 grid (what test_gpu_api.SynthImage reads)."""

    def __init__(self, view, frgb):
        self.name, self.R, self.t, self._view, self._frgb = view.name, view.R, view.t, view, frgb

    def rgb_f32(self):
        return self._frgb

    def depth_f32(self):
        return self._view.depth_f32()


def check_iter_is_the_store(md, r):
    got = list(md.iter(batch_size=1, device='cpu'))
    keep = r.view_keep().cpu().numpy() != 0
    order = [k for k in sorted(range(r.n_views), key=lambda k: md.image_list[k].name if md.image_list else k) if keep[k]]
    assert len(got) == len(order) >= 2
    for (u, v, cP, I), k in zip(got, order):
        v1, u1 = torch.where(r.export_view(k)[0] > 0)
        assert np.array_equal(u.numpy(), u1.cpu().numpy()) and np.array_equal(v.numpy(), v1.cpu().numpy()), k
        want = store_colours(r, k, v1, u1)
        assert I.dtype == torch.float32 and np.array_equal(bits(I.numpy()), bits(want)), (k, 'I is not what the store holds')
        if r.light:
            assert np.array_equal(bits(cP.numpy()), bits(r.export_view_ext(k)[:, v1, u1].cpu().numpy())), (k, 'cP')


@pytest.mark.parametrize('case', ['uint8', 'float', 'light-float'])
def test_matches_data_iterates_the_corrected_colours(case, tmp_path):
    """MatchesData.iter (through _materialise) after a gain round: I is the store's colours, whichever planes hold them."""
    from sucre_amd import loader
    from test_gpu_api import SynthImage
    if case == 'uint8':
        (sc, _), pixels = scene_of('clean75'), scene_of('clean75')[0].views
    else:
        sc, _, frgb = float_scene_of('clean75')
        pixels = [FloatPixels(v, f) for v, f in zip(sc.views, frgb)]
    images = [SynthImage(i + 1, p, sc.K, sc.width, sc.height) for i, p in enumerate(pixels)]
    mf = loader.MatchesFile(tmp_path / 'unused.h5', colmap_model=None)
    images[sc.target].match_images(images, mf, device='cuda', light_model=case == 'light-float')
    md = mf.load_matches()
    r = md.restoration
    assert r.float_colour == (case != 'uint8') and r.both == (case == 'light-float') and r._views_dev is not None
    before = [store_colours(r, k, *torch.where(r.export_view(k)[0] > 0)) for k in range(r.n_views)]
    r.apply_view_gains(torch.tensor(INV[:r.n_views], device=DEV))
    keep = r.view_keep().cpu().numpy() != 0
    after = [store_colours(r, k, *torch.where(r.export_view(k)[0] > 0)) for k in range(r.n_views)]
    assert sum(not np.array_equal(x, y) for x, y, k in zip(before, after, keep) if k) >= 2, 'the round must change colours'
    check_iter_is_the_store(md, r)


def test_matches_data_iterates_an_imported_light_float_store():
    """The same on a store that import_matches filled (no view table, no images): nothing but the store can give I."""
    from sucre_amd import loader
    scene, obs, _ = float_scene_of('clean75')
    r, _ = imported(scene, lists_of(obs, float_colour=True, light=True), light=True, float_colour=True)
    assert r.both
    r.apply_view_gains(torch.tensor(INV, device=DEV))
    check_iter_is_the_store(loader.MatchesData(restoration=r), r)
