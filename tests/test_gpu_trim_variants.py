"""GPU tests of the outlier trim in the store variants, branches and command-line modes tests/test_gpu_trim.py does not reach.

Everything is that file's: the float64 reference (reference_r2), the bars (delta = 1e-6, 2e-6 with the light model -- the
residual suite holds float32 colours to the same delta, a float32 colour is read with no rounding step of its own), the undecided
band 2 delta sqrt(tau^2) + delta^2 + 2^-21 tau^2, the cap max(2, 1e-4 N) on undecided observations, and the refit contract (bit
for bit a plain run on a store into which only the survivors were imported).  No bar is new here.

What is new is WHERE they are applied:
  * float32 colours that are not k/255 (trim_kernel<false, SUCRE_EXT_COLOUR, NoLight>) and the light model on them (<false,
    SUCRE_EXT_POINTS_COLOUR, LightModel>: two extension sets, colours from the second) -- a kernel that read the uint8 colour
    words, or the camera points for the colours, is off by far more than delta;
  * the closed form in front of the trim in every one of them;
  * a view that holds observations and is NOT kept when the trim runs (sweep 2 restates its range pair and must leave everything
    else): min_cover = 0.7 keeps views [T, F, T, T, T, F, T] of the 75 x 52 scene, view 1 with 2495 observations is not kept;
  * what that restated pair is for: a matched store whose smallest range is a dropped observation of a kept view, held in the
    pair of a view that is not kept -- the store's span must be the survivors';
  * a second round after the first one pushed a view below min_cover;
  * a store filled by import_matches (no view table);
  * the store's format decision after a trim: f32 words before, 24-bit offsets once the far observations are gone;
  * --trim-outliers with --light-model, --use-closed-form, --image-scale, --trim-rounds 2 and --keep-matches, and sucre.adam on a
    list-backed MatchesData.
"""
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from sucre_amd import _lib, engine
from test_gpu_trim import (DEV, K_SIGMA, PATCH, _base, _same_bits, device_views, disk_scene, fitted, float_scene_of,   # noqa: F401
                           plant, refit_contract, scene_observations, scene_of, stored_ranges, trim_and_check)

pytestmark = pytest.mark.gpu

PX = 75 * 52
KEPT_07 = [True, False, True, True, True, False, True]


# ---- stores that are imported, not matched ----------------------------------------------------------------------------------
def ranges_of(cP):
    return np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2])   # float32, the order of sucre.py:53


def lists_of(obs, light=False):
    """What import_matches takes, from the oracle's lists (as test_gpu_residuals.py::test_imported_store builds them); the camera
    points as the fifth element with the light model."""
    lists = []
    for u1, v1, cP, I, _, _ in obs:
        item = (torch.tensor(u1, dtype=torch.int16), torch.tensor(v1, dtype=torch.int16), torch.tensor(ranges_of(cP)),
                torch.tensor(np.rint(I.T * 255).astype(np.uint8)))
        if light:
            item += (torch.tensor(np.ascontiguousarray(cP)),)
        lists.append(item)
    return lists


def imported(scene, lists, T, min_cover=1e-6, closed=False, **kw):
    views = device_views(scene)
    r = engine.Restoration(scene.height, scene.width, len(lists), device=DEV, **kw)
    r.import_matches(views[scene.target], lists, min_cover=min_cover)
    r.fit_init(views[scene.target])
    r.fit(T, use_closed_form=closed)
    return r, views


# ---- 1. decisions against float64, in the missing variants ------------------------------------------------------------------
DECISIONS = {'float-colour': dict(float_colour=True), 'float-colour-closed': dict(float_colour=True, closed=True),
             'light-closed': dict(light=True, closed=True), 'light-float-colour': dict(light=True, float_colour=True),
             'light-float-colour-closed': dict(light=True, float_colour=True, closed=True)}


@pytest.mark.parametrize('case', list(DECISIONS))
def test_decisions_in_the_other_store_variants(case):
    kw = dict(DECISIONS[case])
    closed = kw.pop('closed', False)
    if kw.get('float_colour'):
        scene, obs, frgb = float_scene_of('planted75')
        off_grid = max(float(np.abs(o[3] * 255 - np.rint(o[3] * 255)).max()) for o in obs if len(o[0]))
        assert off_grid > 0.05, 'the colours must be off the 1/255 grid'
    else:
        (scene, obs), frgb = scene_of('planted75'), None
    r, _ = fitted(scene, 20, closed=closed, frgb=frgb, **kw)
    _, _, _, zeroed = trim_and_check(case, r, obs, light=bool(kw.get('light')))
    assert zeroed.sum() > 0


@pytest.mark.parametrize('light', [False, True], ids=['plain', 'light'])
def test_decisions_with_a_view_that_holds_observations_and_is_not_kept(light):
    """Sweep 2's branch for such a view: its range pair is restated, its observations, colours, count and extension planes stay."""
    scene, obs = scene_of('planted75')
    assert [len(o[0]) / PX > 0.7 for o in obs] == KEPT_07 and len(obs[1][0]) > 0   # the precondition, on the oracle's lists
    print(f'view 1 holds {len(obs[1][0])} observations and is not kept')
    r, _ = fitted(scene, 20, min_cover=0.7, light=light)
    view_1 = lambda: r.export_view(1) + ((r.export_view_ext(1),) if light else ()) + (r.view_counts()[1:2].clone(),)   # noqa: E731
    before = view_1()
    assert int(before[-1]) == len(obs[1][0]) and int((before[0] > 0).sum()) == len(obs[1][0])
    _, _, _, zeroed = trim_and_check(f'min_cover 0.7{", light" if light else ""}', r, obs, light=light, min_cover=0.7)
    assert zeroed.sum() > 0
    for x, y in zip(before, view_1()):
        assert _same_bits(x, y), 'the view that is not kept changed'
    assert (r.view_keep().cpu().numpy() != 0).tolist() == KEPT_07


@pytest.mark.parametrize('light', [False, True], ids=['plain', 'light'])
def test_decisions_on_an_imported_store(light):
    scene, obs = scene_of('planted75')
    r, _ = imported(scene, lists_of(obs, light), 20, light=light)
    assert r._views_dev is None          # no view table: nothing was matched
    _, _, _, zeroed = trim_and_check(f'imported{", light" if light else ""}', r, obs, light=light)
    assert zeroed.sum() > 0


# ---- 2. the refit contract where the store changes shape ----------------------------------------------------------------------
@pytest.mark.parametrize('case', ['float-colour', 'light-float-colour'])
def test_refit_equals_a_plain_run_on_the_survivors_with_float_colours(case):
    scene, obs, frgb = float_scene_of('planted75')
    a, _ = refit_contract(case, scene, 20, frgb=frgb, obs=obs, float_colour=True, light=case.startswith('light'))
    assert a.n_obs() < sum(len(o[0]) for o in obs)


@pytest.mark.parametrize('rounds', [1, 2], ids=['one-round', 'two-rounds'])
def test_refit_with_a_view_that_is_not_kept(rounds):
    """All views are exported and imported, view 1 included, with the same min_cover: the equality of store_format holds the
    range pair the trim restates for view 1 to account."""
    scene, obs = scene_of('planted75')
    assert [len(o[0]) / PX > 0.7 for o in obs] == KEPT_07 and len(obs[1][0]) > 0
    a, b = refit_contract(f'min_cover 0.7, {rounds} round(s)', scene, 20, rounds=rounds, min_cover=0.7)
    assert all(k.tolist() == KEPT_07 for k in a.kept_before_round)
    assert int(a.view_counts()[1]) == len(obs[1][0]) and a.n_obs() < sum(len(o[0]) for o, k in zip(obs, KEPT_07) if k)


def test_refit_of_a_second_round_after_a_view_fell_below_min_cover():
    """View 0 is kept in round 1 and not in round 2: round 2 walks a view that is not kept and that round 1 partly emptied."""
    scene, obs = scene_of('planted75')
    n0 = len(obs[0][0])
    min_cover = (n0 - 40) / PX          # as test_refit_when_the_planted_view_falls_below_min_cover
    # the precondition on the float64 reference: round 1 takes more than 40 observations from view 0, whichever way the (at most
    # two: trim_and_check's cap) undecided observations and the guards of their pixels go
    r, _ = fitted(scene, 20, min_cover=min_cover)
    _, drops, _, _ = trim_and_check('view loss, round 1', r, obs, min_cover=min_cover)
    assert int(drops[0].sum()) - 2 > 40, 'view 0 must not be kept in round 2'
    a, b = refit_contract('view loss, two rounds', scene, 20, rounds=2, min_cover=min_cover)
    first, second = a.kept_before_round
    assert first[0] and not second[0] and second.sum() >= 2
    counts = a.view_counts().cpu().numpy()
    assert 0 < counts[0] < n0 - 40 and not bool(a.view_keep()[0])


PATCH_VIEW_1 = (slice(19, 33), slice(26, 38))   # rows, columns of view 1 around its pixel (32, 26), which holds the image's smallest range
_SMALLEST = []


def smallest_range_case():
    """The clean 75 x 52 scene with the patch planted in VIEW 1, over the observation with the smallest range of the whole image."""
    if not _SMALLEST:
        scene = plant(scene_of('clean75')[0], PATCH_VIEW_1, view=1)
        _SMALLEST.append((scene, scene_observations(scene)))
    return _SMALLEST[0]


def test_a_dropped_range_does_not_stay_in_the_span_through_a_view_that_is_not_kept():
    """A matched store keeps the ranges a match wave saw over its views (k, k + 4, ...) in the pair of the LAST of them.  Here
    that is view 5 for view 1: view 5 is empty and not kept, view 1 is kept and loses the observation with the image's smallest
    range.  Unless the trim restates the pair of the view that is not kept, that range stays in the span of the store."""
    scene, obs = smallest_range_case()
    patterns = [ranges_of(o[2]).view(np.uint32) for o in obs]
    k = int(np.argmin([int(p.min()) if len(p) else 2 ** 32 for p in patterns]))
    i = int(patterns[k].argmin())
    # the case, on the oracle's lists: the smallest range is view 1's, and the last view of 1, 5, 9, ... is the empty view 5
    assert k == 1 and len(obs) == 7 and len(obs[5][0]) == 0 and len(obs[1][0]) > 0
    r, _ = fitted(scene, 20)
    assert int(r.store_format().cpu().numpy().view(np.uint32)[2]) == int(patterns[1][i])
    _, drops, _, zeroed = trim_and_check('smallest range', r, obs)
    survivors = np.concatenate([p[~d] for p, d in zip(patterns, drops) if d is not None])
    print(f'smallest range: {int(patterns[1][i]):#x} dropped {bool(drops[1][i])}, the survivors\' smallest {int(survivors.min()):#x}')
    assert drops[1][i] and int(survivors.min()) > int(patterns[1][i]), 'the smallest range must be dropped'   # on the reference
    assert zeroed[1, obs[1][1][i], obs[1][0][i]]
    keep = r.view_keep().cpu().numpy() != 0
    assert keep[1] and not keep[5]
    fmt = r.store_format().cpu().numpy().view(np.uint32)
    left = stored_ranges(r)
    left = left[left > 0].view(np.uint32)
    assert int(fmt[2]) == int(left.min()) > int(patterns[1][i]) and int(fmt[3]) == int(left.max())
    refit_contract('smallest range', scene, 20)


def flip_case():
    """planted75's lists with the camera points (hence the ranges: a power of two scales ||cP|| exactly) of view 0's planted
    observations multiplied by 8."""
    scene, obs = scene_of('planted75')
    u1, v1, cP, I, u2, v2 = obs[0]
    far = (v2 >= PATCH[0].start) & (v2 < PATCH[0].stop) & (u2 >= PATCH[1].start) & (u2 < PATCH[1].stop)
    cP8 = cP.copy()
    cP8[:, far] *= np.float32(8.0)
    return scene, [(u1, v1, cP8, I, u2, v2)] + list(obs[1:]), far


def span(patterns):
    return int(patterns.max()) - int(patterns.min())


def test_store_format_flips_once_the_far_observations_are_gone():
    scene, obs, far = flip_case()
    assert far.sum() >= 100
    r, views = imported(scene, lists_of(obs), 20)
    fmt_before = r.store_format().cpu().numpy().view(np.uint32).copy()
    _, drops, _, zeroed = trim_and_check('format flip', r, obs)
    # the case, on the float64 reference alone
    patterns = [ranges_of(o[2]).view(np.uint32) for o in obs]
    everything = np.concatenate(patterns)
    survivors = np.concatenate([p[~d] for p, d in zip(patterns, drops) if d is not None])
    print(f'format flip: span {span(everything):#x} -> {span(survivors):#x}, {int(drops[0][far].sum())} of {int(far.sum())} far observations dropped')
    assert span(everything) > 0xfffffd, 'the untrimmed store must not fit 24-bit offsets'
    assert drops[0][far].all(), 'every far observation must be dropped'
    assert span(survivors) <= 0xfffffd, 'the survivors must fit 24-bit offsets'
    # the store
    fmt_after = r.store_format().cpu().numpy().view(np.uint32)
    assert fmt_before[0] == _lib.STORE_F32 and fmt_after[0] == _lib.STORE_Z24
    left = stored_ranges(r)
    left = left[left > 0].view(np.uint32)
    assert int(fmt_after[2]) == int(left.min()) and int(fmt_after[3]) == int(left.max())
    assert int(fmt_after[3]) < int(patterns[0][far].min())          # no far range is left in the span


def test_refit_across_the_format_flip():
    scene, obs, far = flip_case()
    lists = lists_of(obs)
    a, b = refit_contract('format flip', scene, 20, start=lambda: imported(scene, lists, 20))
    assert int(a.store_format()[0]) == _lib.STORE_Z24 == int(b.store_format()[0])
    # the same with a store that stays on f32 words: another layout of the same observations, the same fit
    c, views = imported(scene, lists, 20, obs_format='f32plain')
    assert int(c.store_format()[0]) == _lib.STORE_F32
    c.trim_outliers(K_SIGMA)
    assert int(c.store_format()[0]) == _lib.STORE_F32
    c.fit_init(views[scene.target])
    tc = c.fit(20)
    assert _same_bits(a.J(), c.J()) and _same_bits(a.params(), c.params()) and _same_bits(a.trace, tc)
    assert _same_bits(a.view_counts(), c.view_counts()) and a.n_obs() == c.n_obs()


# ---- 3. the command line and the host entry points ----------------------------------------------------------------------------
def _trim_run(root, out_dir, name, capsys, *extra):
    from sucre_amd import sucre
    capsys.readouterr()
    sucre.main(_base(root) + ['--output-dir', str(out_dir), '--image-name', name, '--trim-outliers', '3'] + list(extra))
    stem = Path(name).stem
    return capsys.readouterr().out, torch.load(out_dir / f'{stem}_trim.pt'), stem


def _check_record(t, out, name, rounds, H, W):
    n = len(t['views'])
    assert t['dropped'].dtype == torch.int32 and t['dropped'].shape == (rounds, H, W)
    assert t['view_dropped'].dtype == torch.int64 and t['view_dropped'].shape == (rounds, n)
    assert t['thresholds'].dtype == torch.float32 and t['thresholds'].shape == (rounds, 3)
    assert t['n_obs'].shape == (rounds,) and t['view_kept'].shape == (rounds, n)
    for i in range(rounds):
        D = int(t['view_dropped'][i].sum())
        assert D == int(t['dropped'][i].sum())
        assert f'{name}: trim round {i + 1} dropped {D} of {int(t["n_obs"][i])} observations (threshold R ' in out
    return int(t['view_dropped'][0].sum())


CLI_MODES = {'light-model': (['--light-model'], True, False), 'closed-form': (['--use-closed-form'], False, True),
             'light-closed-form': (['--light-model', '--use-closed-form'], True, True)}


@pytest.mark.parametrize('mode', list(CLI_MODES))
def test_cli_trim_in_the_other_fit_modes(disk_scene, tmp_path, capsys, mode):
    """As test_cli_trim_outliers_files for the plain mode: the decisions of the command line are those of the engine path
    (match, fit, trim) bit for bit."""
    root, scene, loaded = disk_scene
    extra, light, closed = CLI_MODES[mode]
    name = scene.names[scene.target]
    out, t, stem = _trim_run(root, tmp_path, name, capsys, *extra)
    assert _check_record(t, out, name, 1, 64, 96) > 0
    assert (tmp_path / f'{stem}_trimmed.png').exists()
    views = engine.device_views_from_scene(loaded, DEV)
    r = engine.Restoration(loaded.height, loaded.width, len(views), device=DEV, light=light)
    r.match(views[loaded.target], views)
    r.fit_init(views[loaded.target])
    r.fit(10, use_closed_form=closed)
    dropped, _, _ = r.trim_outliers(3.0)
    assert _same_bits(t['dropped'][0], dropped.cpu())


@pytest.mark.parametrize('extra', [[], ['--light-model']], ids=['image-scale', 'light-image-scale'])
def test_cli_trim_on_resized_images(disk_scene, tmp_path, capsys, extra):
    from PIL import Image as PILImage
    root, scene, loaded = disk_scene
    name = scene.names[scene.target]
    out, t, stem = _trim_run(root, tmp_path, name, capsys, '--image-scale', '0.5', '--save-quality', *extra)
    D = _check_record(t, out, name, 1, 32, 48)
    assert D > 0
    assert np.asarray(PILImage.open(tmp_path / f'{stem}_trimmed.png')).shape == (32, 48)
    assert torch.load(tmp_path / f'{stem}.pt')['J'].shape == (32, 48, 3)
    q = torch.load(tmp_path / f'{stem}_quality.pt')          # the final fit's counts are the survivors'
    assert q['count'].shape == (32, 48) and int(q['count'].sum()) == int(t['n_obs'][0]) - D


def test_cli_two_rounds(disk_scene, tmp_path, capsys):
    """_enqueue_trim records n_obs and view_kept BEFORE its round, and n_obs is the count over the kept views.  A view leaves
    view_kept between the rounds only when count / (96 * 64) <= 1e-6, i.e. with nothing left, and views that are not kept lose
    nothing: n_obs[1] = n_obs[0] - sum(view_dropped[0])."""
    from PIL import Image as PILImage
    root, scene, loaded = disk_scene
    name = scene.names[scene.target]
    out, t, stem = _trim_run(root, tmp_path, name, capsys, '--trim-rounds', '2')
    assert _check_record(t, out, name, 2, 64, 96) > 0
    kept = t['view_kept']
    assert kept.dtype == torch.bool and not (kept[1] & ~kept[0]).any() and int(t['view_dropped'][0][~kept[0]].sum()) == 0
    assert int(t['view_dropped'][1][~kept[1]].sum()) == 0
    assert int(t['n_obs'][1]) == int(t['n_obs'][0]) - int(t['view_dropped'][0].sum())
    png = np.asarray(PILImage.open(tmp_path / f'{stem}_trimmed.png'))
    assert np.array_equal(png, np.uint8(255 * t['dropped'].numpy().astype(np.int64).sum(axis=0) // int(kept[0].sum())))
    assert t['k'] == 3.0


@pytest.mark.parametrize('extra', [[], ['--light-model'], ['--image-scale', '0.5']], ids=['plain', 'light-model', 'image-scale'])
def test_cli_kept_matches_hold_the_survivors(disk_scene, tmp_path, capsys, extra):
    """With --keep-matches the kept file holds the observations that survived the trim, and a plain run on that file restores
    the image of the trimmed run -- within the bars test_cli_kept_matches_are_reused_in_every_mode holds "matched run vs run on
    its kept file" to (the second run rebuilds the camera points on the host)."""
    from sucre_amd import h5bridge, sucre
    root, scene, loaded = disk_scene
    name = scene.names[scene.target]
    first, again = tmp_path / 'first', tmp_path / 'again'
    out, t, stem = _trim_run(root, first, name, capsys, '--keep-matches', '--save-quality', *extra)
    assert 'Compute' in out and 'survived the trim' in out
    D = int(t['view_dropped'].sum())
    assert D > 0
    kept = [f for f in first.iterdir() if f.suffix in ('.h5', '.npz')]
    assert len(kept) == 1
    groups = h5bridge.read_groups(kept[0]) if kept[0].suffix == '.h5' else h5bridge.read_npz_groups(kept[0])
    assert sum(len(g['u1']) for g in groups.values()) == int(t['n_obs'][0]) - D
    q = torch.load(first / f'{stem}_quality.pt')            # the views kept at the end, and what each of them still holds
    assert {v: int(n) for v, k, n in zip(q['views'], q['view_kept'].tolist(), q['view_n']) if k} == {v: len(g['u1']) for v, g in groups.items()}
    again.mkdir()
    shutil.copy(kept[0], again / kept[0].name)
    sucre.main(_base(root) + ['--output-dir', str(again), '--image-name', name, '--keep-matches'] + extra)
    txt = capsys.readouterr().out
    assert 'Compute' not in txt and 'is not reused' not in txt and f'Total of {int(t["n_obs"][0]) - D} observations' in txt
    assert not (again / f'{stem}_trim.pt').exists()
    a, b = torch.load(first / f'{stem}.pt'), torch.load(again / f'{stem}.pt')
    assert set(a) == set(b)
    assert np.array_equal(np.isnan(a['J'].numpy()), np.isnan(b['J'].numpy()))
    light = '--light-model' in extra
    assert helpers.rms_per_channel(b['J'].numpy(), a['J'].numpy()).max() < (3e-5 if light else 1e-6)
    for k in a:
        if k != 'J':
            assert torch.allclose(a[k], b[k], atol=(2e-3 if k in ('cam2light', 'sigma') else 1e-4) if light else 2e-6), k


def test_adam_trims_a_list_backed_matches_data(tmp_path):
    """sucre.adam(..., trim_outliers=3.0) on the container test_reference_call_sequence_with_hand_built_matches_data builds (matches
    appended view by view, load_matches -> lists), on the planted scene: the engine path on the same lists, bit for bit."""
    from sucre_amd import loader, sucre
    from test_gpu_api import SynthImage
    sc, _ = scene_of('planted75')
    images = [SynthImage(i + 1, v, sc.K, sc.width, sc.height) for i, v in enumerate(sc.views)]
    target = images[sc.target]
    matches_file = loader.MatchesFile(tmp_path / 'm.h5', colmap_model=None)
    u1, v1, wP1 = target.unproject_depth_map(target.get_depth_map().cuda(), to_world=True)
    for other in images:
        other_depth = other.get_depth_map().cuda()
        u2, v2, wP2 = other.unproject_depth_map(other_depth, to_world=True)
        m = target.match_two_way(other, u1=u1, v1=v1, wP1=wP1, u2=u2, v2=v2, wP2=wP2)
        if len(m) / (sc.width * sc.height) > 1e-6:
            matches_file.save_matches(matches=m, d=other_depth[m.v2, m.u2])
    matches_file.prepare_matches()
    matches_file.check_integrity()
    md = matches_file.load_matches()
    assert md.restoration is None and len(md.data) == sum(len(o[0]) > 0 for o in scene_of('planted75')[1]) >= 2
    T = 10
    model = sucre.SUCRe(image=target).to('cuda')
    J0, params0 = model.J.detach().clone(), model.water_vector().detach().cpu().numpy()
    # the engine path first, on the lists MatchesData.to_engine makes of the container (uint8 colours: they are k/255)
    lists = []
    for s in md.data:
        cP = s.cP.to(torch.float32)
        z = torch.sqrt((cP[0] * cP[0] + cP[1] * cP[1]) + cP[2] * cP[2])
        lists.append((s.u, s.v, z, (s.I.to(torch.float64) * 255).round().to(torch.uint8).T.contiguous()))
    view = target.device_view(torch.device(DEV))
    r = engine.Restoration(sc.height, sc.width, len(lists), device=DEV)
    r.import_matches(None, lists)
    r.fit_init(view, params0=params0, J0=J0)
    r.fit(T)
    _, view_dropped, _ = r.trim_outliers(3.0)
    r.fit_init(view, params0=params0, J0=J0)
    r.fit(T)
    sucre.adam(sucre=model, matches_data=md, lr=0.05, num_iter=T, batch_size=5, device='cuda', verbose=False,
               trim_outliers=3.0, trim_rounds=1)
    assert md.restoration is not None and md.restoration is not r
    assert len(model._trim) == 1 and int(model._trim[0]['view_dropped'].sum()) > 0
    assert _same_bits(model._trim[0]['view_dropped'], view_dropped)
    assert _same_bits(model.J.detach(), r.J())
    assert _same_bits(model.water_vector().detach().cpu(), r.params().cpu().clone())
