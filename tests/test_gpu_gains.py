"""GPU tests of the per-view gain compensation (sucre_view_gains*, sucre_apply_view_gains*, engine.Restoration.view_gains /
apply_view_gains, --view-gains): the estimate against a float64 restatement in every variant of the kernel, the rules, the apply
rule bit for bit, the refit as a plain run on the corrected store, the repair of a scene with two mis-exposed views, the CLI.

The reference for the sums is computed HERE, in float64 numpy, from the oracle's match lists: sucre.py:52-64 (l, z) and
sucre.py:79-82 (forward), evaluated at the engine's own float32 J() and params() cast to float64 (test_gains_host.gain_sums).

Bars, derived as test_gpu_residuals.bar is: an error delta in each modelled intensity Ihat moves sum I Ihat by at most
delta sum |I| and sum Ihat^2 by at most 2 delta sum |Ihat| + n delta^2; 1e-5 S covers the float32 accumulation of a tile and view.
delta = 1e-6 for the plain model, 2e-6 with the light model, for the reasons stated there.  The observation counts are exact.
"""
import copy
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from oracle import oracle
from sucre_amd import engine, synth
from test_gains_host import apply_f32, apply_u8, gain_sums, gains_from_sums

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
G_TRUE = {0: (0.80, 0.80, 0.80), 4: (1.25, 1.15, 1.05)}


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def with_gains(scene, gains=G_TRUE):
    """The scene with the colour images of the views in ``gains`` multiplied per channel, rounded and clamped to uint8."""
    bad = copy.copy(scene)
    bad.views = list(scene.views)
    for k, g in gains.items():
        v = copy.copy(scene.views[k])
        v.rgb_u8 = torch.tensor(np.clip(np.rint(v.rgb_u8.numpy().astype(np.float64) * np.asarray(g)), 0, 255).astype(np.uint8))
        bad.views[k] = v
    return bad


def float_images(scene, seed=75):
    """Per view a float32 (H,W,3) colour image that is NOT k/255 (a kernel that rounded a colour through uint8 would show)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for v in scene.views:
        f = (v.rgb_u8.to(torch.float64) / 255).to(torch.float32)
        out.append((f + (torch.rand(f.shape, generator=gen) - 0.5) * 0.003).clamp(0, 1).contiguous())
    return out


def device_views(scene, frgb=None):
    if frgb is None:
        return engine.device_views_from_scene(scene, DEV)
    return [engine.DeviceView(depth=v.depth_f32().to(DEV).contiguous(), rgb=f.to(DEV), K=scene.K, R=v.R, t=v.t, name=v.name)
            for v, f in zip(scene.views, frgb)]


def scene_observations(scene, frgb=None):
    """Per view, in engine order (= scene order), from the oracle: dict(cover, u1, v1, cP (3,n) float32, z (n,) float32 = ||cP||
    as the store holds it, rgb (n,3) uint8, I (n,3) float32 = rgb / 255 or, with ``frgb``, those float32 images' pixels)."""
    per_view, _ = helpers.oracle_scene_samples(scene)
    obs = []
    for k, ((name, _, m), view) in enumerate(zip(per_view, scene.views)):
        cP = oracle.unproject(helpers.oracle_cam(scene, view), m.u2, m.v2, m.d)
        u2, v2 = m.u2.astype(np.int64), m.v2.astype(np.int64)
        rgb = view.rgb_u8.numpy()[v2, u2]
        I = oracle.gather_rgb(view.rgb_u8.numpy(), m.u2, m.v2).T if frgb is None else frgb[k].numpy()[v2, u2]
        obs.append(dict(cover=len(m) / (scene.width * scene.height), u1=m.u1.astype(np.int64), v1=m.v1.astype(np.int64), cP=cP,
                        z=np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2]), rgb=rgb, I=np.ascontiguousarray(I, np.float32)))
    return obs


_SCENES = {}


def scene_of(key):
    """(scene, observations), made once per module run and never changed."""
    if key not in _SCENES:
        if key == 'clean75':      # 5x4 tiles, partial in both directions; 7 views, the target is view 3; view 5 (far) sees nothing
            scene = synth.make_scene(75, 52, 5, seed=11, far_views=1)
        elif key == 'bad75':      # views 0 and 4 mis-exposed
            scene = with_gains(scene_of('clean75')[0])
        elif key == 'views71':    # per-pixel counts above one 64-bit mask word
            scene = synth.make_scene(48, 32, 70, seed=3)
        elif key == 'tiles272':   # 17 x 16 = 272 tiles: the view sums' threads go round twice
            scene = synth.make_scene(272, 250, 3, seed=4)
        _SCENES[key] = (scene, scene_observations(scene))
    return _SCENES[key]


_FLOAT = {}


def float_scene_of(key):
    if key not in _FLOAT:
        scene, _ = scene_of(key)
        frgb = float_images(scene)
        _FLOAT[key] = (scene, scene_observations(scene, frgb), frgb)
    return _FLOAT[key]


def fitted(scene, T, min_cover=1e-6, closed=False, frgb=None, float_views=False, **kw):
    views = device_views(scene, frgb)
    if float_views:
        views = [v.as_float_colour() for v in views]
    r = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
    r.match(views[scene.target], views, min_cover=min_cover)
    r.fit_init(views[scene.target])
    r.trace_first = r.fit(T, use_closed_form=closed)
    return r, views


# ---- the float64 reference ------------------------------------------------------------------------------------------------
def reference_table(obs, J, params, min_cover=1e-6, u16mm=False, light=False):
    """(sums (n_views,7), sum |I| (n_views,3), sum |Ihat| (n_views,3), kept) in float64 at J, params."""
    J64, p = J.astype(np.float64), params.astype(np.float64)
    B, beta, gamma = p[0:3], p[3:6], p[6:9]
    n = len(obs)
    sums, sI, sH, kept = np.zeros((n, 7)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, bool)
    if light:   # sucre.py:54-61 with se3.exp (se3.py:22-27), float64
        from sucre_amd import se3
        R, t = [x.numpy() for x in se3.exp(torch.tensor(p[9:15], dtype=torch.float64))]
        sigma = p[15:19].reshape(2, 2)
        Minv = np.linalg.inv(sigma.T @ sigma)
    for k, o in enumerate(obs):
        kept[k] = o['cover'] > min_cover          # sfm.py:136
        if not kept[k]:
            continue
        z32 = o['z']
        if u16mm:   # what the fit of a u16mm store reads
            z32 = np.clip(np.rint(z32 * np.float32(1000.0)), np.float32(1.0), np.float32(65535.0)) * np.float32(0.001)
        assert z32.dtype == np.float32
        z, l = z32.astype(np.float64), 1.0
        if light:
            lP = R @ o['cP'].astype(np.float64) + t
            lp = lP[:2] / lP[2]
            l = np.exp(-(lp * (Minv @ lp)).sum(axis=0) / 2)[:, None]
            z = z + np.linalg.norm(lP, axis=0)
        z = z[:, None]
        Ihat = l * (J64[o['v1'], o['u1']] * np.exp(-beta * z) + B * (1 - np.exp(-gamma * z)))   # sucre.py:79-82
        sums[k] = gain_sums(o['I'], Ihat)
        ok = np.isfinite(Ihat)
        sI[k] = np.where(ok, np.abs(o['I'].astype(np.float64)), 0.0).sum(axis=0)
        sH[k] = np.where(ok, np.abs(Ihat), 0.0).sum(axis=0)
    return sums, sI, sH, kept


def check_estimate(label, r, obs, min_cover=1e-6, u16mm=False, light=False, limit=2.0):
    delta = 2e-6 if light else 1e-6
    gains, inv, sums = [t.cpu().numpy() for t in r.view_gains(limit)]
    n = r.n_views
    assert gains.dtype == np.float64 and gains.shape == (n, 3) and inv.dtype == np.float32 and inv.shape == (n, 3)
    assert sums.dtype == np.float64 and sums.shape == (n, 7)
    ref, sI, sH, kept = reference_table(obs, r.J().cpu().numpy(), r.params().cpu().numpy(), min_cover, u16mm, light)
    assert np.array_equal(r.view_keep().cpu().numpy() != 0, kept), label
    assert np.array_equal(sums[:, 0], ref[:, 0]), (label, 'observations per view')
    assert np.all(sums[~kept] == 0) and np.isfinite(sums).all(), (label, 'zeros where nothing is kept')
    cnt = ref[:, :1]
    bar_ih = delta * sI + 1e-5 * np.abs(ref[:, 1:4])
    bar_hh = 2 * delta * sH + cnt * delta ** 2 + 1e-5 * ref[:, 4:7]
    d_ih = np.abs(sums[:, 1:4] - ref[:, 1:4]) / np.maximum(bar_ih, 1e-300)
    d_hh = np.abs(sums[:, 4:7] - ref[:, 4:7]) / np.maximum(bar_hh, 1e-300)
    d_ih[~kept] = 0.0; d_hh[~kept] = 0.0
    print(f'{label}: worst |d|/bar S_IIhat {d_ih.max():.3f}, S_IhatIhat {d_hh.max():.3f} ({int(cnt.sum())} observations in {int(kept.sum())} views)')
    assert d_ih.max() <= 1.0, (label, 'S_IIhat', d_ih.max())
    assert d_hh.max() <= 1.0, (label, 'S_IhatIhat', d_hh.max())
    # the gains are the stated function of the device's own sums, to the bit
    g_ref, inv_ref = gains_from_sums(sums, kept, limit)
    assert np.array_equal(gains, g_ref) and np.array_equal(inv, inv_ref), label
    return gains, inv, sums, kept


# ---- 1. the estimate against float64 --------------------------------------------------------------------------------------
def test_estimate_plain_excludes_views_below_min_cover():
    scene, obs = scene_of('clean75')
    r, _ = fitted(scene, 20, min_cover=0.7)
    gains, inv, sums, kept = check_estimate('plain 75x52 min_cover 0.7', r, obs, min_cover=0.7)
    assert kept.tolist() == [True, False, True, True, True, False, True]
    assert r.view_counts().cpu().numpy()[1] > 0          # view 1 has chunks in the dense store, but is not kept
    assert np.all(gains[~kept] == 1.0) and np.all(inv[~kept] == 1.0)
    assert not np.any(gains[kept] == 1.0)                # estimated, not defaulted


@pytest.mark.parametrize('case', ['u16mm', 'closed', 'float', 'light', 'light-float'])
def test_estimate_variants(case):
    scene, obs = scene_of('bad75')
    kw = {'u16mm': dict(obs_format='u16mm'), 'float': dict(float_views=True, float_colour=True), 'light': dict(light=True),
          'light-float': dict(float_views=True, light=True, float_colour=True)}.get(case, {})
    r, _ = fitted(scene, 10, closed=case == 'closed', **kw)
    check_estimate(case, r, obs, u16mm=case == 'u16mm', light=case.startswith('light'))


def test_estimate_float_colours_off_the_grid():
    scene, obs, frgb = float_scene_of('bad75')
    r, _ = fitted(scene, 10, frgb=frgb, float_colour=True)
    check_estimate('float colours off the 1/255 grid', r, obs)


def test_estimate_imported_store():
    scene, obs = scene_of('bad75')
    views = device_views(scene)
    r = engine.Restoration(scene.height, scene.width, len(obs), device=DEV)
    r.import_matches(views[scene.target], lists_of(obs), min_cover=1e-6)
    r.fit_init(views[scene.target])
    r.fit(10)
    check_estimate('imported lists', r, obs)


def test_estimate_71_views():
    scene, obs = scene_of('views71')
    r, _ = fitted(scene, 5)
    _, _, sums, kept = check_estimate('plain 48x32 x 71 views', r, obs)
    assert kept.all() and r.residuals()[0].max() > 64


def test_estimate_more_tiles_than_threads_of_the_view_sums():
    scene, obs = scene_of('tiles272')
    assert (scene.width + 15) // 16 * ((scene.height + 15) // 16) == 272
    r, _ = fitted(scene, 5)
    _, _, _, kept = check_estimate('plain 272x250 x 4 views, 272 tiles', r, obs)
    assert kept.all()


# ---- 2. the rules ---------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8))


def test_limit_clamps():
    scene, obs = scene_of('bad75')
    r, _ = fitted(scene, 20)
    free = check_estimate('limit 2', r, obs)[0]
    tight = check_estimate('limit 1.1', r, obs, limit=1.1)[0]
    assert np.all(free[0] < 1 / 1.1) and free[4, 0] > 1.1          # the two mis-exposed views lie outside the tight limit
    assert np.all(tight[0] == 1 / 1.1) and tight[4, 0] == 1.1
    assert tight.min() >= 1 / 1.1 and tight.max() <= 1.1
    inside = (free >= 1 / 1.1) & (free <= 1.1)
    assert np.array_equal(tight[inside], free[inside])
    with pytest.raises(ValueError, match='limit'):
        r.view_gains(0.5)


@pytest.mark.parametrize('kw', [dict(), dict(light=True), dict(float_views=True, float_colour=True)], ids=['plain', 'light', 'float'])
def test_pure_read_and_reproducible(kw):
    scene, _ = scene_of('bad75')
    a, _ = fitted(scene, 10, **kw)
    ws, lws = a.ws.clone(), None if a.lws is None else a.lws.clone()
    first = a.view_gains()
    second = a.view_gains()
    for x, y in zip(first, second):
        assert _same_bits(x, y)
    assert torch.equal(a.ws, ws) and (lws is None or torch.equal(a.lws, lws))
    assert a.steps_done == 10


# ---- 3. the apply is bit-exact --------------------------------------------------------------------------------------------
# 1.0; 0.5, 1.5 and 2.5 put odd bytes on ties; 6.0 clips every byte from 43 on (the scene's reds are 16 .. 46), 2.0 every byte from
# 128 on (its blues are 66 .. 183); view 1 is not kept and view 5 holds nothing
INV = np.array([[1.0, 0.5, 1.5], [3.0, 3.0, 3.0], [6.0, 0.75, 1.0], [1.0, 1.0, 1.0], [1.25, 0.8, 2.0], [2.0, 2.0, 2.0],
                [0.5, 2.5, 1.1]], np.float32)


def test_apply_uint8_is_the_numpy_rule():
    scene, obs = scene_of('clean75')
    r, views = fitted(scene, 5, min_cover=0.7)
    before = [tuple(t.cpu().numpy() for t in r.export_view(k)) for k in range(r.n_views)]
    counts, keep, n_obs = r.view_counts().clone(), r.view_keep().clone(), r.n_obs()
    kept = keep.cpu().numpy() != 0
    assert kept.tolist() == [True, False, True, True, True, False, True]
    clipped = r.apply_view_gains(torch.tensor(INV, device=DEV)).cpu().numpy()
    assert r.steps_done == 0 and clipped.dtype == np.int64
    assert _same_bits(r.view_counts(), counts) and _same_bits(r.view_keep(), keep) and r.n_obs() == n_obs
    ties = 0
    for k in range(r.n_views):
        z0, rgb0 = before[k]
        z1, rgb1 = [t.cpu().numpy() for t in r.export_view(k)]
        assert np.array_equal(z0.view(np.uint32), z1.view(np.uint32)), (k, 'ranges')
        assert np.array_equal((z0 > 0).sum(), len(obs[k]['u1']))
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
    assert 0 < clipped[2] < (before[2][0] > 0).sum() and clipped[4] > 0 and clipped[3] == 0 and ties > 100
    # the fit reads the corrected store: the refit differs from the first fit
    r.fit_init(views[scene.target])
    assert not _same_bits(r.fit(5), r.trace_first)


def test_apply_float_colours_is_one_multiply():
    scene, obs, frgb = float_scene_of('clean75')
    r, _ = fitted(scene, 5, min_cover=0.7, frgb=frgb, float_colour=True)
    before = [(r.export_view(k)[0].cpu().numpy(), r.export_view_ext(k).cpu().numpy()) for k in range(r.n_views)]
    kept = r.view_keep().cpu().numpy() != 0
    clipped = r.apply_view_gains(torch.tensor(INV, device=DEV)).cpu().numpy()
    assert np.all(clipped == 0)
    top = 0.0
    for k in range(r.n_views):
        z0, I0 = before[k]
        z1, I1 = r.export_view(k)[0].cpu().numpy(), r.export_view_ext(k).cpu().numpy()
        top = max(top, float(I1.max()))
        assert np.array_equal(z0.view(np.uint32), z1.view(np.uint32)), (k, 'ranges')
        at = z0 > 0
        want = apply_f32(I0[:, at].T, INV[k] if kept[k] else np.ones(3, np.float32)).T
        assert np.array_equal(I1[:, at].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (k, 'colours')
        assert np.array_equal(I1[:, ~at].view(np.uint32), I0[:, ~at].view(np.uint32)), (k, 'empty slots')
        if kept[k] and at.any():   # the store held the pictures' own float32 pixels
            o = obs[k]
            assert np.array_equal(I0[:, o['v1'], o['u1']].T, o['I'])
    assert top > 1.0      # no clamp


@pytest.mark.parametrize('kw', [dict(), dict(obs_format='u16mm'), dict(light=True), dict(float_views=True, float_colour=True),
                                dict(float_views=True, light=True, float_colour=True)], ids=['plain', 'u16mm', 'light', 'float', 'light-float'])
def test_apply_of_ones_leaves_every_byte(kw):
    scene, _ = scene_of('bad75')
    r, _ = fitted(scene, 5, **kw)
    ws, lws = r.ws.clone(), None if r.lws is None else r.lws.clone()
    clipped = r.apply_view_gains(torch.ones((r.n_views, 3), dtype=torch.float32, device=DEV))
    assert int(clipped.sum()) == 0
    assert torch.equal(r.ws, ws) and (lws is None or torch.equal(r.lws, lws))


# ---- 4. the refit is a plain run on the corrected store -------------------------------------------------------------------
def lists_of(obs, inv=None, float_colour=False):
    """What import_matches takes, from the oracle's lists; with ``inv`` the colours go through the numpy rule first."""
    lists = []
    for k, o in enumerate(obs):
        item = [torch.tensor(o['u1'], dtype=torch.int16), torch.tensor(o['v1'], dtype=torch.int16), torch.tensor(o['z'])]
        if float_colour:
            I = o['I'] if inv is None else apply_f32(o['I'], inv[k])
            item += [None, torch.tensor(np.ascontiguousarray(I.T))]
        else:
            item += [torch.tensor(o['rgb'] if inv is None else apply_u8(o['rgb'], inv[k])[0])]
        lists.append(tuple(item))
    return lists


@pytest.mark.parametrize('case', ['plain', 'float'])
def test_refit_equals_a_plain_run_on_the_corrected_colours(case):
    T = 20
    if case == 'float':
        scene, obs, frgb = float_scene_of('bad75')
        kw = dict(float_colour=True)
    else:
        (scene, obs), frgb, kw = scene_of('bad75'), None, {}
    a, views = fitted(scene, T, frgb=frgb, **kw)
    target = views[scene.target]
    _, inv, _ = a.view_gains()
    inv_host = inv.cpu().numpy()
    assert np.all(inv_host[0] > 1.1) and inv_host[4, 0] < 0.9
    a.apply_view_gains(inv)
    a.fit_init(target)
    ta = a.fit(T)
    kept = a.view_keep().cpu().numpy() != 0
    b = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
    b.import_matches(target, lists_of(obs, np.where(kept[:, None], inv_host, np.float32(1.0)), float_colour=case == 'float'), min_cover=1e-6)
    b.fit_init(target)
    tb = b.fit(T)
    for name, x, y in (('J', a.J(), b.J()), ('params', a.params(), b.params()), ('trace', ta, tb),
                       ('view_counts', a.view_counts(), b.view_counts()), ('view_keep', a.view_keep(), b.view_keep())):
        assert _same_bits(x, y), (case, name)
    assert a.n_obs() == b.n_obs() > 0 and bool(torch.isfinite(ta).all())
    assert not _same_bits(ta, a.trace_first)


# ---- 5. it repairs the scene ----------------------------------------------------------------------------------------------
def _scaled_rms(J, Jc):
    ok = np.isfinite(J).all(-1) & np.isfinite(Jc).all(-1)
    a, b = J[ok].astype(np.float64), Jc[ok].astype(np.float64)
    sc = (a * b).sum(0) / (a * a).sum(0)
    return np.sqrt(((a * sc - b) ** 2).mean(0))


def test_repairs_a_scene_with_two_misexposed_views():
    """Views 0 and 4 of the 75x52 scene are mis-exposed by G_TRUE.  The figures in brackets are what the float64 CPU oracle
    procedure (fit, g = sum I Ihat / sum Ihat^2, uint8 correction, refit) achieves on exactly these inputs."""
    T = 60
    clean, _ = scene_of('clean75')
    scene, obs = scene_of('bad75')
    Jc = fitted(clean, T)[0].J().cpu().numpy()
    r, views = fitted(scene, T)
    cost_plain = float(r.trace_first[-1, 0].cpu())
    rms_plain = _scaled_rms(r.J().cpu().numpy(), Jc)
    gains, inv, sums, kept = check_estimate('perturbed scene, 60 iterations', r, obs)     # within the bar of the float64 procedure
    r.apply_view_gains(torch.tensor(inv, device=DEV))
    r.fit_init(views[scene.target])
    cost_refit = float(r.fit(T)[-1, 0].cpu())
    rms_refit = _scaled_rms(r.J().cpu().numpy(), Jc)
    rel = gains / gains[scene.target]
    truth = np.ones((len(obs), 3))
    for k, g in G_TRUE.items():
        truth[k] = g
    left = {k: float(np.abs(rel[k] - truth[k]).max() / np.abs(truth[k] - 1).max()) for k in G_TRUE}
    untouched = [k for k in range(len(obs)) if kept[k] and k not in G_TRUE]
    off = float(np.abs(rel[untouched] - 1).max())
    print(f'gains / target: view 0 {rel[0]}, view 4 {rel[4]}; leftover fraction {left} (oracle 0.101); untouched views off by {off:.4f} '
          f'(oracle 0.014); cost {cost_plain:.4g} -> {cost_refit:.4g}, {cost_plain / cost_refit:.1f}x (oracle 39x); RMS(J) {rms_plain} -> '
          f'{rms_refit}, {rms_plain / rms_refit} x (oracle 5x, 10x, 7x)')
    assert scene.target == 3 and kept.tolist() == [True, True, True, True, True, False, True]
    assert max(left.values()) <= 0.25                      # (a)
    assert off <= 0.03                                     # (b)
    assert cost_refit * 10 <= cost_plain                   # (c)
    assert np.all(rms_refit * 2 <= rms_plain)              # (d)


# ---- 6. the command line --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disk_scene(tmp_path_factory):
    from test_gpu_api import scene_as_loaded, write_scene
    from sucre_amd import sfm
    root = tmp_path_factory.mktemp('gain_scene')
    scene = synth.make_scene(96, 64, 4, seed=21, far_views=1)
    scaled = 0 if scene.target != 0 else 1
    bad = with_gains(scene, {scaled: (0.8, 0.8, 0.8)})
    write_scene(bad, root)
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    return root, bad, scene_as_loaded(bad, model), scaled


CLI_ITER = 30


def _base(root):
    return ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'), '--num-iter', str(CLI_ITER)]


def _api_rounds(root, name, out_dir, rounds):
    """The API sequence the flag stands for: the command line's own start (model, matches, initial values), then the engine calls."""
    from sucre_amd import sfm, sucre
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    out_dir.mkdir(parents=True, exist_ok=True)
    job = sucre._restore_submit(model[name], model, out_dir, False, False, 0.000001, list(model.images.values()), 0.05, CLI_ITER, None,
                                False, 0, DEV)
    resto = sucre._adam_begin(job.sucre, job.matches_data)
    resto.fit(CLI_ITER)
    records = []
    for _ in range(rounds):
        gains, inv, sums = resto.view_gains(2.0)
        records.append((gains.cpu(), sums.cpu(), resto.apply_view_gains(inv).cpu()))
        sucre._adam_begin(job.sucre, job.matches_data)
        resto.fit(CLI_ITER)
    sucre._pull_results(job.sucre, resto)
    return job, records


def test_cli_view_gains_files(disk_scene, tmp_path, capsys):
    from sucre_amd import sucre
    root, scene, loaded, scaled = disk_scene
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'off'), '--image-name', name])
    assert not list((tmp_path / 'off').glob('*_gains.pt'))
    capsys.readouterr()
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'on'), '--image-name', name, '--view-gains', '--save-quality'])
    out = capsys.readouterr().out
    g = torch.load(tmp_path / 'on' / f'{stem}_gains.pt')
    assert set(g) == {'views', 'gains', 'sums', 'view_clipped', 'view_kept', 'gain', 'limit'}
    n = len(g['views'])
    assert g['limit'] == 2.0 and all(isinstance(v, str) for v in g['views']) and set(g['views']) <= set(scene.names)
    assert g['gains'].dtype == torch.float64 and g['gains'].shape == (1, n, 3)
    assert g['sums'].dtype == torch.float64 and g['sums'].shape == (1, n, 7)
    assert g['view_clipped'].dtype == torch.int64 and g['view_clipped'].shape == (1, n)
    assert g['view_kept'].dtype == torch.bool and g['view_kept'].shape == (1, n)
    assert g['gain'].dtype == torch.float64 and g['gain'].shape == (n, 3)
    k = g['views'].index(scene.names[scaled])
    assert torch.all(g['gain'][k] < 0.9)
    assert f'{name}: gain round 1: largest correction in view {scene.names[scaled]} (gain R ' in out
    # --save-quality describes the final fit
    q = torch.load(tmp_path / 'on' / f'{stem}_quality.pt')
    assert int(q['count'].sum()) == int(g['sums'][0, :, 0].sum())
    # the API sequence gives the same bits
    job, records = _api_rounds(root, name, tmp_path / 'api', 1)
    assert _same_bits(g['gain'], records[0][0]) and _same_bits(g['sums'][0], records[0][1]) and _same_bits(g['view_clipped'][0], records[0][2])
    got = torch.load(tmp_path / 'on' / f'{stem}.pt')
    assert _same_bits(got['J'], job.sucre.J.detach().cpu())
    for key in ('B', 'beta', 'gamma'):
        assert _same_bits(got[key], getattr(job.sucre, key).detach().cpu()), key
    sucre._save_png(job.sucre.plot_J(), tmp_path / 'api' / 'rgb.png')
    assert (tmp_path / 'on' / f'{stem}_rgb.png').read_bytes() == (tmp_path / 'api' / 'rgb.png').read_bytes()
    off = torch.load(tmp_path / 'off' / f'{stem}.pt')
    assert not torch.equal(torch.nan_to_num(off['J'], nan=-7.0), torch.nan_to_num(got['J'], nan=-7.0))


def test_cli_two_rounds(disk_scene, tmp_path):
    from sucre_amd import sucre
    root, scene, loaded, scaled = disk_scene
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'two'), '--image-name', name, '--view-gains', '--gain-rounds', '2',
                              '--gain-limit', '1.5'])
    g = torch.load(tmp_path / 'two' / f'{stem}_gains.pt')
    n = len(g['views'])
    assert g['limit'] == 1.5 and g['gains'].shape == (2, n, 3) and g['sums'].shape == (2, n, 7) and g['view_clipped'].shape == (2, n)
    assert _same_bits(g['gain'], g['gains'][0] * g['gains'][1])
    k = g['views'].index(scene.names[scaled])
    assert float((g['gains'][1][k] - 1).abs().max()) < float((g['gains'][0][k] - 1).abs().max())     # the second round has less to do


@pytest.mark.parametrize('fit_batch', ['1', 'auto'], ids=['two-in-flight', 'one-launch-per-iteration'])
def test_cli_survey_equals_single_runs(disk_scene, tmp_path, monkeypatch, fit_batch):
    from sucre_amd import sucre
    root, scene, loaded, scaled = disk_scene
    monkeypatch.setenv('SUCRE_IMAGES_IN_FLIGHT', '2')
    monkeypatch.setenv('SUCRE_FIT_BATCH', fit_batch)
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'survey'), '--image-ids', '1', '4', '--view-gains'])
    got = sorted((tmp_path / 'survey').glob('*_gains.pt'))
    assert len(got) == 3
    for p in got:
        stem = p.name[:-len('_gains.pt')]
        sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'single'), '--image-name', f'{stem}.png', '--view-gains'])
        a, b = torch.load(p), torch.load(tmp_path / 'single' / p.name)
        assert a['views'] == b['views'] and a['limit'] == b['limit']
        for k in ('gains', 'sums', 'view_clipped', 'view_kept', 'gain'):
            assert _same_bits(a[k], b[k]), (p.name, k)
        a, b = torch.load(tmp_path / 'survey' / f'{stem}.pt'), torch.load(tmp_path / 'single' / f'{stem}.pt')
        for k in a:
            assert _same_bits(a[k], b[k]), (stem, k)
        assert (tmp_path / 'survey' / f'{stem}_rgb.png').read_bytes() == (tmp_path / 'single' / f'{stem}_rgb.png').read_bytes()
