"""GPU tests of the outlier-trimmed refit (sucre_trim_outliers*, engine.Restoration.trim_outliers, --trim-outliers).

The float64 reference of a decision is computed HERE: the model of the residual tests (sucre.py:52-64 for l and z, sucre.py:79-82
for the forward pass, sucre.py:144 for the residual) on the oracle's match lists, evaluated at the engine's own float32 J() and
params() read before the trim and cast to float64.

Bars.  A threshold tau^2_c = k^2 S_c / N inherits the residual tests' bar on a sum of n squared residuals,
|d| <= 2 delta sqrt(n S) + n delta^2 + 1e-5 S (delta = 1e-6, 2e-6 with the light model: test_gpu_residuals.py), times k^2 / N,
plus one float32 rounding.  An observation is UNDECIDED when, in any channel, |r^2 - tau^2| <= 2 delta sqrt(tau^2) + delta^2 +
2^-21 tau^2: an error delta in the modelled intensity moves r^2 near the threshold by 2 |r| delta + delta^2, and the float32
product r r and the comparison's operands carry a few units of 2^-24.  A pixel holding an undecided observation is undecided
(its guard may go either way); everywhere else the engine's set of zeroed ranges must be exactly the reference's.  At most
max(2, 1e-4 N) observations may be undecided -- a condition on the case, checked on the reference alone.

"Planted": a 12 x 14 patch of view 0 recoloured by (+90, -60, +70), the fish in one neighbour view the feature is for.
"""
import copy
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from oracle import oracle
from sucre_amd import engine, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
K_SIGMA = 3.0
PATCH = (slice(13, 27), slice(19, 31))      # rows, columns of view 0 of the 75 x 52 scene: 14 x 12 pixels, 161 of them matched
PATCH_71, PATCH_272 = (slice(9, 23), slice(18, 30)), (slice(100, 114), slice(120, 132))   # the same in the two other scenes
CAST = (90, -60, 70)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def plant(scene, patch=PATCH, view=0):
    bad = copy.copy(scene)
    bad.views = list(scene.views)
    v = copy.copy(scene.views[view])
    rgb = v.rgb_u8.clone().to(torch.int32)
    rgb[patch[0], patch[1]] += torch.tensor(CAST, dtype=torch.int32)
    v.rgb_u8 = rgb.clamp(0, 255).to(torch.uint8)
    bad.views[view] = v
    return bad


def float_images(scene, seed=75):
    """Per view a float32 (H,W,3) colour image that is NOT k/255: float32(u8 / 255) + (rand - 0.5) 0.003, clamped to [0, 1] (what
    tools/parity_sweep.py feeds its float-colour stores).  A kernel that rounded a colour through uint8 is off by up to 1.5e-3."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for v in scene.views:
        f = (v.rgb_u8.to(torch.float64) / 255).to(torch.float32)
        out.append((f + (torch.rand(f.shape, generator=gen) - 0.5) * 0.003).clamp(0, 1).contiguous())
    return out


def device_views(scene, frgb=None):
    """The scene's views on the device: uint8 colours as stored, or the float32 images ``frgb`` in their place."""
    if frgb is None:
        return engine.device_views_from_scene(scene, DEV)
    return [engine.DeviceView(depth=v.depth_f32().to(DEV).contiguous(), rgb=f.to(DEV), K=scene.K, R=v.R, t=v.t, name=v.name)
            for v, f in zip(scene.views, frgb)]


def scene_observations(scene, frgb=None):
    """Per view, in engine order (= scene order): (u1, v1, cP (3,n) float32, I (3,n) float32, u2, v2) from the oracle.  With
    ``frgb`` the colours are gathered from those float32 images, I = frgb[view][v2, u2] (copies: bit-exact)."""
    per_view, _ = helpers.oracle_scene_samples(scene)
    obs = []
    for k, ((name, _, m), view) in enumerate(zip(per_view, scene.views)):
        cP = oracle.unproject(helpers.oracle_cam(scene, view), m.u2, m.v2, m.d)
        u2, v2 = m.u2.astype(np.int64), m.v2.astype(np.int64)
        I = oracle.gather_rgb(view.rgb_u8.numpy(), m.u2, m.v2) if frgb is None else np.ascontiguousarray(frgb[k].numpy()[v2, u2].T)
        obs.append((m.u1.astype(np.int64), m.v1.astype(np.int64), cP, I, u2, v2))
    return obs


_SCENES = {}


def scene_of(key):
    """(scene, observations), made once per module run and never changed."""
    if key not in _SCENES:
        if key == 'clean75':
            scene = synth.make_scene(75, 52, 5, seed=11, far_views=1)
        elif key == 'planted75':
            scene = plant(scene_of('clean75')[0])
        elif key == 'views71':
            scene = plant(synth.make_scene(48, 32, 70, seed=3), PATCH_71)
        elif key == 'tiles272':
            scene = plant(synth.make_scene(272, 250, 3, seed=4), PATCH_272)
        _SCENES[key] = (scene, scene_observations(scene))
    return _SCENES[key]


_FLOAT_SCENES = {}


def float_scene_of(key):
    """(scene, observations, float32 images) of ``scene_of(key)``'s scene with colours off the 1/255 grid, made once."""
    if key not in _FLOAT_SCENES:
        scene, _ = scene_of(key)
        frgb = float_images(scene)
        _FLOAT_SCENES[key] = (scene, scene_observations(scene, frgb), frgb)
    return _FLOAT_SCENES[key]


def fitted(scene, T, min_cover=1e-6, closed=False, frgb=None, **kw):
    views = device_views(scene, frgb)
    r = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
    r.match(views[scene.target], views, min_cover=min_cover)
    r.fit_init(views[scene.target])
    r.fit(T, use_closed_form=closed)
    return r, views


# ---- the float64 reference ------------------------------------------------------------------------------------------------
def reference_r2(obs, kept, J, params, u16mm=False, light=False):
    """Per view the (n, 3) float64 squared residuals of its observations (None for a view that is not kept)."""
    J64, p = J.astype(np.float64), params.astype(np.float64)
    B, beta, gamma = p[0:3], p[3:6], p[6:9]
    if light:   # sucre.py:54-61 with se3.exp (se3.py:22-27), float64
        from sucre_amd import se3
        R, t = [x.numpy() for x in se3.exp(torch.tensor(p[9:15], dtype=torch.float64))]
        sigma = p[15:19].reshape(2, 2)
        Minv = np.linalg.inv(sigma.T @ sigma)
    out = []
    for k, (u1, v1, cP, I, _, _) in enumerate(obs):
        if not kept[k]:
            out.append(None)
            continue
        z32 = np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2])   # the float32 range the store holds (sucre.py:53)
        if u16mm:   # what the fit of a u16mm store reads
            z32 = np.clip(np.rint(z32 * np.float32(1000.0)), np.float32(1.0), np.float32(65535.0)) * np.float32(0.001)
        z, l = z32.astype(np.float64), 1.0
        if light:
            lP = R @ cP.astype(np.float64) + t
            lp = lP[:2] / lP[2]
            l = np.exp(-(lp * (Minv @ lp)).sum(axis=0) / 2)[:, None]
            z = z + np.linalg.norm(lP, axis=0)
        z = z[:, None]
        Ihat = l * (J64[v1, u1] * np.exp(-beta * z) + B * (1 - np.exp(-gamma * z)))   # sucre.py:79-82
        out.append((I.T.astype(np.float64) - Ihat) ** 2)                               # sucre.py:144
    return out


def reference_round(obs, kept, H, W, r2, tau2, delta):
    """One round at thresholds tau2 (3,) float64: per view the dropped flags of its observations (guard applied), the (H,W) map
    of undecided pixels, the number of undecided observations and the pixels the guard protects."""
    band = 2 * delta * np.sqrt(tau2) + delta ** 2 + 2.0 ** -21 * tau2
    total, alive, undecided_px = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    out, n_undecided = [], 0
    for k, (u1, v1, *_) in enumerate(obs):
        if not kept[k]:
            out.append(None)
            continue
        o = (r2[k] > tau2).any(axis=1)
        und = (np.abs(r2[k] - tau2) <= band).any(axis=1)
        n_undecided += int(und.sum())
        undecided_px[v1[und], u1[und]] = True
        np.add.at(total, (v1, u1), 1)
        np.add.at(alive, (v1, u1), ~o)
        out.append(o)
    guarded = (total > 0) & (alive == 0)
    drops = [None if o is None else o & ~guarded[obs[k][1], obs[k][0]] for k, o in enumerate(out)]
    return drops, undecided_px, n_undecided, guarded


def bar(n, S, delta):
    return 2 * delta * np.sqrt(n * S) + n * delta ** 2 + 1e-5 * S


def stored_ranges(r):
    return np.stack([r.export_view(k)[0].cpu().numpy() for k in range(r.n_views)])


def trim_and_check(label, r, obs, k_sigma=K_SIGMA, u16mm=False, light=False, min_cover=1e-6):
    """Runs one round on ``r`` and checks thresholds, decisions and counts against the float64 reference.  Returns the engine's
    outputs, the reference's per-view drop flags and the guarded pixels."""
    delta = 2e-6 if light else 1e-6
    H, W = r.H, r.W
    J, params = r.J().cpu().numpy(), r.params().cpu().numpy()
    kept = r.view_keep().cpu().numpy() != 0
    assert np.array_equal(kept, np.array([len(o[0]) / (H * W) > min_cover for o in obs])), label
    z_before, counts_before = stored_ranges(r), r.view_counts().cpu().numpy().copy()
    for k, (u1, v1, *_) in enumerate(obs):   # the store holds the oracle's lists
        m = np.zeros((H, W), bool); m[v1, u1] = True
        assert np.array_equal(z_before[k] > 0, m), (label, 'store', k)

    dropped, view_dropped, thresholds = [t.cpu().numpy() for t in r.trim_outliers(k_sigma)]
    assert r.steps_done == 0
    assert dropped.dtype == np.int32 and dropped.shape == (H, W) and view_dropped.dtype == np.int64 and view_dropped.shape == (r.n_views,)
    assert thresholds.dtype == np.float32 and thresholds.shape == (3,)

    r2 = reference_r2(obs, kept, J, params, u16mm, light)
    N = sum(len(x) for x in r2 if x is not None)
    S = sum(x.sum(axis=0) for x in r2 if x is not None)
    tau_ref = k_sigma ** 2 * S / N
    tau_bar = k_sigma ** 2 * bar(N, S, delta) / N + 2.0 ** -23 * tau_ref
    print(f'{label}: N {N}, tau^2 {thresholds}, |d|/bar {np.abs(thresholds - tau_ref) / tau_bar}')
    assert np.all(np.abs(thresholds.astype(np.float64) - tau_ref) <= tau_bar), (label, thresholds, tau_ref)

    tau2 = thresholds.astype(np.float64)
    drops, undecided_px, n_undecided, guarded = reference_round(obs, kept, H, W, r2, tau2, delta)
    dist = min(float((np.abs(x - tau2) / (2 * delta * np.sqrt(tau2) + delta ** 2 + 2.0 ** -21 * tau2)).min()) for x in r2 if x is not None)
    n_ref = sum(int(d.sum()) for d in drops if d is not None)
    print(f'{label}: reference drops {n_ref} of {N}, {int(guarded.sum())} guarded pixels, {n_undecided} undecided observations, '
          f'nearest observation {dist:.1f} band widths from its threshold')
    assert n_undecided <= max(2, 1e-4 * N), (label, 'the case has too many undecided observations', n_undecided)

    z_after = stored_ranges(r)
    zeroed = (z_before > 0) & (z_after == 0)
    assert np.array_equal(z_after[~zeroed], z_before[~zeroed]), (label, 'a range that was not dropped changed')
    decided = ~undecided_px
    ref_zeroed = np.zeros_like(zeroed)
    for k, (u1, v1, *_) in enumerate(obs):
        if drops[k] is not None:
            ref_zeroed[k, v1[drops[k]], u1[drops[k]]] = True
    assert np.array_equal(zeroed[:, decided], ref_zeroed[:, decided]), (label, 'set of dropped observations')
    assert not zeroed[~kept].any(), (label, 'a view that is not kept lost observations')
    # the outputs and the re-finalised store agree with the set
    assert np.array_equal(dropped, zeroed.sum(axis=0)), (label, 'dropped')
    assert np.array_equal(view_dropped, zeroed.sum(axis=(1, 2))), (label, 'view_dropped')
    if n_undecided == 0:
        assert np.array_equal(dropped, ref_zeroed.sum(axis=0)) and np.array_equal(view_dropped, ref_zeroed.sum(axis=(1, 2))), label
    counts = r.view_counts().cpu().numpy()
    assert np.array_equal(counts, counts_before - view_dropped), (label, 'view_counts')
    keep_after = r.view_keep().cpu().numpy() != 0
    assert np.array_equal(keep_after, counts / (H * W) > min_cover), (label, 'view_keep')
    assert r.n_obs() == int(counts[keep_after].sum()), (label, 'n_obs')
    alive = (z_after[kept] > 0).sum(axis=0)
    assert np.all(alive[(z_before[kept] > 0).any(axis=0)] >= 1), (label, 'a pixel lost its last observation')
    return (dropped, view_dropped, thresholds), drops, guarded, zeroed


# ---- 1. decisions against float64 -------------------------------------------------------------------------------------------
def test_decisions_plain_planted():
    scene, obs = scene_of('planted75')
    r, _ = fitted(scene, 200)
    _, drops, guarded, zeroed = trim_and_check('plain 75x52 planted', r, obs)
    assert guarded.sum() >= 1, 'the case must exercise the guard'
    assert zeroed.sum() > 0


def test_decisions_closed_form():
    scene, obs = scene_of('planted75')
    r, _ = fitted(scene, 30, closed=True)
    trim_and_check('closed form', r, obs)


def test_decisions_u16mm():
    scene, obs = scene_of('planted75')
    r, _ = fitted(scene, 20, obs_format='u16mm')
    trim_and_check('u16mm', r, obs, u16mm=True)


def test_decisions_light_model():
    scene, obs = scene_of('planted75')
    r, _ = fitted(scene, 20, light=True)
    trim_and_check('light model', r, obs, light=True)


def test_decisions_71_views():
    scene, obs = scene_of('views71')
    r, _ = fitted(scene, 20)
    _, _, _, zeroed = trim_and_check('71 views', r, obs)
    assert zeroed.sum() > 0 and (stored_ranges(r) > 0).sum(axis=0).max() > 64


def test_decisions_more_than_256_tiles():
    scene, obs = scene_of('tiles272')
    assert (scene.width + 15) // 16 * ((scene.height + 15) // 16) == 272
    r, _ = fitted(scene, 5)
    _, _, _, zeroed = trim_and_check('272 tiles', r, obs)
    assert zeroed.sum() > 0


# ---- 2. the refit contract --------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


def surviving_lists(r, obs=None):
    """The per-view lists import_matches takes, from the store as it stands: camera points along with the light model, float32
    colours in place of the uint8 ones with ``float_colour``.  export_view_ext returns ONE set of planes -- the camera points
    of a store that holds both --, so there the colours are the test's own, ``obs[k]``'s I at the surviving pixels."""
    lists = []
    for k in range(r.n_views):
        z, rgb = r.export_view(k)
        v1, u1 = torch.where(z > 0)
        item = (u1.to(torch.int16), v1.to(torch.int16), z[v1, u1], None if r.float_colour else rgb[v1, u1])
        if r.both:
            I = torch.zeros((3, r.H, r.W), dtype=torch.float32)
            I[:, torch.from_numpy(obs[k][1]), torch.from_numpy(obs[k][0])] = torch.from_numpy(obs[k][3])
            item += (torch.cat([r.export_view_ext(k)[:, v1, u1], I.to(r.device)[:, v1, u1]]).contiguous(),)
        elif r.lws is not None:
            item += (r.export_view_ext(k)[:, v1, u1].contiguous(),)
        lists.append(item)
    return lists


def refit_contract(label, scene, T, rounds=1, min_cover=1e-6, closed=False, frgb=None, obs=None, start=None, **kw):
    """``start``: how the fitted workspace comes about, () -> (restoration, views); ``fitted`` (a matched store) unless given.
    The views kept before every round are left in ``a.kept_before_round``."""
    a, views = (fitted(scene, T, min_cover=min_cover, closed=closed, frgb=frgb, **kw) if start is None else start())
    target = views[scene.target]
    a.kept_before_round = []
    for _ in range(rounds):
        a.kept_before_round.append(a.view_keep().cpu().numpy() != 0)
        a.trim_outliers(K_SIGMA)
        lists = surviving_lists(a, obs)
        a.fit_init(target)
        ta = a.fit(T, use_closed_form=closed)
    b = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
    b.import_matches(target, lists, min_cover=min_cover)
    b.fit_init(target)
    tb = b.fit(T, use_closed_form=closed)
    for name, x, y in (('J', a.J(), b.J()), ('params', a.params(), b.params()), ('trace', ta, tb),
                       ('store_format', a.store_format(), b.store_format()), ('view_counts', a.view_counts(), b.view_counts()),
                       ('view_keep', a.view_keep(), b.view_keep())):
        assert _same_bits(x, y), (label, name)
    assert a.n_obs() == b.n_obs() > 0, label
    assert bool(torch.isfinite(ta).all())
    return a, b


@pytest.mark.parametrize('case', ['plain', 'u16mm', 'closed', 'light', 'two-rounds'])
def test_refit_equals_a_plain_run_on_the_survivors(case):
    scene, _ = scene_of('planted75')
    kw = {'u16mm': dict(obs_format='u16mm'), 'light': dict(light=True)}.get(case, {})
    a, _ = refit_contract(case, scene, 20, rounds=2 if case == 'two-rounds' else 1, closed=case == 'closed', **kw)
    assert a.n_obs() < sum(len(o[0]) for o in scene_of('planted75')[1])


def test_refit_when_the_planted_view_falls_below_min_cover():
    scene, obs = scene_of('planted75')
    n0, px = len(obs[0][0]), scene.width * scene.height
    min_cover = (n0 - 40) / px          # view 0 is kept with its n0 matches and drops out once more than 40 of them are gone
    a, b = refit_contract('min_cover', scene, 20, min_cover=min_cover)
    keep, counts = a.view_keep().cpu().numpy() != 0, a.view_counts().cpu().numpy()
    assert not keep[0] and 0 < counts[0] < n0 - 40 and keep.sum() >= 2
    assert np.array_equal(keep, counts / px > min_cover)


# ---- 3. against the oracle --------------------------------------------------------------------------------------------------
def test_trimmed_refit_against_the_oracle_on_the_survivors():
    scene, obs = scene_of('planted75')
    T = 200
    r, views = fitted(scene, T)
    r.trim_outliers(K_SIGMA)
    z = stored_ranges(r)
    kept = r.view_keep().cpu().numpy() != 0
    r.fit_init(views[scene.target])
    trace = r.fit(T).cpu().numpy()
    J = r.J().cpu().numpy()
    order = sorted(range(len(obs)), key=lambda k: scene.views[k].name)   # kept views in name order, as the loader lists them
    samples = []
    for k in order:
        if not kept[k]:
            continue
        u1, v1, cP, I, _, _ = obs[k]
        alive = z[k][v1, u1] > 0
        samples.append((u1[alive].astype(np.int16), v1[alive].astype(np.int16), np.ascontiguousarray(cP[:, alive]), np.ascontiguousarray(I[:, alive])))
    assert sum(len(s[0]) for s in samples) == r.n_obs()
    tgt = scene.views[scene.target]
    J0 = oracle.init_J(tgt.rgb_u8.numpy(), tgt.depth_f32().numpy())
    Jo, po, to = oracle.fit(scene.height, scene.width, samples, J0, num_iter=T)
    rms = helpers.rms_per_channel(J, Jo)
    print(f'trimmed refit vs oracle on the survivors: rms {rms}, params {np.abs(trace[:, 1:] - to[:, 1:]).max():.2e}, '
          f'cost {np.abs(trace[:, 0] / to[:, 0] - 1).max():.2e}')
    assert np.array_equal(np.isnan(J), np.isnan(Jo))
    assert rms.max() < 1e-5                                   # test_gpu_parity's bars for the J-parameter mode
    assert np.abs(trace[:, 1:] - to[:, 1:]).max() < 1e-5
    assert np.abs(trace[:, 0] / to[:, 0] - 1).max() < 1e-4


# ---- 4. it does its job -----------------------------------------------------------------------------------------------------
def test_trim_removes_the_planted_patch_and_restores_the_fit():
    clean, _ = scene_of('clean75')
    scene, obs = scene_of('planted75')
    T = 200
    rc, _ = fitted(clean, T)
    Jc = rc.J().cpu().numpy()
    r, views = fitted(scene, T)
    J_untrimmed = r.J().cpu().numpy()
    u1, v1, _, _, u2, v2 = obs[0]
    hit = (v2 >= PATCH[0].start) & (v2 < PATCH[0].stop) & (u2 >= PATCH[1].start) & (u2 < PATCH[1].stop)
    assert hit.sum() >= 100
    r.trim_outliers(K_SIGMA)
    gone = r.export_view(0)[0].cpu().numpy()[v1, u1] == 0
    r.fit_init(views[scene.target])
    r.fit(T)
    J = r.J().cpu().numpy()
    hit_px = np.zeros((scene.height, scene.width), bool)
    hit_px[v1[hit], u1[hit]] = True
    ok = np.isfinite(Jc).all(axis=-1)

    def rms(a, where):
        d = (a[where & ok].astype(np.float64) - Jc[where & ok].astype(np.float64))
        return float(np.sqrt((d * d).mean()))
    share = gone[hit].sum() / hit.sum()
    print(f'planted {int(hit.sum())}, dropped {int(gone[hit].sum())} of them ({share:.3f}) and {int(gone[~hit].sum())} others in view 0; '
          f'rms(J) in the hit pixels {rms(J_untrimmed, hit_px):.4f} -> {rms(J, hit_px):.4f}, elsewhere {rms(J_untrimmed, ~hit_px):.5f} -> {rms(J, ~hit_px):.5f}')
    assert share >= 0.9
    assert rms(J, hit_px) <= 0.5 * rms(J_untrimmed, hit_px)
    assert rms(J, ~hit_px) <= 0.2 * rms(J_untrimmed, ~hit_px)


# ---- 5. determinism and hygiene ---------------------------------------------------------------------------------------------
def _trimmed_run(scene, T, fill=None, frgb=None, **kw):
    views = device_views(scene, frgb)
    r = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
    if fill is not None:
        r.ws.fill_(fill)
        if r.lws is not None:
            r.lws.fill_(fill)
    r.match(views[scene.target], views)
    r.fit_init(views[scene.target])
    r.fit(T)
    outs = r.trim_outliers(K_SIGMA)
    r.fit_init(views[scene.target])
    trace = r.fit(T)
    return r, outs + (trace, r.J(), r.params(), r.view_counts().clone(), r.store_format().clone())


@pytest.mark.parametrize('kw', [dict(light=False), dict(light=True), dict(float_colour=True), dict(light=True, float_colour=True)],
                         ids=['plain', 'light', 'float-colour', 'light-float-colour'])
def test_two_runs_and_a_dirty_workspace_give_the_same_bits(kw):
    scene, _ = scene_of('planted75')
    frgb = float_scene_of('planted75')[2] if kw.get('float_colour') else None
    _, first = _trimmed_run(scene, 20, frgb=frgb, **kw)
    _, second = _trimmed_run(scene, 20, frgb=frgb, **kw)
    _, dirty = _trimmed_run(scene, 20, fill=0xFF, frgb=frgb, **kw)
    for x, y, z in zip(first, second, dirty):
        assert _same_bits(x, y) and _same_bits(x, z)
    assert int(first[1].sum()) > 0


def test_clean_scene_with_a_huge_multiple_drops_nothing():
    scene, _ = scene_of('clean75')
    r, views = fitted(scene, 20)
    t0, J0, p0 = r.trace.clone(), r.J(), r.params().clone()
    counts, fmt, n = r.view_counts().clone(), r.store_format().clone(), r.n_obs()
    dropped, view_dropped, _ = r.trim_outliers(1000.0)
    assert int(dropped.sum()) == 0 and int(view_dropped.sum()) == 0
    r.fit_init(views[scene.target])
    t1 = r.fit(20)
    assert _same_bits(t0, t1) and _same_bits(J0, r.J()) and _same_bits(p0, r.params())
    assert _same_bits(counts, r.view_counts()) and _same_bits(fmt, r.store_format()) and n == r.n_obs()


def test_residuals_after_the_trimmed_refit():
    from test_gpu_residuals import check_against_reference
    scene, obs = scene_of('planted75')
    r, views = fitted(scene, 20)
    r.trim_outliers(K_SIGMA)
    z = stored_ranges(r)
    r.fit_init(views[scene.target])
    r.fit(20)
    px = scene.width * scene.height
    surviving = []
    for k, (u1, v1, cP, I, _, _) in enumerate(obs):
        alive = z[k][v1, u1] > 0
        surviving.append((alive.sum() / px, u1[alive], v1[alive], cP[:, alive], I[:, alive]))
    check_against_reference('after the trimmed refit', r, surviving)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disk_scene(tmp_path_factory):
    from test_gpu_api import scene_as_loaded, write_scene
    from sucre_amd import sfm
    root = tmp_path_factory.mktemp('trim_scene')
    scene = synth.make_scene(96, 64, 4, seed=21, far_views=1)
    bad = copy.copy(scene)
    bad.views = list(scene.views)
    v = copy.copy(scene.views[0])
    rgb = v.rgb_u8.clone().to(torch.int32)
    rgb[25:39, 42:54] += torch.tensor(CAST, dtype=torch.int32)
    v.rgb_u8 = rgb.clamp(0, 255).to(torch.uint8)
    bad.views[0] = v
    write_scene(bad, root)
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    return root, bad, scene_as_loaded(bad, model)


def _base(root):
    return ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'), '--num-iter', '10']


TRIM_FILES = ('_trim.pt', '_trimmed.png')


def test_cli_trim_outliers_files(disk_scene, tmp_path, capsys):
    from PIL import Image as PILImage
    from sucre_amd import sucre
    root, scene, loaded = disk_scene
    name = scene.names[scene.target]
    stem = Path(name).stem
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'off'), '--image-name', name])
    assert not [p for p in (tmp_path / 'off').iterdir() if p.name.endswith(TRIM_FILES)]
    capsys.readouterr()
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'on'), '--image-name', name, '--trim-outliers', '3', '--save-quality'])
    out = capsys.readouterr().out
    t = torch.load(tmp_path / 'on' / f'{stem}_trim.pt')
    assert set(t) >= {'dropped', 'views', 'view_dropped', 'thresholds', 'k'}
    n = len(t['views'])
    assert t['k'] == 3.0 and t['dropped'].dtype == torch.int32 and t['dropped'].shape == (1, 64, 96)
    assert t['view_dropped'].dtype == torch.int64 and t['view_dropped'].shape == (1, n)
    assert t['thresholds'].dtype == torch.float32 and t['thresholds'].shape == (1, 3)
    D = int(t['view_dropped'].sum())
    assert D == int(t['dropped'].sum()) > 0
    assert f'{name}: trim round 1 dropped {D} of {int(t["n_obs"][0])} observations (threshold R ' in out
    png = np.asarray(PILImage.open(tmp_path / 'on' / f'{stem}_trimmed.png'))
    n_kept = int(t['view_kept'][0].sum())
    assert np.array_equal(png, np.uint8(255 * t['dropped'].numpy().astype(np.int64).sum(axis=0) // n_kept))
    # --save-quality describes the final fit: its counts are the survivors'
    q = torch.load(tmp_path / 'on' / f'{stem}_quality.pt')
    assert int(q['count'].sum()) == int(t['n_obs'][0]) - D
    # J in the .pt is the engine path: match, fit, trim, fit_init, fit
    views = engine.device_views_from_scene(loaded, DEV)
    r = engine.Restoration(loaded.height, loaded.width, len(views), device=DEV)
    r.match(views[loaded.target], views)
    r.fit_init(views[loaded.target])
    r.fit(10)
    dropped, _, thresholds = r.trim_outliers(3.0)
    r.fit_init(views[loaded.target])
    r.fit(10)
    got = torch.load(tmp_path / 'on' / f'{stem}.pt')
    # The command line hands the fit a float32 J0 made by torch on the host and leaves out the view its overlap cull removes, the
    # engine path above starts from the uint8 image on the device and keeps that (empty) view: the same fit up to float32
    # rounding of the start, which test_gpu_api holds to 1e-6 RMS between two such paths.  The decisions are discrete and the
    # same; the thresholds are float32 numbers formed from sums that agree to that rounding (a few units of 2^-24, relative).
    assert _same_bits(t['dropped'][0], dropped.cpu())
    assert helpers.rms_per_channel(got['J'].numpy(), r.J().cpu().numpy()).max() < 1e-6
    assert np.array_equal(np.isnan(got['J'].numpy()), np.isnan(r.J().cpu().numpy()))
    assert np.abs(t['thresholds'][0].numpy() / thresholds.cpu().numpy() - 1).max() < 1e-5
    off = torch.load(tmp_path / 'off' / f'{stem}.pt')
    assert not torch.equal(torch.nan_to_num(off['J'], nan=-7.0), torch.nan_to_num(got['J'], nan=-7.0))


@pytest.mark.parametrize('fit_batch', ['1', 'auto'], ids=['two-in-flight', 'one-launch-per-iteration'])
def test_cli_survey_trim_equals_single_runs(disk_scene, tmp_path, monkeypatch, fit_batch):
    from sucre_amd import sucre
    root, scene, loaded = disk_scene
    monkeypatch.setenv('SUCRE_IMAGES_IN_FLIGHT', '2')
    monkeypatch.setenv('SUCRE_FIT_BATCH', fit_batch)
    sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'survey'), '--image-ids', '1', '4', '--trim-outliers', '3'])
    got = sorted((tmp_path / 'survey').glob('*_trim.pt'))
    assert len(got) == 3
    for p in got:
        stem = p.name[:-len('_trim.pt')]
        sucre.main(_base(root) + ['--output-dir', str(tmp_path / 'single'), '--image-name', f'{stem}.png', '--trim-outliers', '3'])
        a, b = torch.load(p), torch.load(tmp_path / 'single' / p.name)
        assert a['views'] == b['views'] and a['k'] == b['k']
        for k in ('dropped', 'view_dropped', 'thresholds', 'n_obs', 'view_kept'):
            assert _same_bits(a[k], b[k]), (p.name, k)
        a, b = torch.load(tmp_path / 'survey' / f'{stem}.pt'), torch.load(tmp_path / 'single' / f'{stem}.pt')
        for k in a:
            assert _same_bits(a[k], b[k]), (stem, k)
        assert (tmp_path / 'survey' / f'{stem}_trimmed.png').read_bytes() == (tmp_path / 'single' / f'{stem}_trimmed.png').read_bytes()
