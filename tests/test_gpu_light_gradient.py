"""The --light-model gradient on the device against float64 autograd (tests/light64.py), read through the public interface.

ONE Adam iteration at lr = 1024, eps = 1 from a chosen parameter point: the step p1 - p0 = -lr g / (|g| + eps) is an almost
linear image of the gradient, read from the trace row, ``params()`` and ``J()``.  The points (light64.POINTS) put weight on what
the reference's start (cam2light = 0, sigma = I) leaves idle: Q and the coefficients D, E of the SE(3) left Jacobian, the
trigonometric branch of se3_coefficients and its switch at theta^2 = 1/4, theta ~ pi, and the sigma chain rule at a sigma that is
not diagonal.  Every light entry point is driven: sucre_fit_run_light on uint8 colours, on float32 colours (kBoth), float32
colours without light (kColour), and the shared-lamp group (sucre_light_group_*) over two images of different sizes.

Bar, per component (the crafted rule, tests/crafted.py): |step_engine - step64| <= max(8 |step_oracle - step64|, 4 x 2^-24 x
max(|p0|, |p1|), lane) -- eight times the float32 CPU oracle's own distance from float64, measured here on the same case, or
the float32 rounding of the step itself, or ``lane`` = light64.lane_sum_bar: 2^-22 sum_obs |d l_i / d p_k| through the step's
slope, what light_grad_kernel's float32 lane sums and its 1-ulp v_rcp_f32 / v_rsq_f32 / v_exp_f32 may move a component by (the
oracle adds the same float32 terms in float64 and divides in IEEE; DESIGN.md, "The light gradient against autograd").  Measured
on the MI355X: with the first two terms alone eleven components of six cases missed by factors of 1.01 to 3.0 (u8 start jparam
[13] 2.07e-7 against 7.8e-8; u8 start closed [4] 1.26e-6 against 5.7e-7), all of them cancelling sums (sum |term| = 7 .. 65 |g|)
where the oracle happened to land within a few 1e-8 of float64; ``lane`` is 7e-7 .. 5.7e-6 there, 4 .. 12 x the engine's error.
With it the worst component of any case stands at 0.92 of its bar, and every step is at least 3.5e3 bars long.  J (one
value per pixel and channel, J-parameter mode) is held as a group: 8 x the oracle's largest |dJ_oracle - dJ64| over the pixels.
Both errors are printed per case and group on one ``LIGHTGRAD`` line.  Conditions on the cases (every component's step at least
100 bars long; the roll component at 'start', whose gradient is 0 by symmetry, excepted and held to its bar all the same) are
asserted on the yardstick before the engine is looked at.
"""
import numpy as np
import pytest
import torch

import light64
from light64 import EPS, GROUPS, LR, POINTS, ROLL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
COST_BAR = 1e-6          # relative, tests/test_gpu_parity.py::test_light_model_vs_oracle_short
ALIVE = 100.0

_CACHE: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _scene(name):
    from sucre_amd import synth
    return _cached(('scene', name), lambda: synth.make_scene(48, 32, 3, seed=3) if name == 'a' else synth.make_scene(47, 33, 2, seed=5))


def _float_images(name):
    from test_gpu_trim import float_images
    return _cached(('frgb', name), lambda: float_images(_scene(name)))


def _image(name, fcol=False):
    """light64.Image of the scene's target: the oracle's match lists (uint8 colours, or gathered from the float32 images) and
    the J the fit starts from."""
    def make():
        sc = _scene(name)
        if not fcol:
            return light64.scene_image(sc)
        from test_gpu_trim import scene_observations
        frgb = _float_images(name)
        obs = scene_observations(sc, frgb)
        samples = [(u1.astype(np.int16), v1.astype(np.int16), cP, I) for u1, v1, cP, I, _, _ in obs if len(u1) / (sc.width * sc.height) > 1e-6]
        tgt = sc.views[sc.target]
        J0 = frgb[sc.target].numpy().copy()
        J0[tgt.depth_f32().numpy() <= 0] = np.nan             # sucre.py:47-49
        return light64.Image(sc.height, sc.width, samples, J0)
    return _cached(('image', name, fcol), make)


def _reference(names, fcol, point, closed, light=True):
    """(yardstick result, oracle's (cost, p1, Js)) of the images ``names`` at the point, computed once."""
    def make():
        ims = [_image(n, fcol) for n in names]
        res = light64.evaluate(ims, POINTS[point], light=light, closed=closed, per_observation=True)
        return res, light64.oracle_step(ims, POINTS[point], closed, light=light)
    return _cached(('ref', names, fcol, point, closed, light), make)


def _restoration(name, light=True, fcol=False, role='single'):
    """The scene matched once per flavour and role; every case starts over with fit_init.  A role per launch sequence: a light group
    leaves ITS n_obs total in every image's workspace (SUCRE_WS_N_OBS_TOTAL, as sucre_set_n_obs_total does) until the next match,
    and a single fit on that workspace would be scaled by it."""
    def make():
        from sucre_amd import engine
        sc = _scene(name)
        if fcol:
            from test_gpu_trim import device_views
            views = device_views(sc, _float_images(name))
        else:
            views = engine.device_views_from_scene(sc, DEV)
        r = engine.Restoration(sc.height, sc.width, len(views), device=DEV, light=light, float_colour=fcol)
        r.match(views[sc.target], views)
        return r, views[sc.target]
    return _cached(('restoration', name, light, fcol, role), make)


def _init(name, point, light=True, fcol=False, role='single'):
    r, target = _restoration(name, light, fcol, role)
    r.fit_init(target, params0=POINTS[point], J0=torch.from_numpy(_image(name, fcol).J0).to(DEV))
    return r


def _params19(r):
    """All 19 stored parameters (``params()`` hands out the nine water values of a restoration without light)."""
    off = r.lib.sucre_light_params_offset(r.H, r.W, r.n_views)
    return r.lws[off:off + 76].view(torch.float32).cpu().numpy()


def _check(label, point, closed, ref, cost, p1, Js, J0s, n_obs, light=True):
    """The conditions on the case, then the engine's step against the yardstick's."""
    res, (ocost, op1, oJs) = ref
    p0 = POINTS[point].astype(np.float64)
    n = 19 if light else 9
    assert EPS >= 4 * np.abs(res.g).max(), (label, 'eps against the largest |g|', np.abs(res.g).max())
    d64, do = light64.delta64(res.g), op1 - p0
    lane = light64.lane_sum_bar(res)
    bar = light64.crafted_bar(d64, do, p0, extra=lane)
    alive = np.abs(d64) / bar
    live = np.ones(19, bool)
    live[n:] = False
    if point == 'start':
        assert abs(res.g[ROLL]) < 1e-12, (label, 'roll gradient at the start', res.g[ROLL])
        live[ROLL] = False
    assert (alive[live] >= ALIVE).all(), (label, 'a component is not alive', np.nonzero(live & (alive < ALIVE))[0], alive)
    assert abs(ocost / res.cost - 1) < COST_BAR and n_obs == res.n_obs, (label, 'n_obs', n_obs, res.n_obs)
    # -- the engine
    assert abs(cost / res.cost - 1) < COST_BAR, (label, 'cost', cost, res.cost)
    de = p1.astype(np.float64) - p0
    err, oerr = np.abs(de - d64), np.abs(do - d64)
    line = f'LIGHTGRAD {label}'
    for gname, sl in GROUPS[:3 if light else 1]:
        k = sl.start + int(np.argmax(err[sl] / bar[sl]))
        line += (f' | {gname} engine {err[sl].max():.2e} oracle {oerr[sl].max():.2e} worst[{k}] {err[k]:.2e}/{bar[k]:.2e}'
                 f' (lane {lane[k]:.1e}) alive {alive[sl][live[sl]].min():.1e}')
    dJ = None
    if not closed:
        dJ, barJ = [], []
        for J, J0, oJ, gJ, seen in zip(Js, J0s, oJs, res.gJ, res.seen):
            assert np.array_equal(J[~seen].view(np.uint32), J0[~seen].view(np.uint32)), (label, 'a pixel without observations moved')
            dJ64 = light64.delta64(gJ)
            dJ.append(np.abs(J.astype(np.float64) - J0 - dJ64)[seen].max())
            barJ.append(8 * np.abs(oJ.astype(np.float64) - J0 - dJ64)[seen].max())
            assert np.median(np.abs(dJ64[seen])) >= ALIVE * barJ[-1], (label, 'J is not alive')
        line += ' | J ' + ' '.join(f'engine {a:.2e} bar {b:.2e}' for a, b in zip(dJ, barJ))
    print(line)
    bad = np.nonzero(~(err[:n] <= bar[:n]))[0]
    assert bad.size == 0, (label, 'components', bad.tolist(), 'error', err[bad], 'bar', bar[bad], 'step64', d64[bad], 'oracle error', oerr[bad], 'lane', lane[bad])
    if dJ is not None:
        assert all(a <= b for a, b in zip(dJ, barJ)), (label, 'J', dJ, barJ)


def _single(name, point, closed, fcol=False, role='single'):
    r = _init(name, point, fcol=fcol, role=role)
    trace = r.fit(1, lr=LR, eps=EPS, use_closed_form=closed, keep_J=True)
    torch.cuda.synchronize()
    t = trace.cpu().numpy()
    assert t.shape == (1, 20)
    p1 = r.params().cpu().numpy()
    assert np.array_equal(p1, t[0, 1:].astype(np.float32)) and np.array_equal(p1.astype(np.float64), t[0, 1:]), 'the trace row and params() differ'
    return r, t, p1, r.J().cpu().numpy()


@pytest.mark.parametrize('closed', [False, True], ids=['jparam', 'closed'])
@pytest.mark.parametrize('point', list(POINTS))
def test_single_image_uint8(point, closed):
    """sucre_fit_run_light on uint8 colours, 48x32 with 3 neighbours: every point, both modes."""
    im = _image('a')
    r, t, p1, J = _single('a', point, closed)
    _check(f'u8 {point} {"closed" if closed else "jparam"}', point, closed, _reference(('a',), False, point, closed), t[0, 0], p1, [J], [im.J0], r.n_obs())


@pytest.mark.parametrize('closed', [False, True], ids=['jparam', 'closed'])
@pytest.mark.parametrize('point', ['small', 'roll3'])
def test_single_image_float_colours(point, closed):
    """The kBoth instantiation: the light model on float32 colours that are not k/255."""
    im = _image('a', True)
    r, t, p1, J = _single('a', point, closed, fcol=True)
    _check(f'f32 {point} {"closed" if closed else "jparam"}', point, closed, _reference(('a',), True, point, closed), t[0, 0], p1, [J], [im.J0], r.n_obs())


def test_float_colours_without_light():
    """kColour: l = 1, z = ||cP||.  The water step against the no-light yardstick; cam2light and sigma keep their bits."""
    point, im = 'small', _image('a', True)
    r = _init('a', point, light=False, fcol=True)
    trace = r.fit(1, lr=LR, eps=EPS)
    torch.cuda.synchronize()
    t, p19 = trace.cpu().numpy(), _params19(r)
    assert t.shape == (1, 10) and np.array_equal(r.params().cpu().numpy(), p19[:9]) and np.array_equal(p19[:9].astype(np.float64), t[0, 1:])
    assert np.array_equal(p19[9:].view(np.uint32), POINTS[point][9:].view(np.uint32)), 'cam2light or sigma moved without a light model'
    _check('f32 no light small jparam', point, False, _reference(('a',), True, point, False, light=False), t[0, 0], p19, [r.J().cpu().numpy()],
           [im.J0], r.n_obs(), light=False)


def _group(names, point, closed, role='pair'):
    from sucre_amd import engine
    rs = [_init(n, point, role=role) for n in names]
    trace = torch.zeros((1, 20), dtype=torch.float64, device=DEV)
    g = engine.HipWaterGroup(rs, lr=LR, eps=EPS, use_closed_form=closed, trace=trace, params0=POINTS[point])
    g.set_n_obs_total(g.n_obs())
    g.grad(1)
    g.step(1)
    g.finish()
    torch.cuda.synchronize()
    return rs, trace.cpu().numpy(), [r.params().cpu().numpy() for r in rs], [r.J().cpu().numpy() for r in rs]


@pytest.mark.parametrize('closed', [False, True], ids=['jparam', 'closed'])
@pytest.mark.parametrize('point', ['small', 'above', 'roll3'])
def test_group_of_two_sizes(point, closed):
    """engine.HipWaterGroup over two light images of different sizes (48x32 and 47x33): grad(1), step(1), finish() against the
    yardstick over both images' observations with the total n_obs; each image's J step in J-parameter mode.  (In closed-form
    mode finish() solves J again at the stepped parameters, which mean nothing: J is not read there.)"""
    names = ('a', 'b')
    rs, t, ps, Js = _group(names, point, closed)
    assert np.array_equal(ps[0], ps[1]) and np.array_equal(ps[0].astype(np.float64), t[0, 1:])
    ims = [_image(n) for n in names]
    assert [r.n_obs() for r in rs] == [im.n_obs() for im in ims]
    _check(f'group {point} {"closed" if closed else "jparam"}', point, closed, _reference(names, False, point, closed), t[0, 0], ps[0], Js,
           [im.J0 for im in ims], sum(r.n_obs() for r in rs))


@pytest.mark.parametrize('closed', [False, True], ids=['jparam', 'closed'])
@pytest.mark.parametrize('name', ['a', 'b'])
def test_group_of_one_is_the_single_fit(name, closed):
    """A group of one image leaves the bits of the single image's two calls, fit(1, keep_J) and (closed form) update_J()."""
    point = 'roll3'
    r, t1, p1, J1 = _single(name, point, closed, role='one')
    if closed:
        r.update_J()
        J1 = r.J().cpu().numpy()
    _, tg, pg, Jg = _group((name,), point, closed, role='one')
    assert np.array_equal(tg, t1) and np.array_equal(pg[0], p1)
    assert np.array_equal(Jg[0].view(np.uint32), J1.view(np.uint32))


def test_the_water_values_are_the_inversion_tests():
    import test_gpu_invert
    assert light64.WATER == test_gpu_invert.WATER
