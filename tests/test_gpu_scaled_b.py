"""The B-scaled chunk arithmetic of csrc/fit.hip (grad_terms / closed_terms: bo = fma(-B, g, B), the sums of r (1 - g) accumulated
as B sum r (1 - g) and divided by B where a launch's sums become final) and its fallback, the unscaled form, which a launch takes
whenever one |B_c| is 0, not finite or outside fit_math.h's window (scaled_b_ok).

One hand-built store (tests/crafted.py) whose count histogram holds every kind of item the two forms are compiled into -- unmasked
and masked full chunks, short last chunks of 1, 2 and 3 levels, pixels nobody observes -- and starts of B on either side of every
edge of the predicate, through every launch that runs the pass: the fused fit, a batch launch, a shared-water group and the split
grad / step path.  Five iterations against the CPU oracle at the bars tests/test_gpu_parity.py holds short fits to."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import crafted
import helpers
from oracle import oracle

pytestmark = pytest.mark.gpu

T = 5
H, W, N_VIEWS = 48, 64, 12
MODES = [False, True]
MODE_IDS = ['J-parameter', 'closed-form']


def _window():
    """kScaledBMin, kScaledBMax as csrc/fit_math.h states them (C hexadecimal float literals)."""
    text = (Path(helpers.ROOT) / 'sucre_amd' / 'csrc' / 'fit_math.h').read_text()
    m = re.search(r'kScaledBMin = (0x1p[-+]\d+)f, kScaledBMax = (0x1p[-+]\d+)f;', text)
    return np.float32(float.fromhex(m.group(1))), np.float32(float.fromhex(m.group(2)))


LO, HI = _window()
_below = lambda x: np.nextafter(np.float32(x), np.float32(0))
_above = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
# name -> (B of the three channels, does the FIRST launch run the scaled form?)
STARTS = {
    'default': ((0.1, 0.1, 0.1), True),
    'zero': ((0.0, 0.0, 0.0), False),
    'one_zero': ((0.1, 0.0, 0.1), False),            # one channel fails the predicate: the whole launch falls back
    'negative': ((-0.05, -0.05, -0.05), True),        # a negative scale
    'lo_inside': ((LO, LO, LO), True),
    'lo_outside': ((_below(LO), LO, LO), False),
    'hi_inside': ((HI, HI, HI), True),
    'hi_outside': ((HI, _above(HI), HI), False),
    # just below the window; the first step (Adam: lr = 0.05 long, whatever the gradient's size) carries B to about -0.05 (J as a
    # parameter) or +0.05 (closed form), inside: the form changes between two launches of ONE fit
    'crossing': ((_below(LO),) * 3, False),
}


def scaled_b_ok(B):
    """fit_math.h scaled_b_ok restated (tests/native/scaled_b_check.cpp holds the C++ one to its edges on the host)."""
    a = np.abs(np.asarray(B, np.float32))
    return bool(np.all(np.isfinite(a)) and np.all(a >= LO) and np.all(a <= HI))


def test_starts_sit_where_they_claim():
    assert LO <= np.float32(0.1) <= HI
    for name, (B, scaled) in STARTS.items():
        assert scaled_b_ok(B) == scaled, name


# ---- the store --------------------------------------------------------------------------------------------------------------------
_CACHE: dict = {}


def _geometry():
    if 'g' not in _CACHE:
        count = np.random.default_rng(3).permutation(np.arange(H * W) % (N_VIEWS + 1))      # 0 .. 12 observations, scattered
        _CACHE['g'] = crafted.build(H, W, N_VIEWS, count, seed=4)
    return _CACHE['g']


def test_histogram_holds_every_kind_of_item():
    """The strips are 64 count-sorted pixels each (csrc/compact.hip); in either sorting direction the store has a strip with an
    unmasked full chunk, one with a masked full chunk, short last chunks of 1, 2 and 3 levels and pixels without an observation."""
    cm = np.sort(_geometry().count_map().reshape(-1))
    assert cm[0] == 0 and H * W % 64 == 0
    for order in (cm, cm[::-1]):
        strips = order.reshape(-1, 64)
        levels, full = strips.max(axis=1), strips.min(axis=1)
        assert len(strips) > 16                                  # more than one workgroup's waves
        assert np.any(full >= 4)                                 # a chunk every pixel of the strip fills
        assert np.any(levels // 4 > full // 4)                   # a full chunk with empty slots
        assert {1, 2, 3} <= set((levels % 4).tolist())


def _list_set(seed=0):
    g = _geometry()
    return crafted.ListSet(g, rgb=crafted.random_colours(g, seed))


def _J0(closed):
    """crafted.trajectory's start, J0 in [3, 4): every residual negative, every gradient a sum of terms of one sign (no Adam knee).
    J-parameter mode: NaN where nobody observes the pixel, as fit_init leaves a pixel without depth."""
    J0 = (3.0 + np.random.default_rng(11).random((H, W, 3))).astype(np.float32)
    if not closed:
        J0[_geometry().count_map() == 0] = np.nan
    return J0


def _params0(start):
    p = np.full(9, 0.1, np.float32)
    p[:3] = np.asarray(STARTS[start][0], np.float32)
    return p


def _restoration():
    from sucre_amd import engine
    return engine.Restoration(H, W, N_VIEWS)


def _load(r, ls, p0, J0):
    tgt = crafted.target_view(H, W)
    r.import_matches(tgt, crafted.device_lists(ls, 'cuda'), min_cover=ls.geom.min_cover)
    r.fit_init(tgt, p0, J0=torch.from_numpy(np.ascontiguousarray(J0)).cuda())


def _oracle_fit(start, closed, seed=0):
    key = ('oracle', start, closed, seed)
    if key not in _CACHE:
        _CACHE[key] = oracle.fit(H, W, _list_set(seed).samples(), None if closed else _J0(closed), params0=_params0(start), num_iter=T,
                                 use_closed_form=closed)
    return _CACHE[key]


def _engine_alone(start, closed, seed=0):
    """(trace, J, params) of the image fitted by itself, the fused launch."""
    key = ('alone', start, closed, seed)
    if key not in _CACHE:
        r = _restoration()
        _load(r, _list_set(seed), _params0(start), _J0(closed))
        trace = r.fit(T, use_closed_form=closed).cpu().numpy()
        _CACHE[key] = (trace, r.J().cpu().numpy(), r.params().cpu().numpy())
    return _CACHE[key]


def _hold(label, closed, trace, J, params, to, Jo, po):
    """The bars of tests/test_gpu_parity.py's short fits against the oracle (e.g. test_views_beyond_the_first_mask_word)."""
    assert np.array_equal(np.isnan(J), np.isnan(Jo)), label
    rms = helpers.rms_per_channel(J, Jo).max()
    dpar = np.abs(trace[:, 1:] - to[:, 1:]).max()
    dcost = np.abs(trace[:, 0] / to[:, 0] - 1).max()
    print(f'SCALED_B {label}: rms(J) {rms:.2e} parameters {dpar:.2e} cost {dcost:.2e}')
    assert rms < (1e-4 if closed else 1e-5), (label, rms)
    assert dpar < (2e-4 if closed else 1e-5), (label, dpar)
    assert dcost < (1e-4 if closed else 1e-5), (label, dcost)
    assert np.array_equal(params, trace[-1, 1:].astype(np.float32)), label
    assert np.abs(params - po).max() < (2e-4 if closed else 1e-5), label


@pytest.mark.parametrize('closed', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('start', list(STARTS))
def test_fit_against_the_oracle(start, closed):
    trace, J, params = _engine_alone(start, closed)
    Jo, po, to = _oracle_fit(start, closed)
    if not closed:
        assert np.isnan(J).any()      # the pixels nobody observes
    _hold((start, MODE_IDS[closed]), closed, trace, J, params, to, Jo, po)
    if start == 'crossing':           # the second launch runs the other form than the first
        assert not scaled_b_ok(_params0(start)[:3]) and scaled_b_ok(trace[0, 1:4].astype(np.float32)), trace[0, 1:4]


# one image in the fallback between two in the scaled form (at their first launch), every start once
BATCHES = [('default', 'zero', 'negative'), ('lo_inside', 'one_zero', 'hi_inside'), ('default', 'lo_outside', 'negative'),
           ('lo_inside', 'hi_outside', 'hi_inside'), ('default', 'crossing', 'negative')]


@pytest.mark.parametrize('closed', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('starts', BATCHES, ids=['-'.join(b) for b in BATCHES])
def test_batch_launch_of_three_equals_the_fits_alone(starts, closed):
    """sucre_fit_run_batch's promise: every image of a launch gets the bits of its own fit -- here with the form picked per image."""
    from sucre_amd import engine
    assert [STARTS[s][1] for s in starts] == [True, False, True]
    rs = []
    for s in starts:
        r = _restoration()
        _load(r, _list_set(), _params0(s), _J0(closed))
        rs.append(r)
    traces = engine.fit_batch(rs, T, use_closed_form=closed)
    for s, r, tr in zip(starts, rs, traces):
        t1, J1, p1 = _engine_alone(s, closed)
        assert np.array_equal(tr.cpu().numpy()[:, :10], t1, equal_nan=True), (s, 'trace')
        assert np.array_equal(r.J().cpu().numpy().view(np.uint32), J1.view(np.uint32)), (s, 'J')
        assert np.array_equal(r.params().cpu().numpy(), p1, equal_nan=True), (s, 'parameters')


def _oracle_lockstep(start, closed, seeds):
    """The oracle's shared-water fit of the images `seeds` (tests/test_gpu_api.py): (parameter rows, cost rows, images)."""
    imgs = [oracle.SharedWaterImage(H, W, _list_set(sd).samples(), None if closed else _J0(closed), use_closed_form=closed) for sd in seeds]
    total = sum(o.n_obs for o in imgs)
    pstate = np.zeros(27, np.float32)
    pstate[:9] = _params0(start)
    rows, costs = [], []
    for it in range(1, T + 1):
        acc = sum(o.grad(pstate[:9], it, total) for o in imgs)
        oracle.shared_step(pstate, acc, it, total)
        rows.append(pstate[:9].copy())
        costs.append(acc[9])
    if closed:
        for o in imgs:
            o.final_update_J(pstate[:9])
    return np.array(rows), np.array(costs), imgs


@pytest.mark.parametrize('closed', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('start', list(STARTS))
def test_shared_water_group_of_two(start, closed):
    """group_iter_kernel: the step is taken in the next launch's prologue, and the finisher divides by the B that launch stepped to."""
    from sucre_amd import dist as sdist
    from sucre_amd import engine
    rs = []
    for sd in (0, 1):
        r = _restoration()
        _load(r, _list_set(sd), _params0(start), _J0(closed))
        rs.append(r)
    trace = torch.zeros((T, 10), dtype=torch.float64, device='cuda')
    sdist.fit_shared_water(engine.HipWaterGroup(rs, use_closed_form=closed, trace=trace, params0=_params0(start)), T)
    trace = trace.cpu().numpy()
    rows, costs, imgs = _oracle_lockstep(start, closed, (0, 1))
    dpar, dcost = np.abs(trace[:, 1:] - rows).max(), np.abs(trace[:, 0] / costs - 1).max()
    print(f'SCALED_B group {start} {MODE_IDS[closed]}: parameters {dpar:.2e} cost {dcost:.2e}')
    assert dpar < (2e-4 if closed else 1e-5) and dcost < (1e-4 if closed else 1e-5), (dpar, dcost)
    for r, o in zip(rs, imgs):
        J = r.J().cpu().numpy()
        assert np.array_equal(np.isnan(J), np.isnan(o.J))
        assert helpers.rms_per_channel(J, o.J).max() < (1e-4 if closed else 1e-5)
        assert np.array_equal(r.params().cpu().numpy(), trace[-1, 1:].astype(np.float32))


@pytest.mark.parametrize('closed', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('start', list(STARTS))
def test_split_path_publishes_unscaled_sums(start, closed):
    """launch_fit_grad + launch_fit_step through engine.HipWaterBackend: what the host all-reduces keeps its meaning, sum r (1 - g).
    Every iteration's three sums are held to the oracle's AT THE ENGINE'S OWN PARAMETERS of that iteration (a second oracle image
    driven by them, so that the two trajectories' distance is not in the figure).  The bar: the sum adds n terms |r (1 - g)| <= |r|
    whose absolute values total at most sqrt(n sum r^2) = sqrt(n cost); float32 accumulation in any order and 1-ulp exponentials
    move it by sqrt(n) 2^-24 ~ 8e-6 of that total at n = 18 414: 1e-5 sqrt(n cost), which is 1e-5 .. 3e-4 of the sums themselves
    here.  B times the sum -- B is 0.1, -0.05 and the window's two edges in the starts that run the scaled form -- is nowhere near.
    (oracle.SharedWaterImage.grad returns dS/dB = -2 sum r (1 - g) for S = sum r^2: oracle/sucre_oracle.c.)"""
    from sucre_amd import engine
    r = _restoration()
    _load(r, _list_set(), _params0(start), _J0(closed))
    trace = torch.zeros((T, 10), dtype=torch.float64, device='cuda')
    be = engine.HipWaterBackend(r, use_closed_form=closed, trace=trace)
    total = be.n_obs()
    be.set_n_obs_total(total)
    got = []
    for it in range(1, T + 1):
        got.append(be.grad(it).cpu().numpy()[:10].copy())
        be.step(it)
    if closed:
        r.update_J()
    torch.cuda.synchronize()

    trace = trace.cpu().numpy()
    follower = oracle.SharedWaterImage(H, W, _list_set().samples(), None if closed else _J0(closed), use_closed_form=closed)
    for it in range(1, T + 1):
        at = _params0(start) if it == 1 else trace[it - 2, 1:].astype(np.float32)     # the parameters the engine's pass it ran with
        acc = follower.grad(at, it, total)
        want = -0.5 * acc[:3]
        bar = 1e-5 * np.sqrt(total * acc[9])
        err = np.abs(got[it - 1][:3] - want).max()
        print(f'SCALED_B split {start} {MODE_IDS[closed]} it {it}: sums {got[it - 1][:3]} oracle {want} distance {err:.2e} bar {bar:.2e}')
        assert err < bar, (start, it, got[it - 1][:3], want, err, bar)
        if it == 1 and scaled_b_ok(at[:3]):       # ... and B times the sum would have missed it (later sums may pass through 0)
            assert np.abs(at[:3].astype(np.float64) * want - want).min() > 10 * bar, (start, it)
    rows, costs, imgs = _oracle_lockstep(start, closed, (0,))
    assert np.abs(trace[:, 1:] - rows).max() < (2e-4 if closed else 1e-5)
    assert np.abs(trace[:, 0] / costs - 1).max() < (1e-4 if closed else 1e-5)
    J = r.J().cpu().numpy()
    assert np.array_equal(np.isnan(J), np.isnan(imgs[0].J))
    assert helpers.rms_per_channel(J, imgs[0].J).max() < (1e-4 if closed else 1e-5)


# ---- an observed pixel whose every a^2 underflows (fit.hip, closed_pass's strip end) ---------------------------------------------
def _underflow_list_set():
    """The store above with one pixel's observations -- the brightest colour -- at 600 m: a = exp(-0.1 * 600) = 2^-86.6 is an
    ordinary float32, a^2 is 0, so D = 0 and N = sum p a > 0 (p = 1 - B (1 - g) > 0 for either B below)."""
    if 'underflow' not in _CACHE:
        g = _geometry()
        p = int(np.argmax(g.count_map().reshape(-1) >= 5))
        z = g.z.copy()
        z[g.px == p] = 600.0
        g2 = crafted.Geometry(g.H, g.W, g.n_views, g.min_cover, g.view, g.px, z)
        rgb = crafted.random_colours(g2)
        rgb[g2.px == p] = 255
        _CACHE['underflow'] = (crafted.ListSet(g2, rgb=rgb), p)
    return _CACHE['underflow']


@pytest.mark.parametrize('B', [0.1, -0.05], ids=['positive', 'negative'])
def test_closed_form_overflow_is_handed_over(B):
    """The reference's J of that pixel is +inf, the iteration's cost inf, and all nine parameters (the pixel's three channels) are NaN
    from that iteration's step on -- in the scaled form too, where the strip end adds B dJ and the finisher divides by B."""
    from sucre_amd import engine
    ls, p = _underflow_list_set()
    p0 = np.full(9, 0.1, np.float32)
    p0[:3] = B
    assert scaled_b_ok(p0[:3])
    zero = np.zeros((H, W, 3), np.float32)
    Jo, po, to = oracle.fit(H, W, ls.samples(), None, params0=p0, num_iter=3, use_closed_form=True)
    assert to[0, 0] == np.inf and np.isnan(to[1:, 1:]).all()       # what the oracle (and the reference) do on this scene
    r = _restoration()
    _load(r, ls, p0, zero)
    tr = r.fit(3, use_closed_form=True).cpu().numpy()
    assert tr[0, 0] == np.inf, tr[:, 0]
    assert np.array_equal(np.isnan(tr), np.isnan(to)) and np.isnan(tr[1:, 1:]).all(), tr
    # the sums themselves, through the split path: dJ = N / 0 = +inf for either sign of B, and so is what is published
    r = _restoration()
    _load(r, ls, p0, zero)
    be = engine.HipWaterBackend(r, use_closed_form=True)
    be.set_n_obs_total(be.n_obs())
    sums = be.grad(1).cpu().numpy()
    assert np.all(sums[:3] == np.inf) and sums[9] == np.inf, sums
