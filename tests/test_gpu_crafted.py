"""The HIP engine on the hand-built count histograms of tests/crafted.py: compaction (compact.hip), item plans (plan_kernel) and
the per-wave item stream, held to identities that are exact small-integer arithmetic and to the float64 model of
tests/model64.py at ``GPU_FACTOR`` x the CPU oracle's own distance from it (``Case.D``; tests/test_crafted_host.py pins those).
One lost, duplicated or misplaced observation anywhere in a store fails an identity by name: case, store form, round, pixel, count.

Every test prints what it measured (``pytest -s``): the engine's distances next to the bars."""
import time

import numpy as np
import pytest
import torch

import crafted
from crafted import CASE, CASES, GPU_FACTOR, EngineBackend
from oracle import oracle

pytestmark = pytest.mark.gpu

SMALL = [c.id for c in CASES if c.id != 'maxviews']      # 'maxviews' is its own test
FORMATS = ('f32', 'f32plain', 'f32z26', 'u16mm')
BATCHED = ('stair', 'ragged40x24', 'ragged80x16')          # check (b) also through fit_batch and a HipWaterGroup

# The one bar above GPU_FACTOR x D: the J-parameter COST of 'maxviews'.  A lane of fit.hip keeps its share of sum r^2 in ONE
# float32 register across all its strips (Acc::cost, grad_terms: fma(r, r, cost)), where the oracle and the float64 model add
# in double; with 4096 levels x 3 channels that is a running float32 sum of L = 12288 terms of one sign, whose rounding errors
# walk to sqrt(L) u of the sum (u = 2^-24; L u in the worst case) -- 6.6e-6 relative for a lane, less over the 64 lanes of the
# heavy strip, whose errors are independent.  Measured: 1.7e-7 (24-bit codes) and 5.8e-7 (uint16 mm) against D = 2.8e-8, which
# is small on this case BECAUSE the oracle's double sum over 815 520 terms has no such term.  The hardware forms of
# fit_math.h (exp2, and the reciprocal and square root of J's step) are not what shows here: J and the parameters hold
# GPU_FACTOR x D on this case too, and every other case -- at most 300 levels -- holds it on the cost.  A lost observation
# is check (b)'s to catch, exactly; this bar guards the arithmetic.
COST_BAR = {'maxviews': (3 * 4096) ** 0.5 * 2.0 ** -24}


def _store(fmt):
    from sucre_amd import _lib
    return {'f32': _lib.STORE_Z24, 'f32plain': _lib.STORE_F32, 'f32z26': _lib.STORE_Z26, 'u16mm': _lib.STORE_U16MM}[fmt]


def _restoration(g, **kw):
    from sucre_amd import engine
    return engine.Restoration(g.H, g.W, g.n_views, **kw)


def _geometry(case, fmt):
    """'f32' runs on the narrow ranges, where the default store must pick 24-bit codes; the other forms on the wide ones."""
    return case.geometry(narrow=(fmt == 'f32'))


def _closed_form(case, fmt, rounds=None):
    g = _geometry(case, fmt)
    t = time.perf_counter()
    d = crafted.check_closed_form(g, EngineBackend(_restoration(g, obs_format=fmt)), GPU_FACTOR * case.D['R'], (case.id, fmt),
                                  quantize=(fmt == 'u16mm'), rounds=rounds, store_format=_store(fmt))
    print(f'CRAFTED {case.id} (a) {fmt}: R {d:.2e} (bar {GPU_FACTOR * case.D["R"]:.1e}) {time.perf_counter() - t:.2f} s')


def _closed_form_float(case):
    g = case.geometry()
    t = time.perf_counter()
    d = crafted.check_closed_form_float(g, EngineBackend(_restoration(g, float_colour=True)), GPU_FACTOR * case.D['R'], (case.id, 'float colour'))
    print(f'CRAFTED {case.id} (a) float colour: R {d:.2e} (bar {GPU_FACTOR * case.D["R"]:.1e}) {time.perf_counter() - t:.2f} s')


def _trajectories(case, fmt):
    g = _geometry(case, fmt)
    for closed in ((False, True) if case.closed else (False,)):
        t = time.perf_counter()
        D = dict(case.D)
        if not closed and case.id in COST_BAR:
            D['cost'] = max(D['cost'], COST_BAR[case.id] / GPU_FACTOR)
        dJ, dpar, dcost = crafted.check_trajectory(g, EngineBackend(_restoration(g, obs_format=fmt)), D, (case.id, fmt), closed=closed,
                                                   quantize=(fmt == 'u16mm'), factor=GPU_FACTOR)
        k = ('cJ', 'cpar', 'ccost') if closed else ('J', 'par', 'cost')
        print(f'CRAFTED {case.id} (c) {fmt} {"closed form" if closed else "J-parameter"}: J {dJ:.2e} ({GPU_FACTOR * case.D[k[0]]:.1e}) '
              f'parameters {dpar:.2e} ({GPU_FACTOR * case.D[k[1]]:.1e}) cost {dcost:.2e} ({GPU_FACTOR * D[k[2]]:.1e}) {time.perf_counter() - t:.2f} s')


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('cid', SMALL)
def test_closed_form_is_exact(cid, fmt):
    """Check (a) on the uint8-colour store in each of its four forms."""
    _closed_form(CASE[cid], fmt)


@pytest.mark.parametrize('cid', SMALL)
def test_closed_form_is_exact_on_float_colours(cid):
    _closed_form_float(CASE[cid])


@pytest.mark.parametrize('fmt', ('f32', 'f32plain', 'u16mm'))
@pytest.mark.parametrize('cid', SMALL)
def test_cost_is_exact(cid, fmt):
    """Check (b) through ``fit``."""
    g = _geometry(CASE[cid], fmt)
    crafted.check_cost(g, EngineBackend(_restoration(g, obs_format=fmt)), (cid, fmt))


@pytest.mark.parametrize('cid', BATCHED)
def test_cost_is_exact_in_a_batch_and_in_a_group(cid):
    """Check (b) through the item loops of the batch and group kernels: ``fit_batch`` over two different cases of one size (in
    either position of the launch) and a ``HipWaterGroup`` of one."""
    g = CASE[cid].geometry()
    g2 = crafted.partner_geometry(CASE[cid])
    rgb2 = np.zeros((len(g2.view), 3), np.uint8)
    rgb2[:, 0] = 255
    for slot in (0, 1):
        r2 = _restoration(g2)
        crafted.check_cost(g, EngineBackend(_restoration(g), 'batch', partner=(r2, crafted.ListSet(g2, rgb=rgb2)), slot=slot), (cid, 'batch', slot))
        assert int(r2.trace.cpu().numpy()[0, 0]) == g2.n_obs and r2.n_obs() == g2.n_obs    # the other image of the launch
        assert np.array_equal(r2.residuals()[0].cpu().numpy(), g2.count_map())
    crafted.check_cost(g, EngineBackend(_restoration(g), 'group'), (cid, 'group'))


@pytest.mark.parametrize('fmt', ('f32', 'u16mm'))
@pytest.mark.parametrize('cid', SMALL)
def test_trajectories_against_float64(cid, fmt):
    """Check (c): J-parameter mode, and closed form on every case that has such a trajectory."""
    _trajectories(CASE[cid], fmt)


def test_maxviews():
    """kMaxViews = 4096 views of a 16x16 image, every kind of check.  An import of 4096 views is 12 288 launches, 0.15 s: all 13
    rounds of check (a) on the four forms of the uint8-colour store would be 8 s of the 10 s this test may take next to its
    other checks.  The default store (24-bit codes) runs all 13; the other three forms the rounds {0, 5, 12} (the lowest bit,
    one in the middle, the bit that only view 4095 sets in view + 1); the float-colour store its full round."""
    case = CASE['maxviews']
    t = time.perf_counter()
    for fmt in FORMATS:
        _closed_form(case, fmt, rounds=None if fmt == 'f32' else crafted.SPARSE_ROUNDS)
    _closed_form_float(case)
    for fmt in ('f32', 'f32plain', 'u16mm'):
        g = _geometry(case, fmt)
        crafted.check_cost(g, EngineBackend(_restoration(g, obs_format=fmt)), (case.id, fmt))
    for fmt in ('f32', 'u16mm'):
        _trajectories(case, fmt)
    print(f'CRAFTED maxviews: {time.perf_counter() - t:.1f} s')


def test_results_do_not_depend_on_what_the_workspace_held():
    """Check (a)'s J of 'stair' from a workspace that has just held 'maxviews', and the reverse: the bits of a fresh workspace."""
    gs, gm = CASE['stair'].geometry(), CASE['maxviews'].geometry()
    zero = np.zeros((16, 16, 3), np.float32)

    def J(r, g, j):
        return EngineBackend(r)(crafted.ListSet(g, rgb=crafted.round_colours(g, j)), crafted.PARAMS_A, zero, T=0).J
    for j in (0, 8):
        fresh_s, fresh_m = J(_restoration(gs), gs, j), J(_restoration(gm), gm, j)
        r = _restoration(gm)
        assert np.array_equal(J(r, gm, j).view(np.uint32), fresh_m.view(np.uint32))
        assert np.array_equal(J(r, gs, j).view(np.uint32), fresh_s.view(np.uint32)), ('stair after maxviews', j)
        assert np.array_equal(J(r, gm, j).view(np.uint32), fresh_m.view(np.uint32)), ('maxviews after stair', j)


@pytest.mark.parametrize('closed', [False, True], ids=['J-parameter', 'closed-form'])
@pytest.mark.parametrize('cid', ['stair', 'straddle'])
def test_light_model(cid, closed):
    """The light model's own store (camera points in the extension planes, x and y != 0) on two of the histograms, T = 3, against
    ``oracle.fit_light`` at the bars of tests/test_gpu_parity.py::test_light_model_vs_oracle_short."""
    import helpers
    g = CASE[cid].geometry(light=True)
    ls = crafted.ListSet(g, rgb=crafted.random_colours(g))
    J0 = np.random.default_rng(13).random((g.H, g.W, 3)).astype(np.float32)
    r = _restoration(g, light=True)
    tgt = crafted.target_view(g.H, g.W)
    r.import_matches(tgt, crafted.device_lists(ls, 'cuda', 'points'), min_cover=g.min_cover)
    r.fit_init(tgt, J0=torch.from_numpy(J0).cuda())
    trace = r.fit(3, use_closed_form=closed).cpu().numpy()
    J, params = r.J().cpu().numpy(), r.params().cpu().numpy()
    Jo, po, to = oracle.fit_light(g.H, g.W, ls.samples(), None if closed else J0, num_iter=3, use_closed_form=closed)
    assert r.n_obs() == g.n_obs
    dcost, dpar, dlight = abs(trace[0, 0] / to[0, 0] - 1), np.abs(trace[:, 1:10] - to[:, 1:10]).max(), np.abs(trace[:, 10:] - to[:, 10:]).max()
    assert np.array_equal(np.isnan(J), np.isnan(Jo))
    rms = helpers.rms_per_channel(J, Jo).max()
    print(f'CRAFTED {cid} light {"closed form" if closed else "J-parameter"}: cost {dcost:.2e} parameters {dpar:.2e} light {dlight:.2e} rms(J) {rms:.2e}')
    assert dcost < 1e-6
    assert dpar < 2e-5
    assert dlight < 1e-3
    assert rms < 2e-5
    assert np.array_equal(params, trace[-1, 1:].astype(np.float32))
