"""Paired J-parameter iterations (csrc/fit.hip, 'Paired iterations'; ``engine.Restoration.fit(paired=...)``): ``sucre_fit_run``
takes its iterations two launches at a time, the pixels' Adam moments read and written once per pair.  The bar is BIT EQUALITY
with the one-launch-per-iteration form of the same build (``SUCRE_FIT_UNPAIRED``), from the same starting workspace contents:
the whole workspace outside the pair's gradient plane -- state block, the 27 parameter words, sums, partials, tickets, plans --,
``J()`` and the trace.  The stores are the hand-built count histograms of tests/crafted.py; one check at the golden fixtures
holds the paired form to the reference's numbers at the bars of tests/test_gpu_parity.py."""
import numpy as np
import pytest
import torch

import crafted
import helpers
from crafted import CASE, EngineBackend

pytestmark = pytest.mark.gpu

FORMATS = ('f32', 'f32plain', 'f32z26', 'u16mm')     # 24-bit codes (on narrow ranges), float32 words, 26-bit codes, uint16 mm
# tail only (eq1), three levels, exactly one full chunk (eq4), a full chunk + a tail (eq5), 64 distinct counts in a wave and a
# masked chunk in every strip (stair), levels = 64 next to full = 1 (heavy), strips of 0 .. 8 levels three to a wave, back to back
# (ragged: F's three start items follow the previous strip's stores at once)
SMALL = ('eq1', 'eq3', 'eq4', 'eq5', 'stair', 'heavy', 'ragged40x24', 'ragged80x16')
P_IN = np.full(9, 0.1, np.float32)                                   # B inside scaled_b_ok's window: the B-scaled pass
P_OUT = np.array([0.0, 0.1, 16.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1], np.float32)   # a zero and a 16: the whole launch runs the unscaled pass


def _unseen_geometry(narrow=False):
    """16x16: strips of 5, 4 (masked: 32 pixels have three), 1 and 0 levels -- the last one a strip nobody observes."""
    key = ('paired_unseen', narrow)
    if key not in crafted._GEOMS:
        cnt = np.concatenate([np.full(64, 5), np.full(32, 4), np.full(32, 3), np.full(64, 1), np.full(64, 0)])
        crafted._GEOMS[key] = crafted.build(16, 16, 8, cnt[np.random.default_rng(3).permutation(256)], seed=2, narrow=narrow)
    return crafted._GEOMS[key]


def _geometry(cid, fmt):
    """'f32' runs on the narrow ranges, where the default store must pick 24-bit codes; the other forms on the wide ones."""
    if cid == 'unseen':
        return _unseen_geometry(narrow=(fmt == 'f32'))
    return CASE[cid].geometry(narrow=(fmt == 'f32'))


def _loaded(g, fmt, p0, nan_unseen=True):
    """A restoration holding the store of ``g`` and a seeded J0 -- NaN where nobody observes the pixel -- and its workspace bytes."""
    from sucre_amd import engine
    r = engine.Restoration(g.H, g.W, g.n_views, obs_format=fmt)
    J0 = (3.0 + np.random.default_rng(11).random((g.H, g.W, 3))).astype(np.float32)
    if nan_unseen:
        J0[g.count_map() == 0] = np.nan
    EngineBackend(r)._load(r, crafted.ListSet(g, rgb=crafted.random_colours(g)), p0, J0)
    _, g_off, n_strips = _regions(r)
    r.ws[g_off:g_off + n_strips * 768] = 0xff    # the pair's gradient plane starts as NaNs: L writes a strip's before F reads it
    torch.cuda.synchronize()
    return r, r.ws.clone()


def _regions(r):
    from sucre_amd import _lib
    g_off = r.lib.sucre_ws_offset(r.H, r.W, r.n_views, _lib.WS_PAIR_GRADIENT)
    s_off = r.lib.sucre_ws_offset(r.H, r.W, r.n_views, _lib.WS_STATE)
    n_strips = 4 * ((r.H + 15) // 16) * ((r.W + 15) // 16)
    assert 0 < s_off < g_off and g_off + n_strips * 768 <= r.ws.numel()
    return s_off, g_off, n_strips


def _run(r, ws0, calls, paired, t0=0, lr=0.05):
    """The fit cut into ``calls`` from the workspace contents ``ws0`` at step ``t0`` -> (workspace outside the gradient plane, state
    block, 27 parameter words, J, trace), all as integers: NaNs compare by their bits."""
    from sucre_amd import _lib
    r.ws.copy_(ws0)
    r.steps_done = t0
    traces = [r.fit(T, lr=lr, paired=paired) for T in calls]
    torch.cuda.synchronize()
    assert r.steps_done == t0 + sum(calls)
    s_off, g_off, n_strips = _regions(r)
    ws = r.ws.cpu().numpy()
    outside = np.concatenate([ws[:g_off], ws[g_off + n_strips * 768:]])
    state = ws[s_off:s_off + n_strips * 2304].copy()
    params = r._region(_lib.WS_PARAMS, torch.float32, 27).cpu().numpy().view(np.uint32).copy()
    trace = torch.cat(traces).cpu().numpy().view(np.uint64) if traces else np.zeros((0, 10), np.uint64)
    return dict(outside=outside, state=state, params=params, J=r.J().cpu().numpy().view(np.uint32), trace=trace,
                gplane=ws[g_off:g_off + n_strips * 768].copy())


def _assert_same(a, b, label):
    for k in ('state', 'params', 'J', 'trace', 'outside'):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (label, k, int((a[k] != b[k]).sum()), 'words differ')


def _check_store(cid, fmt, Ts=(0, 1, 2, 3, 7), t0s=(0, 1), params=(P_IN, P_OUT)):
    g = _geometry(cid, fmt)
    for p0 in params:
        r, ws0 = _loaded(g, fmt, p0)
        assert int(r.store_format().cpu().numpy()[0]) == {'f32': 2, 'f32plain': 0, 'f32z26': 3, 'u16mm': 1}[fmt]
        s_off, _, n_strips = _regions(r)
        state0 = ws0[s_off:s_off + n_strips * 2304].cpu().numpy()
        for t0 in t0s:
            for T in Ts:
                one = _run(r, ws0, [T], False, t0)
                two = _run(r, ws0, [T], True, t0)
                _assert_same(one, two, (cid, fmt, 'B0', float(p0[0]), 't0', t0, 'T', T))
                assert np.array_equal(two['state'], state0) == (T == 0), (cid, fmt, T, 'T = 0 touches nothing; any other T moves the state')
                # the switch switches: only a call with a pair in it writes the gradient plane, and then every strip's
                assert (one['gplane'] == 0xff).all() and (two['gplane'] == 0xff).all() == (T < 2), (cid, fmt, T, 'gradient plane')
                if T >= 2:
                    assert not (two['gplane'].view(np.uint32) == 0xffffffff).any(), (cid, fmt, T, 'a strip without its gradient')
            # a fit cut into calls: nothing is pending between them, whatever the parity of the pieces
            whole = _run(r, ws0, [7], False, t0)
            _assert_same(whole, _run(r, ws0, [2, 3, 2], True, t0), (cid, fmt, 't0', t0, '2 + 3 + 2 paired'))
            _assert_same(whole, _run(r, ws0, [2, 3, 2], False, t0), (cid, fmt, 't0', t0, '2 + 3 + 2 unpaired'))


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('cid', ('unseen',) + SMALL)
def test_paired_fit_keeps_every_bit(cid, fmt):
    _check_store(cid, fmt)


@pytest.mark.parametrize('fmt', ('f32', 'u16mm'))
def test_paired_fit_keeps_every_bit_at_kmaxviews(fmt):
    """A strip of 4096 levels (1024 full chunks between F's start items and its end) next to strips of 0, 1, 15 .. 17 and 255."""
    _check_store('maxviews', fmt, Ts=(2, 3), t0s=(0,), params=(P_IN,))


def test_an_unobserved_strip_keeps_its_nan():
    """The strip nobody observes: its NaN J stays NaN through both launches of a pair, its moments decay as in single launches,
    and no NaN reaches a sum."""
    g = _unseen_geometry()
    r, ws0 = _loaded(g, 'f32plain', P_IN)
    out = _run(r, ws0, [4], True)
    J = out['J'].view(np.float32)
    unseen = g.count_map() == 0
    assert unseen.sum() == 64 and np.isnan(J[unseen]).all() and np.isfinite(J[~unseen]).all()
    assert np.isfinite(out['trace'].view(np.float64)).all()


def test_two_workspaces_on_two_streams():
    """Two images fitted at once, each on its own stream (what the benchmark's two images in flight do): each keeps the bits of
    its own unpaired fit."""
    ga, gb = CASE['stair'].geometry(), CASE['ragged40x24'].geometry()
    (ra, wa), (rb, wb) = _loaded(ga, 'f32plain', P_IN), _loaded(gb, 'f32plain', P_IN)
    want = [_run(ra, wa, [7], False), _run(rb, wb, [7], False)]
    ra.ws.copy_(wa); rb.ws.copy_(wb)
    ra.steps_done = rb.steps_done = 0
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    traces = {}
    for _ in range(2):     # 2 + 5 and 5 + 2: the pairs of the two images interleave differently
        for r, s, T in ((ra, sa, 2 if _ == 0 else 5), (rb, sb, 5 if _ == 0 else 2)):
            with torch.cuda.stream(s):
                traces.setdefault(id(r), []).append(r.fit(T, paired=True))
    torch.cuda.synchronize()
    for r, w in ((ra, want[0]), (rb, want[1])):
        got = torch.cat(traces[id(r)]).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, w['trace']) and np.array_equal(r.J().cpu().numpy().view(np.uint32), w['J']), 'two streams'


def test_paired_fit_on_the_persistent_grid():
    """The smallest image that gets the persistent grid and its weighted deal (5120 tiles: 1280 workgroups, 5120 waves of four
    strips on average): a matched 1280x1024 store of two neighbours, T = 3 (a pair and a single launch) against three single
    launches."""
    from sucre_amd import engine, synth
    scene = synth.make_scene(1280, 1024, 2, seed=4)
    views = engine.device_views_from_scene(scene, 'cuda')
    r = engine.Restoration(scene.height, scene.width, len(views))
    r.match(views[scene.target], views)
    r.fit_init(views[scene.target])
    torch.cuda.synchronize()
    ws0 = r.ws.clone()
    assert (scene.width // 16) * (scene.height // 16) == 5120
    _assert_same(_run(r, ws0, [3], False), _run(r, ws0, [3], True), 'persistent grid, T = 3')


def test_paired_fit_against_the_reference(golden):
    """200 iterations in pairs on the golden fixtures at the bars of tests/test_gpu_parity.py::test_fit_J_parameter_mode."""
    from sucre_amd import engine
    scene = golden.scene
    views = engine.device_views_from_scene(scene, 'cuda')
    r = engine.Restoration(scene.height, scene.width, len(views))
    r.match(views[scene.target], views)
    r.fit_init(views[scene.target])
    trace = r.fit(200, paired=True).cpu().numpy()
    J, params, ref = r.J().cpu().numpy(), r.params().cpu().numpy(), golden['J_param_200']
    assert np.array_equal(np.isnan(J), np.isnan(ref))
    assert helpers.rms_per_channel(J, ref).max() < 1e-4
    assert np.abs(trace[:, 1:] - golden['trace_param'][:200, 1:]).max() < 1e-4
    assert np.abs(trace[:, 0] / golden['trace_param'][:200, 0] - 1).max() < 1e-4
    assert np.allclose(params, trace[-1, 1:], rtol=0, atol=0)
