"""Host tests of the direct solve of the mosaic's gain compensation: ``engine.mosaic_gain_solve_direct`` on hand-built matrices, the
chain of tests/mosaic_gain_direct_crafted.py through the restatement (the property the feature exists for, checked against
tests/mosaic_gain_direct_ref.py and not against the code under test), the restatement against plain loops over the definition, the
option checks and every refusal of the command line.  No GPU.
"""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_gain_direct_crafted as chain
import mosaic_gain_direct_ref as dref
import mosaic_gains_ref as gref
from sucre_amd import _lib, engine, sucre
from test_mosaic_gains_host import answer, small_survey

MU = engine.MOSAIC_GAIN_PRIOR


def system(n, cells):
    """``(pairs (n, n, 4), diag (n, 4))`` of flat images: ``cells``: a list of {image: (count, X)} -- per cell the samples and
    the one quantised colour, in all three channels, of every image that reaches it; exact integers (the quotients divide)."""
    pairs, diag = np.zeros((n, n, 4), np.int64), np.zeros((n, 4), np.int64)
    for held in cells:
        N = sum(k for k, _ in held.values())
        for i, (ki, xi) in held.items():
            diag[i, 0] += ki
            diag[i, 1:4] += ki * xi * xi
            for j, (kj, xj) in held.items():
                if i <= j:
                    assert (ki * xi * kj * xj) % N == 0
                    pairs[i, j, :3] += ki * xi * kj * xj // N
                    pairs[i, j, 3] += 1
    return pairs, diag


RESIDUAL = 1e-12     # |row of (A + mu diag Q) g - mu Q| / Q_i: LAPACK is backward stable, so this is a few float64 roundings of
#                      entries of size Q_i against gains of size 1 -- 2^-53 times a small multiple of n <= 4


def unclamped(pairs, diag, c=0, channels=(0, 1, 2), prior=MU):
    """Channel ``c`` of the ENGINE's solution before gauge and clamp (``engine.mosaic_gain_direct_unclamped``), after checking
    that it solves the normal equations in every channel of ``channels``: ``dref.residual``, built from the integers by the
    restatement, over the images with n > 0 and Q > 0."""
    x, kept = engine.mosaic_gain_direct_unclamped(pairs, diag, prior)
    assert x.dtype == np.float64 and x.shape == (len(diag), 3) and not set(kept) & set(channels)
    for ch in channels:
        act = (np.asarray(diag)[:, 0] > 0) & (np.asarray(diag)[:, 1 + ch] > 0)
        assert bool(np.isfinite(x[act, ch]).all()) and bool(np.isnan(x[~act, ch]).all()), ch
        worst = dref.residual(pairs, diag, np.nan_to_num(x[:, ch]), ch, prior)
        assert worst < RESIDUAL, (ch, worst)
    return x[:, c].tolist()


def follows(got, pairs, diag, G, L, kept=()):
    """The engine's gains ARE its unclamped solution after the gauge and the clamp: per channel not in ``kept``, over the images with
    n > 0, ``float32(min(max(g_i / s, 1 / L), L))`` with ``s`` the n-weighted mean and ``g_i`` the old gain where the solve has none."""
    x, _ = engine.mosaic_gain_direct_unclamped(pairs, diag)
    n = np.asarray(diag)[:, 0].astype(np.float64)
    for c in range(3):
        if c in kept:
            continue
        g = np.where(np.isnan(x[:, c]), np.asarray(G, np.float64)[:, c], x[:, c])
        s = float((n * g).sum() / n.sum())
        want = np.clip(g / s, 1.0 / L, L)
        live = n > 0
        assert np.allclose(np.asarray(got, np.float64)[live, c], want[live], rtol=2.0 ** -22, atol=0), c


# ---- the solve on hand-built matrices ----------------------------------------------------------------------------------------------

def test_two_images_that_agree_after_a_gain_of_two():
    pairs, diag = system(2, [{0: (4, 8192), 1: (4, 4096)}] * 10)
    got, kept = engine.mosaic_gain_solve_direct(pairs, diag, np.ones((2, 3), np.float32), 16.0)
    assert got.dtype == np.float32 and got.shape == (2, 3) and kept == []
    assert np.allclose(got[1].astype(np.float64) / got[0], 2.0, rtol=1e-5)                   # the prior's share: mu-sized
    assert np.allclose((got[0].astype(np.float64) + got[1]) / 2, 1.0, atol=1e-6)              # the gauge: equal overlap
    g = unclamped(pairs, diag)                                                                # the engine's, residual checked
    assert abs(g[1] / g[0] - 2.0) < 1e-5
    follows(got, pairs, diag, np.ones((2, 3)), 16.0)
    want, _ = dref.solve(pairs, diag, np.ones((2, 3), np.float32), 16.0)
    assert np.abs(got.astype(np.float64) / want - 1).max() <= 2.0 ** -20


def test_two_disconnected_pairs_are_each_pulled_towards_one():
    cells = [{0: (2, 8192), 1: (2, 4096)}] * 6 + [{2: (3, 3000), 3: (3, 9000)}] * 4
    pairs, diag = system(4, cells)
    assert engine.mosaic_gain_groups(pairs, diag) == 2 == dref.components(pairs, diag)
    got, kept = engine.mosaic_gain_solve_direct(pairs, diag, np.ones((4, 3), np.float32), 16.0)
    assert kept == []
    g = got.astype(np.float64)
    assert np.allclose(g[1] / g[0], 2.0, rtol=1e-5) and np.allclose(g[2] / g[3], 3.0, rtol=1e-5)
    # Within a group the prior fixes the level: with v the gains that make the group agree, v^T A = 0, so the normal equations
    # leave sum v_i Q_i (g_i - 1) = 0 -- each group has a gain above 1 and one below, whatever the other group does
    assert g[0, 0] < g[1, 0] and g[3, 0] < g[2, 0]
    u = unclamped(pairs, diag)
    assert u[0] < 1 < u[1] and u[3] < 1 < u[2]
    for group, v in (((0, 1), (1.0, 2.0)), ((2, 3), (3.0, 1.0))):
        assert abs(sum(w * float(diag[i, 1]) * (u[i] - 1) for i, w in zip(group, v))) / float(diag[group[0], 1]) < 1e-6
    follows(got, pairs, diag, np.ones((4, 3)), 16.0)
    want, _ = dref.solve(pairs, diag, np.ones((4, 3), np.float32), 16.0)
    assert np.abs(g / want - 1).max() <= 2.0 ** -20


def test_an_image_without_colour_or_without_overlap_keeps_the_gain_it_had():
    cells = [{0: (3, 9216), 1: (3, 4608), 2: (3, 0)}] * 6           # image 2: X = 0 everywhere, Q = 0; image 3: no shared cell
    pairs, diag = system(4, cells)
    assert diag[2].tolist() == [18, 0, 0, 0] and diag[3].tolist() == [0, 0, 0, 0]
    G = np.array([[1, 1, 1], [1, 1, 1], [1.5, 1.5, 1.5], [0.75, 0.75, 0.75]], np.float32)
    got, kept = engine.mosaic_gain_solve_direct(pairs, diag, G, 16.0)
    assert kept == [] and got[3].tolist() == [0.75] * 3                                          # untouched: outside the gauge too
    want, _ = dref.solve(pairs, diag, G, 16.0)
    assert np.abs(got.astype(np.float64) / want - 1).max() <= 2.0 ** -20
    # image 2 enters the gauge with the gain it had: g_2 / s with s the n-weighted mean over images 0, 1, 2.  (Its black samples
    # pull every cell's mean down, so the two other gains fall until the prior holds them -- and the clamp catches them.)
    u = unclamped(pairs, diag)                                          # the residual over the active images 0 and 1
    assert np.isnan(u[2]) and np.isnan(u[3])
    follows(got, pairs, diag, G, 16.0)
    s = (18 * u[0] + 18 * u[1] + 18 * 1.5) / 54
    assert got[2, 0] == np.float32(1.5 / s) and got[0, 0] == np.float32(max(u[0] / s, 1 / 16.0)) and 0 < u[0] < u[1]


def test_a_channel_without_a_solution_keeps_its_gains_and_is_reported():
    pairs, diag = system(2, [{0: (4, 8192), 1: (4, 4096)}] * 10)
    G = np.array([[1.25, 1, 1], [0.8, 1, 1]], np.float32)
    bad = pairs.copy()
    bad[0, 1, 0] = -bad[0, 1, 0]                  # channel R: the images pull apart -- a negative gain solves it
    got, kept = engine.mosaic_gain_solve_direct(bad, diag, G, 16.0)
    assert kept == [0] and got[:, 0].tolist() == G[:, 0].tolist()
    assert np.allclose(got[1, 1:].astype(np.float64) / got[0, 1:], 2.0, rtol=1e-5)
    assert dref.solve(bad, diag, G, 16.0)[1] == [0]
    x, k = engine.mosaic_gain_direct_unclamped(bad, diag)
    assert k == [0] and bool(np.isnan(x[:, 0]).all())
    unclamped(bad, diag, 1, channels=(1, 2))                              # the residual on the two channels that do solve
    follows(got, bad, diag, G, 16.0, kept=[0])
    sing = pairs.copy()
    sing[:, :, 1] = 0
    d0 = diag.copy()
    d0[:, 2] = 0                                  # channel G: Q = 0 for every image -- nothing to solve, nothing to report
    got, kept = engine.mosaic_gain_solve_direct(sing, d0, G, 16.0, prior=0.0)
    assert 1 not in kept and got[:, 1].tolist() == [1.0, 1.0]
    # without the prior A is singular exactly because the images can be made to agree: LAPACK raises or returns no finite positive
    # gain, or a solution of the consistent singular system; never an exception of ours
    assert set(kept) <= {0, 2} and bool(np.isfinite(got).all()) and bool((got > 0).all())


def test_the_clamp_and_the_limit_of_one():
    pairs, diag = system(3, [{0: (3, 12288), 1: (3, 3072), 2: (3, 6144)}] * 5)       # gains 1 : 4 : 2
    ones = np.ones((3, 3), np.float32)
    free, _ = engine.mosaic_gain_solve_direct(pairs, diag, ones, 16.0)
    assert np.allclose(free[1].astype(np.float64) / free[0], 4.0, rtol=1e-5)
    unclamped(pairs, diag)                                                # the residual of the L = 16 solve: nothing is clamped there
    follows(free, pairs, diag, ones, 16.0)
    assert bool((free > 1 / 16.0).all()) and bool((free < 16.0).all())
    got, _ = engine.mosaic_gain_solve_direct(pairs, diag, ones, 1.5)
    assert got[0].tolist() == [float(np.float32(1 / 1.5))] * 3 and got[1].tolist() == [1.5] * 3 and 1 / 1.5 < got[2, 0] < 1.5
    one, _ = engine.mosaic_gain_solve_direct(pairs, diag, ones, 1.0)
    assert one.tolist() == [[1.0] * 3] * 3
    none, kept = engine.mosaic_gain_solve_direct(np.zeros((2, 2, 4), np.int64), np.zeros((2, 4), np.int64), ones[:2] * 2, 2.0)
    assert none.tolist() == [[2.0] * 3] * 2 and kept == []                                        # nothing shared: nothing moves


# ---- the chain: what the feature exists for ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def chain_case():
    views, Js = chain.survey()
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * chain.N)
    return views, Js, gsd, dref.gains(views, Js, torch.eye(3), gsd, 1, chain.LIMIT)


def test_one_direct_solve_removes_the_drift_that_eight_rounds_leave(chain_case):
    views, Js, gsd, got = chain_case
    assert float(gsd) == float(np.float32(chain.GSD)) and min(float(J.min()) for J in Js) >= 0.25
    cells = got['pairs'][:, :, 3]
    assert [int(cells[i, i + 1]) for i in range(chain.N - 1)] == [384] * (chain.N - 1)            # only neighbours overlap
    assert int(np.triu(cells, 2).sum()) == 0 and got['excluded'] == 0 and dref.components(got['pairs'], got['diag']) == 1
    before, direct = chain.spread(got['tables'][0]), chain.spread(got['direct'])
    rounds = chain.spread(gref.gains(views, Js, torch.eye(3), gsd, 8, chain.LIMIT)['gains'])
    print(f'chain: spread {before:.6g}; after 8 rounds {rounds:.6g}; after one direct solve {direct:.6g} (bound {chain.BOUND:.6g}); '
          f'rms {got["rms"][0].tolist()} -> {got["rms"][1].tolist()}')
    assert abs(before - (chain.RATIO ** (chain.N - 1) - 1)) < 1e-6
    assert direct <= chain.BOUND
    assert rounds > chain.ROUNDS_LEFT
    assert got['kept'] == [] and bool((got['rms'][1] < got['rms'][0] / 100).all())
    # the engine's solve on the restatement's integers: LAPACK on both sides
    mine, kept = engine.mosaic_gain_solve_direct(got['pairs'], got['diag'], got['tables'][0], chain.LIMIT)
    assert kept == [] and np.abs(mine.astype(np.float64) / got['direct'] - 1).max() <= 2.0 ** -20


def test_the_prior_costs_less_than_the_bound_leaves_room_for(chain_case):
    *_, got = chain_case
    ones = got['tables'][0]
    weak, _ = dref.solve(got['pairs'], got['diag'], ones, chain.LIMIT, prior=2.0 ** -30)
    share = abs(chain.spread(got['direct']) - chain.spread(weak))
    print(f'chain: the prior\'s share of the spread {share:.3g}')
    assert share < 1e-4


# ---- the restatement against plain loops ----------------------------------------------------------------------------------------------

def test_the_restatement_equals_plain_loops_over_the_definition():
    views, Js = small_survey()
    axes, gsd = torch.eye(3), 0.2
    st = dref.state(views, Js, axes, gsd)
    per_cell, over, pairs, diag = dref.loops(views, Js, axes, gsd, st['base'])
    assert np.array_equal(pairs, st['pairs']) and np.array_equal(diag, st['diag']) and not over and st['excluded'] == 0
    shared = st['span'][:, 0] < st['span'][:, 1]
    assert sorted(per_cell) == np.nonzero(shared)[0].tolist() and shared.any()
    for cell, held in per_cell.items():
        k = len(held)
        assert st['slot_ord'][cell, :k].tolist() == sorted(held) and bool((st['slot_ord'][cell, k:] == dref.FREE).all())
        assert st['slot_sum'][cell, :k].tolist() == [held[i] for i in sorted(held)]
    assert bool((st['slot_ord'][~shared] == dref.FREE).all()) and not st['slot_sum'][~shared].any()
    assert pairs[1, 3, 3] > 0 and not np.tril(pairs[:, :, 3], -1).any() and diag[4].tolist() == [0] * 4      # a view twice; one far away
    assert np.array_equal(diag[:, 0], gref.gains(views, Js, axes, gsd, 0)['overlap'])               # no overflow: the rounds' overlap


def test_the_overflow_rule_counts_different_images():
    views, Js = small_survey()
    views, Js = [views[0]] * 9 + [views[4]], [Js[0]] * 9 + [Js[4]]
    st = dref.state(views, Js, torch.eye(3), 0.2)
    per_cell, over, pairs, diag = dref.loops(views, Js, torch.eye(3), 0.2, st['base'])
    shared = st['span'][:, 0] < st['span'][:, 1]
    assert st['excluded'] == int(shared.sum()) == len(over) > 0 and not pairs.any() and not diag.any()
    assert not st['pairs'].any() and not st['diag'].any()
    st8 = dref.state(views[1:], Js[1:], torch.eye(3), 0.2)
    assert st8['excluded'] == 0 and int(st8['pairs'][0, 7, 3]) == int(shared.sum())


# ---- the options, the refusals and the keyword's place ----------------------------------------------------------------------------------

def test_the_solve_is_checked_like_the_other_values():
    assert engine.MOSAIC_GAIN_SOLVES == ('rounds', 'direct') and engine.MOSAIC_GAIN_PRIOR == 2.0 ** -20
    assert _lib.MOSAIC_GAIN_CELL_IMAGES == 8 == dref.SLOTS
    def checked(gain_solve, gains, who):
        return engine.MosaicOptions(gain_solve=gain_solve, gains=gains).checked(who).gain_solve
    assert checked(None, None, 'x') is None and checked(None, 3, 'x') is None
    assert checked('rounds', 3, 'x') is None and checked('direct', 3, 'x') == 'direct'
    for bad in ('Direct', 'exact', '', 1, True, 2.5):
        with pytest.raises(ValueError, match='mosaic gain solve must be one of rounds or direct') as e:
            checked(bad, 3, 'x')
        assert e.value.field == 'gain_solve'
    for solve in ('rounds', 'direct'):
        with pytest.raises(ValueError, match=r'who: the solve finds the gains of the first round.*\(gains=R\)') as e:
            checked(solve, None, 'who')
        assert e.value.field == 'gain_solve'
    view = SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')))
    for kw, who in ((dict(gains=2, gain_solve='exact'), 'must be one of'), (dict(gain_solve='direct'), 'mosaic_of: the solve finds')):
        with pytest.raises(ValueError, match=who) as e:       # before a Mosaic is made
            engine.mosaic_of([view], [None], torch.eye(3), 0.1, **kw)
        assert e.value.field == 'gain_solve'
    assert list(inspect.signature(sucre.mosaic).parameters)[-1] == 'gain_solve'      # a new keyword, placed last
    assert inspect.signature(sucre.mosaic).parameters['gain_solve'].default is None
    for f in (engine.mosaic_of, engine.Mosaic.run, engine.Mosaic.begin):      # these take it as a field of the record, and no other name
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.kind is inspect.Parameter.VAR_KEYWORD and 'options' in inspect.signature(f).parameters
    assert engine.MosaicOptions().gain_solve is None and engine.MosaicOptions().over(gain_solve='direct').gain_solve == 'direct'
    with pytest.raises(TypeError):
        engine.MosaicOptions().over(gain_solver='direct')
    with pytest.raises(TypeError):
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, gain_solver='direct')
    assert engine.MOSAIC_VALUES['gain_solve'] == ('gain solve', ('rounds', 'direct'), None, None, str, 'S', None)
    for name in ('sucre_mosaic_gain_slots', 'sucre_mosaic_gain_pairs', 'sucre_mosaic_gain_diag'):
        assert name in _lib.SIGNATURES
    for name in ('add_gain_slots', 'gain_pairs', 'add_gain_diag', 'solve_gains_direct'):
        assert callable(getattr(engine.Mosaic, name))
    assert not any('gain' in k for k in engine.MOSAIC_OUTPUTS) and sucre._MOSAIC_FLAG['gain_solve'] == '--mosaic-gain-solve'


def test_the_command_line_refuses_before_any_file_is_opened(monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    lone = '--mosaic-gain-solve: only with --mosaic-gains R'
    assert answer(['--mosaic-gain-solve', 'direct']) == lone
    assert answer(['--mosaic', 'results', '--mosaic-gain-solve', 'direct']) == lone
    assert answer(['--mosaic', 'results', '--mosaic-gain-solve', 'rounds']) == lone
    assert answer(['--mosaic-gains', '3', '--mosaic-gain-solve', 'direct']) == '--mosaic-gains: only with --mosaic DIR'
    for bad in ('exact', 'Direct', '1'):
        assert answer(['--mosaic', 'results', '--mosaic-gains', '3', '--mosaic-gain-solve', bad]) == \
            f'--mosaic-gain-solve: S must be rounds or direct, not {bad}'
    for good in (['--mosaic-gain-solve', 'direct'], ['--mosaic-gain-solve', 'rounds'],
                 ['--mosaic-gain-solve', 'direct', '--mosaic-gain-limit', '4', '--mosaic-surface', '0.05', '--mosaic-blend', '0.5']):
        assert answer(['--mosaic', 'results', '--mosaic-gains', '1'] + good) == 'accepted', good


def test_the_python_entry_refuses_like_the_command_line(monkeypatch):
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda device, what: None)
    image = SimpleNamespace(name='a.png')
    for kw, code in ((dict(gain_solve='direct'), '--mosaic-gain-solve: only with --mosaic-gains R'),
                     (dict(gains=2, gain_solve='exact'), "--mosaic-gain-solve: mosaic gain solve must be one of rounds or direct, not 'exact'")):
        with pytest.raises(SystemExit) as e:
            sucre.mosaic([image], None, 'results', 'out', **kw)
        assert e.value.code == code, kw


def test_the_groups_and_the_matrix_are_those_of_the_definition():
    rng = np.random.default_rng(5)
    n = 40
    pairs = np.zeros((n, n, 4), np.int64)
    for i, j in rng.integers(0, n, (25, 2)):
        pairs[min(i, j), max(i, j)] = rng.integers(1, 1 << 60, 4)
    pairs[np.tril_indices(n, -1)] = -7                                     # whatever lies below the diagonal is not read
    diag = np.zeros((n, 4), np.int64)
    diag[rng.random(n) < 0.8] = 5
    assert engine.mosaic_gain_groups(pairs, diag) == dref.components(pairs, diag) > 1
    for w in range(4):
        M = engine.mosaic_gain_pair_matrix(pairs, w)
        assert M.dtype == np.float64 and np.array_equal(M, M.T)
        assert all(M[i, j] == float(int(pairs[min(i, j), max(i, j), w])) for i in range(n) for j in range(n))
