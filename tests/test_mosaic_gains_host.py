"""Host tests of the mosaic's per-image gain compensation: the solve on hand-built sums, the option checks, every refusal of the
command line, the pinned tables, and the self-checks of tests/mosaic_gains_ref.py (the yardstick of test_gpu_mosaic_gains.py)
against plain loops over the definition.  No GPU.
"""
import dataclasses
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_gains_crafted as crafted
import mosaic_gains_ref as gref
import mosaic_ref as ref
from sucre_amd import _lib, engine, sucre

NAN = float('nan')


def sums_row(n, A, B, R2=(0, 0, 0)):
    return [n, *A, *B, *R2]


# ---- the solve ----------------------------------------------------------------------------------------------------------------------

def test_solve_an_image_without_overlap_keeps_exactly_one():
    sums = [sums_row(100, (50, 60, 70), (100, 100, 100)), sums_row(0, (0, 0, 0), (0, 0, 0)), sums_row(100, (200, 150, 110), (100, 100, 100))]
    G = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    got = engine.mosaic_gain_solve(sums, G, 16.0)
    assert got.dtype == np.float32 and got.shape == (3, 3)
    assert got[1].tolist() == [1.0, 1.0, 1.0]
    # the gauge: the overlap-weighted mean of the unrounded gains is 1; g0 : g2 = A0/B0 : A2/B2
    assert np.allclose(got[0] / got[2], [0.25, 0.4, 70 / 110], rtol=1e-6)
    assert np.allclose((100 * got[0].astype(np.float64) + 100 * got[2]) / 200, 1.0, atol=1e-7)
    assert np.array_equal(got, gref.solve(sums, G, 16.0))


def test_solve_a_non_positive_sum_keeps_the_old_gain():
    G = np.array([[1.5, 0.75, 1.0], [1.0, 1.0, 1.0]], np.float32)
    sums = [sums_row(10, (0, -5, 30), (40, 40, 0)), sums_row(30, (40, 40, 40), (40, 40, 40))]
    got = engine.mosaic_gain_solve(sums, G, 16.0)
    for c in range(3):      # image 0 enters the gauge with its old gain, image 1 with 1
        s = (10 * float(G[0, c]) + 30 * 1.0) / 40
        assert got[0, c] == np.float32(float(G[0, c]) / s) and got[1, c] == np.float32(1.0 / s), c
    assert np.array_equal(got, gref.solve(sums, G, 16.0))


def test_solve_the_gauge_weighs_by_overlap():
    sums = [sums_row(300, (2, 2, 2), (1, 1, 1)), sums_row(100, (1, 1, 1), (2, 2, 2))]
    got = engine.mosaic_gain_solve(sums, np.ones((2, 3), np.float32), 16.0)
    s = math.fsum([300 * 2.0, 100 * 0.5]) / math.fsum([300.0, 100.0])
    assert got[0, 0] == np.float32(2.0 / s) and got[1, 0] == np.float32(0.5 / s)
    assert abs((300 * float(got[0, 1]) + 100 * float(got[1, 1])) / 400 - 1) < 1e-7


def test_solve_clamps_at_the_limit_and_its_reciprocal():
    sums = [sums_row(100, (4, 4, 4), (1, 1, 1)), sums_row(100, (1, 1, 1), (4, 4, 4)), sums_row(100, (1, 1, 1), (1, 1, 1))]      # 4, 1/4, 1: mean 1.75
    got = engine.mosaic_gain_solve(sums, np.ones((3, 3), np.float32), 2.0)
    assert got[0].tolist() == [2.0] * 3 and got[1].tolist() == [0.5] * 3 and 0.5 < got[2, 0] < 2.0
    got = engine.mosaic_gain_solve(sums, np.ones((3, 3), np.float32), 3.0)
    assert got[0].tolist() == [float(np.float32(4 / 1.75))] * 3 and got[1].tolist() == [float(np.float32(1.0 / 3.0))] * 3
    one = engine.mosaic_gain_solve(sums, np.ones((3, 3), np.float32), 1.0)
    assert one.tolist() == [[1.0] * 3] * 3                                  # L = 1: every gain is exactly 1
    assert np.array_equal(got, gref.solve(sums, np.ones((3, 3), np.float32), 3.0))


def test_solve_takes_sums_beyond_float64_s_integers():
    big = (1 << 61) + 12345
    sums = [sums_row(1 << 26, (big, big, big), (big - 7, big, big + 7)), sums_row(5, (3, 3, 3), (3, 3, 3))]
    got = engine.mosaic_gain_solve(np.array(sums, np.int64), np.ones((2, 3), np.float32), 2.0)
    assert np.array_equal(got, gref.solve(sums, np.ones((2, 3), np.float32), 2.0)) and bool(np.isfinite(got).all())
    assert engine.mosaic_gain_solve(np.zeros((0, 10), np.int64), np.ones((0, 3), np.float32), 2.0).shape == (0, 3)
    assert engine.mosaic_gain_solve([sums_row(0, (0,) * 3, (0,) * 3)], np.ones((1, 3), np.float32), 2.0).tolist() == [[1.0] * 3]


def test_rms_is_an_integer_sum_under_one_root():
    sums = [sums_row(3, (0,) * 3, (0,) * 3, (16384 ** 2 * 3, 0, 4)), sums_row(1, (0,) * 3, (0,) * 3, (16384 ** 2, 0, 0))]
    assert engine.mosaic_gain_rms(sums) == [1.0, 0.0, math.sqrt(4 / 4) / 16384.0] == gref.rms_of(sums)
    assert engine.mosaic_gain_rms([sums_row(0, (0,) * 3, (0,) * 3)]) == [0.0, 0.0, 0.0]


# ---- the options --------------------------------------------------------------------------------------------------------------------

def test_the_rounds_and_the_limit_are_checked_like_the_other_values():
    assert engine.MOSAIC_GAIN_ROUNDS_RANGE == (1, 64) and engine.MOSAIC_GAIN_LIMIT_RANGE == (1.0, 16.0) and engine.MOSAIC_GAIN_LIMIT == 2.0
    for good in (1, 3, 64, 2.0, np.int64(5)):
        R = engine.mosaic_gain_rounds(good)
        assert type(R) is int and R == int(good)
    for bad in (0, 65, -1, 2.5, True, NAN, float('inf'), None, 'x'):
        with pytest.raises(ValueError, match=r'mosaic gain rounds R must be an integer within \[1, 64\] rounds') as e:
            engine.mosaic_gain_rounds(bad)
        assert e.value.field == 'gains'
    for good in (1, 1.0, 2.5, 16, np.float32(4)):
        L = engine.mosaic_gain_limit(good)
        assert type(L) is float and L == float(good)
    for bad in (0.99, 16.5, 0, -2, NAN, float('inf'), None, 'x'):
        with pytest.raises(ValueError, match=r'mosaic gain limit L must be finite and within \[1, 16\] times') as e:
            engine.mosaic_gain_limit(bad)
        assert e.value.field == 'gain_limit'
    def checked(gains, gain_limit, who):
        o = engine.MosaicOptions(gains=gains, gain_limit=gain_limit).checked(who)
        assert (o.gains is None or type(o.gains) is int) and (o.gain_limit is None or type(o.gain_limit) is float)
        return o.gains, o.gain_limit
    assert checked(None, None, 'x') == (None, None)
    assert checked(3, None, 'x') == (3, 2.0) and checked(3.0, 4, 'x') == (3, 4.0)
    with pytest.raises(ValueError, match=r'who: the limit clamps the gains .* \(gains=R\)') as e:
        checked(None, 2.0, 'who')
    assert e.value.field == 'gain_limit'
    with pytest.raises(ValueError) as e:          # the limit's value before the missing rounds
        checked(None, 17, 'who')
    assert e.value.field == 'gain_limit' and 'within' in str(e.value)
    view = SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')))
    with pytest.raises(ValueError, match='gain rounds R') as e:       # before a Mosaic is made
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, gains=65)
    assert e.value.field == 'gains'
    with pytest.raises(ValueError, match='mosaic_of: the limit clamps') as e:
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, gain_limit=2)
    assert e.value.field == 'gain_limit'


def test_the_pinned_tables_are_extended_and_not_reordered():
    assert [f.name for f in dataclasses.fields(engine.MosaicOptions)][:8] == ['blend', 'feather', 'fill', 'bands', 'surface', 'support', 'gains',
                                                                              'gain_limit']
    assert list(engine.MOSAIC_VALUES)[:8] == ['blend', 'fill', 'feather', 'bands', 'surface', 'support', 'gains', 'gain_limit']
    assert engine.MOSAIC_VALUES['gains'] == ('gain rounds R', (1, 64), True, 'rounds', int, 'R', 'an integer')
    assert engine.MOSAIC_VALUES['gain_limit'] == ('gain limit L', (1.0, 16.0), False, 'times', float, 'L', 'a finite limit')
    assert engine.MOSAIC_VALUES['gains'][1] is engine.MOSAIC_GAIN_ROUNDS_RANGE and engine.MOSAIC_VALUES['gain_limit'][1] is engine.MOSAIC_GAIN_LIMIT_RANGE
    rows = list(engine.MOSAIC_OUTPUTS)
    assert rows[:13] == ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'J_multiband', 'surface',
                         'culled', 'fill_level']
    assert rows[13:22] == ['J_filled', 'raw_filled', 'J_blend_filled', 'raw_blend_filled', 'J_multiband_filled', 'support', 'surface_source',
                           'culled_above', 'surface_top']
    assert not any('gain' in k for k in rows)
    assert sucre._MOSAIC_FLAG['gains'] == '--mosaic-gains' and sucre._MOSAIC_FLAG['gain_limit'] == '--mosaic-gain-limit'
    assert sucre._ONLY_WITH[:5] == [('--mosaic-gsd', '--mosaic', 'DIR'), ('--mosaic-blend', '--mosaic', 'DIR'), ('--mosaic-fill', '--mosaic', 'DIR'),
                                    ('--mosaic-feather', '--mosaic-blend', 'H'), ('--mosaic-bands', '--mosaic-blend', 'H')]
    assert sucre._ONLY_WITH[5:7] == [('--mosaic-gain-limit', '--mosaic-gains', 'R'), ('--mosaic-gains', '--mosaic', 'DIR')]
    assert sucre._ONLY_WITH[7:9] == [('--mosaic-support', '--mosaic-surface', 'T'), ('--mosaic-surface', '--mosaic', 'DIR')]
    assert sucre._ONLY_WITH[9:] == [('--mosaic-gain-solve', '--mosaic-gains', 'R'), ('--mosaic-reject', '--mosaic', 'DIR')]
    assert _lib.MOSAIC_GAIN_WORDS == 10 and _lib.MOSAIC_GAIN_ROW_WORDS * 8 == 128
    for name in ('sucre_mosaic_gain_span', 'sucre_mosaic_gain_apply', 'sucre_mosaic_gain_sums'):
        assert name in _lib.SIGNATURES


BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def answer(extra):
    try:
        sucre.main(BASE + extra)
    except SystemExit as e:
        return e.code
    except FileNotFoundError:
        return 'accepted'
    raise AssertionError(extra)


def test_the_command_line_refuses_before_any_file_is_opened(monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert answer(['--mosaic-gain-limit', '2']) == '--mosaic-gain-limit: only with --mosaic-gains R'
    assert answer(['--mosaic', 'results', '--mosaic-gain-limit', '2']) == '--mosaic-gain-limit: only with --mosaic-gains R'
    assert answer(['--mosaic-gains', '3']) == '--mosaic-gains: only with --mosaic DIR'
    assert answer(['--mosaic-gains', '3', '--mosaic-gain-limit', '2']) == '--mosaic-gains: only with --mosaic DIR'
    for bad, shown in (('0', '0'), ('65', '65'), ('2.5', '2.5'), ('-1', '-1'), ('nan', 'nan'), ('inf', 'inf')):
        assert answer(['--mosaic', 'results', '--mosaic-gains', bad]) == f'--mosaic-gains: R must be an integer within [1, 64] rounds, not {shown}'
    for bad in ('0.99', '0', '16.5', '-2', 'nan', 'inf'):
        assert answer(['--mosaic', 'results', '--mosaic-gains', '3', '--mosaic-gain-limit', bad]) == \
            f'--mosaic-gain-limit: L must be a finite limit within [1, 16] times, not {float(bad)}'
    for good in (['--mosaic-gains', '1'], ['--mosaic-gains', '64'], ['--mosaic-gains', '3.0', '--mosaic-gain-limit', '1'],
                 ['--mosaic-gains', '3', '--mosaic-gain-limit', '16'],
                 ['--mosaic-gains', '3', '--mosaic-surface', '0.05', '--mosaic-support', '2', '--mosaic-blend', '0.5', '--mosaic-bands', '2',
                  '--mosaic-feather', '8', '--mosaic-fill', '0.1']):
        assert answer(['--mosaic', 'results'] + good) == 'accepted', good
    assert answer(['--mosaic', 'results', '--mosaic-gains', '3', '--shared-water']).startswith('--mosaic: --shared-water does not combine')


def test_the_python_entry_refuses_like_the_command_line(monkeypatch):
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda device, what: None)
    image = SimpleNamespace(name='a.png')
    for kw, code in ((dict(gain_limit=2), '--mosaic-gain-limit: only with --mosaic-gains R'),
                     (dict(gains=0), '--mosaic-gains: mosaic gain rounds R must be an integer within [1, 64] rounds, not 0'),
                     (dict(gains=3, gain_limit=0.5), '--mosaic-gain-limit: mosaic gain limit L must be finite and within [1, 16] times, not 0.5')):
        with pytest.raises(SystemExit) as e:
            sucre.mosaic([image], None, 'results', 'out', **kw)
        assert e.value.code == code, kw


# ---- the restatement against plain loops ----------------------------------------------------------------------------------------------

def small_survey():
    """Three small views of one plane from slightly different places, random colours with NaN and an infinity, one view twice."""
    g = torch.Generator().manual_seed(21)
    K = torch.tensor([[20.0, 0.0, 6.0], [0.0, 20.0, 5.0], [0.0, 0.0, 1.0]])
    views, Js = [], []
    for tx, ty in ((0.0, 0.0), (0.21, -0.1), (-0.15, 0.12)):
        depth = torch.full((10, 12), 2.0)
        depth[1, 2] = 0.0
        J = torch.rand((10, 12, 3), generator=g) * 1.5
        J[3, 4, 1] = NAN
        J[5, 5] = torch.tensor([float('inf'), 20.0, -9.0])
        rgb = torch.randint(0, 256, (10, 12, 3), generator=g, dtype=torch.uint8)
        views.append(SimpleNamespace(depth=depth, rgb=rgb, K=K.clone(), R=torch.eye(3), t=torch.tensor([[tx], [ty], [0.0]])))
        Js.append(J)
    far = SimpleNamespace(depth=torch.full((4, 4), 2.0), rgb=torch.zeros((4, 4, 3), dtype=torch.uint8), K=K.clone(), R=torch.eye(3),
                          t=torch.tensor([[5.0], [5.0], [0.0]]))
    return views + [views[1], far], Js + [Js[1], torch.full((4, 4, 3), 0.5)]


def test_the_restatement_equals_plain_loops_over_the_definition():
    views, Js = small_survey()
    axes, gsd = torch.eye(3), 0.2
    got = gref.gains(views, Js, axes, gsd, 2, 2.0)
    n_cells = got['Hm'] * got['Wm']
    assert got['span'].shape == (n_cells, 2) and got['sums'].shape == (3, 5, 10) and got['rms'].shape == (3, 3)
    shared = got['span'][:, 0] < got['span'][:, 1]
    assert shared.any() and (~shared).any()
    for r in (0, 2):
        span, sums = gref.loops(views, Js, axes, gsd, got['tables'][r], got['base'])
        assert np.array_equal(span, got['span']) and np.array_equal(sums, got['sums'][r]), r
    assert got['tables'][0].tolist() == [[1.0] * 3] * 5
    assert got['overlap'][4] == 0 and got['gains'][4].tolist() == [1.0] * 3              # the image that overlaps nothing
    assert bool((got['overlap'][:4] > 0).all())
    # a view listed twice: two ordinals, every cell it reaches is shared
    for p, cell, _ in (got['samples'][1], got['samples'][3]):
        assert bool(shared[cell].all())
    assert np.array_equal(got['samples'][1][1], got['samples'][3][1])
    # the clamp at +-8: the infinity and 20.0 enter as 8 x 16384, -9 as -8 x 16384
    assert gref.quantise(np.array([np.inf, 20.0, -9.0, -np.inf, 8.0, 0.25], np.float32)).tolist() == [131072, 131072, -131072, -131072, 131072, 4096]
    # every table obeys the gauge (before float32 and the clamp: to 1e-6) and the limit
    for G, s in zip(got['tables'][1:], got['sums']):
        assert bool((G >= 0.5).all()) and bool((G <= 2.0).all())
        free = bool(((G > 0.5) & (G < 2.0)).all())
        if free:
            assert np.allclose((s[:, 0:1] * G.astype(np.float64)).sum(axis=0) / s[:, 0].sum(), 1.0, atol=1e-6)
    assert np.array_equal(got['rms'], np.array([engine.mosaic_gain_rms(s) for s in got['sums']]))
    for t, s in zip(got['tables'], got['sums']):       # the engine's solve is the restatement's, to the bit
        assert np.array_equal(engine.mosaic_gain_solve(s, t, 2.0), gref.solve(s, t, 2.0))


def test_limit_one_leaves_every_gain_at_one():
    views, Js = small_survey()
    got = gref.gains(views, Js, torch.eye(3), 0.2, 3, 1.0)
    assert all(t.tolist() == [[1.0] * 3] * 5 for t in got['tables'])
    assert np.array_equal(got['sums'][0], got['sums'][3])
    base = ref.mosaic(views, Js, torch.eye(3), 0.2)
    assert (base['Hm'], base['Wm']) == (got['Hm'], got['Wm'])


def test_the_crafted_survey_on_the_cpu():
    views, Js = crafted.survey()
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * 3)
    assert float(gsd) == float(np.float32(crafted.GSD))
    assert min(float(J.min()) for J in Js) >= 0.25
    got = gref.gains(views, Js, torch.eye(3), gsd, 1, crafted.LIMIT)
    assert bool((got['span'][:, 0] == 0).all()) and bool((got['span'][:, 1] == 2).all())      # fully overlapping: every cell is shared
    assert got['overlap'].tolist() == [crafted.HW[0] * crafted.HW[1]] * 3
    assert crafted.spread(got['tables'][0]) > 0.5
    spread = crafted.spread(got['gains'])
    print(f'crafted: gain x factor spread {crafted.spread(got["tables"][0]):.6g} -> {spread:.6g} (bound {crafted.BOUND:.6g}); '
          f'rms {got["rms"][0].tolist()} -> {got["rms"][1].tolist()}')
    assert spread <= crafted.BOUND
    assert bool((got['rms'][1] < got['rms'][0]).all())
