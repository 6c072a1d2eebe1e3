"""Host tests of the mosaic's view-supported surface: tests/mosaic_support_ref.py against plain Python loops over the definition
(csrc/support.h) on small hand-built cells, the restatement's M = 1 against the surface test's restatement, the crafted fish on
the CPU, the checks of the view count in every entry point and on the command line, the tables older tests pin, the picture of
``culled_above`` and the order in which ``Mosaic.run`` drives the levels.  No GPU."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_ref as ref
import mosaic_support_crafted as crafted
import mosaic_support_ref as pref
import mosaic_surface_ref as sref
from sucre_amd import engine, sucre

NAN = float('nan')
ALL_ONES = 0xffffffffffffffff


# ---- the restatement against loops ----------------------------------------------------------------------------------------------------

def key32(x):
    return int(sref.order_key(np.array([x], np.float32))[0])


def levels_by_loops(samples, n_cells, M):
    """The definition, level by level: ``samples`` is a list of (cell, a_n, ordinal); returns n_cells lists of M key64 integers."""
    out = []
    for cell in range(n_cells):
        mine = [(key32(a) << 32) | o for c, a, o in samples if c == cell and a == a]       # a NaN adds nothing
        taken, words = set(), []
        for _ in range(M):
            left = [w for w in mine if (w & 0xffffffff) not in taken]
            if not left:
                words.append(ALL_ONES)       # and so do all levels above it: `taken` no longer grows
                continue
            words.append(min(left))
            taken.add(words[-1] & 0xffffffff)
        out.append(words)
    return out


def hand_built_cells():
    """Five cells: 0 seen by three images, several samples each; 1 an exact height tie between ordinals 2 and 5 (and -0.0 against
    +0.0 between 1 and 3, which is no tie); 2 one view listed twice (ordinals 0 and 4 hold the same samples) and a third; 3 empty;
    4 one image alone, with a NaN height next to a real one, and an image whose only sample there is a NaN."""
    f = np.float32
    s = []
    s += [(0, f(2.00), 0), (0, f(1.98), 0), (0, f(1.50), 1), (0, f(1.52), 1), (0, f(1.51), 1), (0, f(2.01), 2), (0, f(1.99), 2)]
    s += [(1, f(2.25), 5), (1, f(2.25), 2), (1, f(2.5), 2), (1, f(0.0), 3), (1, f(-0.0), 1), (1, f(3.0), 3)]
    s += [(2, f(-1.0), 0), (2, f(-0.75), 0), (2, f(-1.0), 4), (2, f(-0.75), 4), (2, f(-0.9), 2)]
    s += [(4, f(NAN), 6), (4, f(7.0), 6), (4, f(NAN), 3)]
    return s, 5


@pytest.mark.parametrize('M', [1, 2, 3, 4])
def test_the_levels_equal_the_definition_on_hand_built_cells(M):
    samples, n_cells = hand_built_cells()
    rng = np.random.default_rng(M)
    order = rng.permutation(len(samples))      # the order of arrival means nothing
    cell, a_n, ordinal = (np.array([samples[i][j] for i in order]) for j in range(3))
    rank = pref.ranks(cell, a_n.astype(np.float32), ordinal, n_cells, M)
    assert rank.dtype == np.uint64 and rank.shape == (M, n_cells)
    want = levels_by_loops(samples, n_cells, M)
    assert [[int(rank[r, c]) for r in range(M)] for c in range(n_cells)] == want
    top, n, source = pref.supported_top(rank)
    seen = [3, 4, 3, 0, 1]                      # images that reach each cell
    assert n.tolist() == [min(M, k) for k in seen]
    for c in range(n_cells):
        held = [w for w in want[c] if w != ALL_ONES]
        assert int(top[c]) == (held[-1] >> 32 if held else 0xffffffff)
        assert int(source[c]) == (held[-1] & 0xffffffff if held else -1)
    # what the cases are there for
    first = [w & 0xffffffff for w in want[1]]
    assert first[:min(M, 4)] == [1, 3, 2, 5][:M]                        # -0.0 below +0.0; the tie at 2.25 goes to ordinal 2
    assert [w & 0xffffffff for w in want[2]][:min(M, 3)] == [0, 4, 2][:M]  # a view listed twice holds two levels
    assert want[3] == [ALL_ONES] * M and want[4][1:] == [ALL_ONES] * (M - 1) and want[4][0] == (key32(7.0) << 32) | 6
    heights = pref.heights_of(top)
    assert np.isnan(heights[3]) and heights[4] == 7.0
    assert heights[0] == np.float32([1.50, 1.98, 1.99, 1.99][M - 1])    # fewer than M images: the lowest of the per-image tops
    assert heights[2] == np.float32([-1.0, -1.0, -0.9, -0.9][M - 1])       # at M = 2 the twice-listed view supports itself


@pytest.mark.parametrize('M', [1, 2, 3, 4])
def test_the_two_sided_cull_equals_the_definition_on_hand_built_cells(M):
    samples, n_cells = hand_built_cells()
    cell, a_n, ordinal = (np.array([s[j] for s in samples]) for j in range(3))
    a_n = a_n.astype(np.float32)
    top, _, _ = pref.supported_top(pref.ranks(cell, a_n, ordinal, n_cells, M))
    for T in (0.015, 0.3, 1e6):
        below, above = pref.cull_sides(cell, a_n, top, T)
        for i, (c, a, o) in enumerate(samples):
            d = np.float32(a) - pref.heights_of(top)[c]
            assert bool(below[i]) == bool(d > np.float32(T)) and bool(above[i]) == bool(d < -np.float32(T)), (M, T, i)
        if M == 1:
            assert not above.any()                                       # nothing stands above a minimum
        if T == 1e6:
            assert not below.any() and not above.any()
        # the sample that defines the top is never culled
        for c in range(n_cells):
            mine = [i for i, s in enumerate(samples) if s[0] == c and key32(s[1]) == int(top[c]) and s[1] == s[1]]
            assert all(not below[i] and not above[i] for i in mine) and (mine or top[c] == 0xffffffff)
    below, above = pref.cull_sides(cell, a_n, top, 0.015)
    if M == 2:
        assert above[[2, 3, 4]].all() and not above[[0, 1, 5, 6]].any()       # cell 0: image 1 stands 0.46 above what two images reach


def tiny_triple():
    """test_mosaic_surface_host.py's pair and a third image, the first view once more (a view listed twice)."""
    g = torch.Generator().manual_seed(3)
    K = torch.tensor([[8.0, 0.0, 3.5], [0.0, 8.0, 2.5], [0.0, 0.0, 1.0]])
    views, Js = [], []
    for tz, rough in ((0.0, 0.02), (-0.3, 0.3)):
        depth = 2.0 - tz + rough * (2 * torch.rand((5, 7), generator=g) - 1)
        views.append(SimpleNamespace(depth=depth, rgb=torch.zeros((5, 7, 3), dtype=torch.uint8), K=K, R=torch.eye(3),
                                     t=torch.tensor([[0.01], [-0.02], [tz]])))
        Js.append(torch.rand((5, 7, 3), generator=g))
    views[0].depth[1, 2] = 0.0
    Js[1][3, 4, 1] = NAN
    return views + [views[0]], Js + [Js[0]]


@pytest.mark.parametrize('T', [0.05, 0.25, 1e6])
def test_one_supporting_view_is_the_surface_test(T):
    views, Js = tiny_triple()
    axes, gsd = torch.eye(3), 0.3
    was = sref.surface(views, Js, axes, gsd, T)
    got = pref.support(views, Js, axes, gsd, T, 1)
    assert got['top'].tobytes() == was['top'].tobytes() and got['bounds'] == was['bounds'] and (got['Hm'], got['Wm']) == (was['Hm'], was['Wm'])
    assert got['counts'] == (was['counts'][0], 0, was['counts'][1]) and not bool(got['culled_above'].any())
    assert got['surface'].numpy().tobytes() == was['surface'].numpy().tobytes() == got['surface_top'].numpy().tobytes()
    assert torch.equal(got['culled'], was['culled'])
    for a, b in zip(got['Js'], was['Js']):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    filled = ~torch.isnan(got['surface'])
    assert torch.equal(got['support'] == 1, filled) and torch.equal(got['surface_source'] >= 0, filled)


def test_the_images_against_loops_with_a_view_listed_twice():
    views, Js = tiny_triple()
    axes, gsd, T = torch.eye(3), 0.3, 0.05
    for M in (2, 3, 4):
        got = pref.support(views, Js, axes, gsd, T, M)
        samples = []      # the heights from the surface test's restatement; the cells from `support` (its chain is the surface test's)
        for i, (view, J) in enumerate(zip(views, Js)):
            p, _, _, a_n = sref.heights(view, J, axes)
            px, cell = got['cells'][i]
            assert np.array_equal(px, p)                                 # every member has a cell here
            samples += [(int(c), a, i) for c, a in zip(cell, a_n)]
        want = levels_by_loops(samples, got['Hm'] * got['Wm'], M)
        assert [[int(got['rank'][r, c]) for r in range(M)] for c in range(got['Hm'] * got['Wm'])] == want
        # ordinals 0 and 2 are one view: wherever it reaches a cell, both hold a level with one height
        r = got['rank']
        both = (r[0] != pref.NO_RANK) & (r[1] != pref.NO_RANK) & ((r[0] & np.uint64(0xffffffff)) == 0) & ((r[1] & np.uint64(0xffffffff)) == 2)
        assert both.any() and bool(((r[0] >> np.uint64(32)) == (r[1] >> np.uint64(32)))[both].all())
        n_below = sum(1 for c, a, _ in samples if np.float32(a - pref.heights_of(got['top'])[c]) > np.float32(T))
        n_above = sum(1 for c, a, _ in samples if np.float32(a - pref.heights_of(got['top'])[c]) < -np.float32(T))
        assert got['counts'] == (n_below, n_above, len(samples)) and int(got['culled'].sum()) == n_below
        assert int(got['culled_above'].sum()) == n_above


# ---- the fish on the CPU --------------------------------------------------------------------------------------------------------------
FISH_CELLS_WHOLLY, FISH_CELLS_REACHED = 63, 63       # cells whose every sample of the fish's view is the fish; cells the fish reaches


def fish_cells(got):
    """(cells the fish reaches, those of them in which the fish's view has no other sample), from the restatement alone."""
    px, cell = got['cells'][crafted.FISH_VIEW]
    is_fish = np.isin(px, crafted.fish_pixels())
    reached = set(cell[is_fish].tolist())
    return reached, reached - set(cell[~is_fish].tolist())


def test_the_fish_on_the_cpu():
    views, Js = crafted.survey()
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * 3)
    assert float(gsd) == float(np.float32(crafted.GSD))
    axes, T, fish = torch.eye(3), crafted.TOL, crafted.FISH_VIEW
    plain = sref.expected(views, Js, axes, gsd, T)
    got = pref.expected(views, Js, axes, gsd, T, 2)
    reached, wholly = fish_cells(got)
    assert (len(wholly), len(reached)) == (FISH_CELLS_WHOLLY, FISH_CELLS_REACHED)      # some tens of cells, completely
    patch = torch.zeros(got['Hm'] * got['Wm'], dtype=torch.bool)
    patch[sorted(reached)] = True
    patch = patch.view(got['Hm'], got['Wm'])
    # the plain minimum: the fish owns every cell it reaches, and the plane's samples there are culled
    assert bool((plain['source'][patch] == fish).all()) and bool((plain['surface'][patch] == crafted.FISH).all())
    assert bool((plain['culled'][patch] > 0).all()) and not bool(plain['culled'][~patch].any())
    assert bool(np.isin(plain['pixel'][patch].numpy(), crafted.fish_pixels()).all())
    # two supporting views: the fish is gone
    won_by_fish_view = got['source'] == fish
    assert not bool(np.isin(got['pixel'][won_by_fish_view].numpy(), crafted.fish_pixels()).any())
    assert bool(((got['surface'][patch] - crafted.PLANE).abs() <= T).all())
    assert torch.equal(got['culled_above'] > 0, patch) and not bool(got['culled'].any())
    assert got['counts'][1] == len(crafted.fish_pixels())
    for k in ('J', 'source', 'surface'):
        a, b = got[k][~patch], plain[k][~patch]
        assert a.numpy().tobytes() == b.numpy().tobytes(), k
    assert torch.equal(got['source'] >= 0, plain['source'] >= 0)          # the filled set does not change
    assert bool((got['surface_top'][patch] == crafted.FISH).all())        # where support changed the surface


# ---- the view count and the tables ----------------------------------------------------------------------------------------------------

def test_the_view_count_is_checked_like_the_other_values():
    assert engine.MOSAIC_SUPPORT_RANGE == (1, 4)
    for good in (1, 2, 4, 3.0, np.int64(2)):
        M = engine.mosaic_support_views(good)
        assert type(M) is int and M == int(good)
    for bad in (0, 5, -1, 2.5, True, NAN, float('inf'), None, 'x'):
        with pytest.raises(ValueError, match=r'mosaic supporting views M must be an integer within \[1, 4\] views') as e:
            engine.mosaic_support_views(bad)
        assert e.value.field == 'support'
    view = SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')))
    with pytest.raises(ValueError, match='supporting views M') as e:       # before a Mosaic is made
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, surface=0.05, support=5)
    assert e.value.field == 'support'
    with pytest.raises(ValueError, match=r'mosaic_of: the support decides which top .* \(surface=T\)') as e:
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, support=2)
    assert e.value.field == 'support'
    assert engine.MosaicOptions().checked('x').support is None
    both = engine.MosaicOptions(support=2.0, surface=np.float32(0.1)).checked('x')
    assert both.support == 2 and type(both.support) is int
    with pytest.raises(ValueError, match=r'who: the support decides which top .* \(surface=T\)') as e:
        engine.MosaicOptions(support=2).checked('who')
    assert e.value.field == 'support'


def test_the_pinned_tables_are_extended_and_not_reordered():
    assert [f.name for f in dataclasses.fields(engine.MosaicOptions)][:6] == ['blend', 'feather', 'fill', 'bands', 'surface', 'support']
    assert list(engine.MOSAIC_VALUES)[:6] == ['blend', 'fill', 'feather', 'bands', 'surface', 'support']
    assert engine.MOSAIC_VALUES['support'] == ('supporting views M', (1, 4), True, 'views', int, 'M', 'an integer')
    assert engine.MOSAIC_VALUES['support'][1] is engine.MOSAIC_SUPPORT_RANGE
    rows = list(engine.MOSAIC_OUTPUTS)
    assert rows[:13] == ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'J_multiband', 'surface',
                         'culled', 'fill_level']
    assert rows[13:18] == ['J_filled', 'raw_filled', 'J_blend_filled', 'raw_blend_filled', 'J_multiband_filled']
    assert rows[18:22] == ['support', 'surface_source', 'culled_above', 'surface_top']
    nan = engine.MOSAIC_OUTPUTS['range'][3]
    assert engine.MOSAIC_OUTPUTS['support'] == ('support', (), torch.int32, 0, None, None)
    assert engine.MOSAIC_OUTPUTS['surface_source'] == ('support', (), torch.int32, -1, None, None)
    assert engine.MOSAIC_OUTPUTS['culled_above'] == ('support', (), torch.int32, 0, 'mosaic_culled_above.png', 'count')
    assert engine.MOSAIC_OUTPUTS['surface_top'] == ('support', (), torch.float32, nan, None, None) and nan != nan
    assert sucre._MOSAIC_FLAG['support'] == '--mosaic-support'
    assert sucre._ONLY_WITH[7:9] == [('--mosaic-support', '--mosaic-surface', 'T'), ('--mosaic-surface', '--mosaic', 'DIR')]
    assert sucre._ONLY_WITH[:5] == [('--mosaic-gsd', '--mosaic', 'DIR'), ('--mosaic-blend', '--mosaic', 'DIR'), ('--mosaic-fill', '--mosaic', 'DIR'),
                                    ('--mosaic-feather', '--mosaic-blend', 'H'), ('--mosaic-bands', '--mosaic-blend', 'H')]


def test_the_picture_of_culled_above_follows_the_count_rule():
    group, tail, dtype, empty, png, how = engine.MOSAIC_OUTPUTS['culled_above']
    assert (png, how) == ('mosaic_culled_above.png', engine.MOSAIC_OUTPUTS['culled'][5])
    c = torch.tensor([[0, 3, 1], [2, 0, 3]], dtype=torch.int32)
    got = sucre._MOSAIC_PNG[how](c, None)
    assert got.dtype == np.uint8 and got.tolist() == [[0, 255, 85], [170, 0, 255]]
    assert np.array_equal(got, sucre.mosaic_culled_picture(c.numpy()))
    assert sucre._MOSAIC_PNG[how](torch.zeros((2, 2), dtype=torch.int32), None).tolist() == [[0, 0], [0, 0]]


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
    assert answer(['--mosaic-support', '2']) == '--mosaic-support: only with --mosaic-surface T'
    assert answer(['--mosaic', 'results', '--mosaic-support', '2']) == '--mosaic-support: only with --mosaic-surface T'
    assert answer(['--mosaic', 'results', '--mosaic-blend', '0.5', '--mosaic-support', '2']) == '--mosaic-support: only with --mosaic-surface T'
    assert answer(['--mosaic-surface', '0.05', '--mosaic-support', '2']) == '--mosaic-surface: only with --mosaic DIR'
    for bad, shown in (('0', '0'), ('5', '5'), ('-1', '-1'), ('2.5', '2.5'), ('nan', 'nan'), ('inf', 'inf')):
        assert answer(['--mosaic', 'results', '--mosaic-surface', '0.05', '--mosaic-support', bad]) == \
            f'--mosaic-support: M must be an integer within [1, 4] views, not {shown}'
    for good in ('1', '2', '4', '3.0'):
        assert answer(['--mosaic', 'results', '--mosaic-surface', '0.05', '--mosaic-support', good]) == 'accepted'
    assert answer(['--mosaic', 'results', '--mosaic-surface', '0.05', '--mosaic-support', '2', '--mosaic-blend', '0.5', '--mosaic-bands', '2',
                   '--mosaic-fill', '0.1']) == 'accepted'
    assert answer(['--mosaic', 'results', '--mosaic-surface', '0', '--mosaic-support', '2']).startswith('--mosaic-surface: T must be')
    assert answer(['--mosaic', 'results', '--mosaic-surface', '0.05', '--mosaic-support', '2', '--shared-water']).startswith(
        '--mosaic: --shared-water does not combine')


# ---- the order of the phases ----------------------------------------------------------------------------------------------------------

class Recorder(engine.Mosaic):
    log, begun = [], []

    def __init__(self, axes, gsd, device):
        self._held = {}

    def add_bounds(self, views, Js):
        self.log.append(('add_bounds', None, len(views)))

    def begin(self, bounds=None, blend=None, feather=None, bands=None, surface=None, support=None):
        self.log.append(('begin', None, None))
        self.begun.append((blend, feather, bands, surface, support))

    def add_surface(self, views, Js, first_ordinal, plain_atomic=False):
        self.log.append(('add_surface', first_ordinal, len(views)))

    def add_support(self, views, Js, first_ordinal, level, plain_atomic=False):
        self.log.append(('add_support', first_ordinal, len(views), level, plain_atomic))

    def finish_support(self):
        self.log.append(('finish_support', None, None))

    def culled_images(self, views, Js, first_ordinal, count=False):
        self.log.append(('culled_images', first_ordinal, count))
        return ['culled'] * len(views)


for _name in ('splat', 'resolve', 'gather'):
    def _phase(self, views, Js, first_ordinal, _name=_name, **kw):
        self.log.append((_name, first_ordinal, len(views), self._held.get('cull')))
    setattr(Recorder, _name, _phase)


@pytest.fixture
def recorder(monkeypatch):
    monkeypatch.setattr(Recorder, 'log', [])
    monkeypatch.setattr(Recorder, 'begun', [])
    monkeypatch.setattr(engine, 'Mosaic', Recorder)
    return Recorder


VIEWS = [SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')), name=f'v{i}') for i in range(3)]


def test_run_takes_every_level_over_every_batch_before_the_next(recorder):
    m = engine.mosaic_of(VIEWS, [object()] * 3, torch.eye(3), 0.25, batch=2, surface=0.05, support=3.0, plain_atomic=True)
    assert recorder.begun == [(None, None, None, np.float32(0.05), 3)] and type(recorder.begun[0][4]) is int
    levels = [('add_support', first, n, level, True) for level in range(3) for first, n in ((0, 2), (2, 1))]
    phase = lambda name: [(name, 0, 2, None), (name, 2, 1, None)]
    assert recorder.log == [('add_bounds', None, 2), ('add_bounds', None, 1), ('begin', None, None)] + levels \
        + [('finish_support', None, None)] + phase('splat') + phase('resolve') + phase('gather')
    assert m._held == {}


def test_a_single_batch_is_culled_once_after_the_top_is_formed(recorder):
    held = ['culled'] * 3
    engine.mosaic_of(VIEWS, [object()] * 3, torch.eye(3), 0.25, surface=0.05, support=1)
    assert recorder.log == [('add_bounds', None, 3), ('begin', None, None), ('add_support', 0, 3, 0, False), ('finish_support', None, None),
                            ('culled_images', 0, True), ('splat', 0, 3, held), ('resolve', 0, 3, held), ('gather', 0, 3, held)]


def test_without_the_flag_the_surface_test_runs_as_before(recorder):
    engine.mosaic_of(VIEWS, [object()] * 3, torch.eye(3), 0.25, batch=2, surface=0.05)
    assert recorder.begun == [(None, None, None, np.float32(0.05), None)]
    assert [r[0] for r in recorder.log] == ['add_bounds'] * 2 + ['begin'] + ['add_surface'] * 2 + ['splat'] * 2 + ['resolve'] * 2 + ['gather'] * 2
