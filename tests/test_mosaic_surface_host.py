"""Host tests of the mosaic's surface test: tests/mosaic_surface_ref.py against plain Python loops over the definition
(csrc/surface.h) on a tiny case, the checks of the tolerance in every entry point and on the command line, the tables an older
test pins, the two picture functions and the order in which ``Mosaic.run`` drives the phases.  No GPU."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_ref as ref
import mosaic_surface_ref as sref
from sucre_amd import engine, sucre

NAN = float('nan')


# ---- the restatement against loops ----------------------------------------------------------------------------------------------------

def tiny_pair():
    """Two 5 x 7 images over one another, the second from 0.3 m further back and with a rough depth map; a depth hole, a NaN and a
    -0.0 / inf colour among them."""
    g = torch.Generator().manual_seed(3)
    K = torch.tensor([[8.0, 0.0, 3.5], [0.0, 8.0, 2.5], [0.0, 0.0, 1.0]])
    views, Js = [], []
    for tz, rough in ((0.0, 0.02), (-0.3, 0.3)):
        depth = 2.0 - tz + rough * (2 * torch.rand((5, 7), generator=g) - 1)
        J = torch.rand((5, 7, 3), generator=g)
        views.append(SimpleNamespace(depth=depth, rgb=torch.zeros((5, 7, 3), dtype=torch.uint8), K=K, R=torch.eye(3),
                                     t=torch.tensor([[0.01], [-0.02], [tz]])))
        Js.append(J)
    views[0].depth[1, 2] = 0.0
    Js[1][3, 4, 1] = NAN
    Js[0][0, 0] = torch.tensor([-0.0, float('inf'), -2000.0])
    return views, Js


def by_loops(views, Js, axes, gsd, T, bounds):
    """The definition, pixel by pixel: (top per cell, culled count per cell, counts, culled pixels per image)."""
    f = np.float32
    fma = lambda a, b, c: f(ref.fma32(f(a), f(b), f(c)))
    dot = lambda r, x, y, z: fma(r[2], z, fma(r[1], y, f(r[0]) * f(x)))
    lo_s, lo_t, hi_s, hi_t = (f(x) for x in bounds)
    g, T = f(gsd), f(T)
    Wm, Hm = int((hi_s - lo_s) / g) + 1, int((hi_t - lo_t) / g) + 1
    A = np.asarray(axes, np.float32).reshape(3, 3)
    samples = []
    for i, (view, J) in enumerate(zip(views, Js)):
        depth, Jn = view.depth.numpy(), J.numpy()
        Kinv, R, t = view.K.inverse().numpy(), view.R.numpy(), view.t.numpy().reshape(3)
        for v in range(depth.shape[0]):
            for u in range(depth.shape[1]):
                d = depth[v, u]
                if not d > 0 or any(x != x for x in Jn[v, u]):
                    continue
                x, y, w = d * (f(u) + f(0.5)), d * (f(v) + f(0.5)), d * f(1.0)
                cP = [dot(Kinv[r], x, y, w) for r in range(3)]
                wP = [dot(R[r], *cP) + t[r] for r in range(3)]
                a_s, a_t, a_n = (dot(A[r], *wP) for r in range(3))
                qs, qt = (a_s - lo_s) / g, (a_t - lo_t) / g
                if 0 <= qs < Wm and 0 <= qt < Hm:
                    samples.append((i, v, u, int(qt) * Wm + int(qs), a_n))
    top = {}
    for _, _, _, cell, a_n in samples:
        top[cell] = min(top.get(cell, a_n), a_n)
    count, gone = {}, [set() for _ in views]
    for i, v, u, cell, a_n in samples:
        if f(a_n - top[cell]) > T:
            count[cell] = count.get(cell, 0) + 1
            gone[i].add((v, u))
    return top, count, (sum(count.values()), len(samples)), gone, (Hm, Wm)


@pytest.mark.parametrize('T', [0.05, 0.25, 1e6])
def test_the_restatement_equals_plain_loops_on_a_tiny_case(T):
    views, Js = tiny_pair()
    axes, gsd = torch.eye(3), 0.3
    bounds = ref.bounds_of(views, Js, axes)
    got = sref.surface(views, Js, axes, gsd, T)
    top, count, counts, gone, (Hm, Wm) = by_loops(views, Js, axes.numpy(), gsd, T, bounds)
    assert (got['Hm'], got['Wm']) == (Hm, Wm) and got['bounds'] == bounds and got['counts'] == counts
    want_top = np.full(Hm * Wm, NAN, np.float32)
    want_count = np.zeros(Hm * Wm, np.int32)
    for cell, a_n in top.items():
        want_top[cell] = a_n
    for cell, n in count.items():
        want_count[cell] = n
    assert got['surface'].numpy().tobytes() == want_top.reshape(Hm, Wm).tobytes()
    assert np.array_equal(got['culled'].numpy(), want_count.reshape(Hm, Wm))
    if T == 0.05:
        assert 0 < counts[0] < counts[1] and len(top) > 1       # something is culled, something stays
    if T == 1e6:
        assert counts[0] == 0
    for view, J, Jc, mask, away in zip(views, Js, got['Js'], got['mask'], gone):
        assert {(int(v), int(u)) for v, u in zip(*np.nonzero(mask))} == away
        for v in range(5):
            for u in range(7):
                member = bool(view.depth[v, u] > 0) and not bool(torch.isnan(J[v, u]).any())
                if member and (v, u) not in away:
                    assert Jc[v, u].numpy().tobytes() == J[v, u].numpy().tobytes()      # -0.0 and inf included
                else:
                    assert Jc[v, u].numpy().view(np.uint32).tolist() == [0x7fc00000] * 3


def test_the_keys_order_like_the_values():
    x = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    k = sref.order_key(x)
    assert k.dtype == np.uint32 and bool((k[1:] > k[:-1]).all())
    assert sref.key_value(k).tobytes() == x.tobytes()


def test_the_two_layers_on_the_cpu():
    """What the issue measured: range alone lets the lower layer win 588 of the 999 cells; a test at 0.1 m gives every cell to the
    upper one and culls every sample of the lower, one at 0.6 m culls nothing."""
    views, Js = sref.two_layers()
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0, 100.0])
    assert float(gsd) == float(np.float32(sref.LAYERS_GSD))
    plain = ref.mosaic(views, Js, torch.eye(3), gsd)
    assert (plain['Hm'], plain['Wm']) == sref.LAYERS_CELLS and int((plain['source'] >= 0).sum()) == 999
    assert int((plain['source'] == 1).sum()) == 588
    tested = sref.expected(views, Js, torch.eye(3), gsd, 0.1)
    assert bool((tested['source'] == 0).all()) and bool((tested['surface'] == 2.0).all())
    assert int(tested['culled'].sum()) == 3072 and tested['counts'] == (3072, 6144)
    loose = sref.expected(views, Js, torch.eye(3), gsd, 0.6)
    assert loose['counts'] == (0, 6144)
    for k in ('J', 'raw', 'source', 'pixel', 'range'):
        assert torch.equal(loose[k].view(torch.uint8), plain[k].view(torch.uint8)), k


# ---- the tolerance and the tables -----------------------------------------------------------------------------------------------------

def test_the_tolerance_is_checked_like_the_other_values():
    assert engine.MOSAIC_SURFACE_RANGE == (1e-6, 1e6)
    for good in (1e-6, 0.05, 1, 1e6, np.float32(1e-6)):
        T = engine.mosaic_surface_tol(good)
        assert type(T) is np.float32 and T == np.float32(good)
    for bad in (0, -1.0, 9e-7, 1.1e6, NAN, float('inf'), None, 'x'):
        with pytest.raises(ValueError, match=r'mosaic surface tolerance T must be finite and within \[1e-06, 1e\+06\] metres') as e:
            engine.mosaic_surface_tol(bad)
        assert e.value.field == 'surface'
    view = SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')))
    with pytest.raises(ValueError, match='surface tolerance T'):       # before a Mosaic is made
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, surface=0)


def test_the_pinned_tables_are_what_they_were():
    assert [f.name for f in dataclasses.fields(engine.MosaicOptions)][:5] == ['blend', 'feather', 'fill', 'bands', 'surface']
    assert list(engine.MOSAIC_VALUES)[:5] == ['blend', 'fill', 'feather', 'bands', 'surface']
    assert engine.MOSAIC_VALUES['surface'] == ('surface tolerance T', (1e-6, 1e6), False, 'metres', np.float32, 'T', 'a finite tolerance')
    assert engine.MOSAIC_VALUES['surface'][1] is engine.MOSAIC_SURFACE_RANGE
    rows = list(engine.MOSAIC_OUTPUTS)
    assert rows[:10] == ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'J_multiband']
    assert rows[10:12] == ['surface', 'culled'] and rows[12] == 'fill_level'
    assert engine.MOSAIC_OUTPUTS['surface'] == ('surface', (), torch.float32, engine.MOSAIC_OUTPUTS['range'][3], 'mosaic_surface.png', 'height')
    assert engine.MOSAIC_OUTPUTS['surface'][3] != engine.MOSAIC_OUTPUTS['surface'][3]      # NaN
    assert engine.MOSAIC_OUTPUTS['culled'] == ('surface', (), torch.int32, 0, 'mosaic_culled.png', 'count')
    assert set(sucre._MOSAIC_PNG) >= {how for *_, how in engine.MOSAIC_OUTPUTS.values() if how}
    assert sucre._MOSAIC_FLAG['surface'] == '--mosaic-surface' and sucre._ONLY_WITH[8] == ('--mosaic-surface', '--mosaic', 'DIR')


BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def answer(extra):
    try:
        sucre.main(BASE + extra)
    except SystemExit as e:
        return e.code
    except FileNotFoundError as e:
        return 'accepted'
    raise AssertionError(extra)


def test_the_command_line_refuses_before_any_file_is_opened(monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert answer(['--mosaic-surface', '0.05']) == '--mosaic-surface: only with --mosaic DIR'
    assert answer(['--mosaic-surface', '0.05', '--mosaic-blend', '0.5']) == '--mosaic-blend: only with --mosaic DIR'
    for bad, shown in (('0', '0.0'), ('-1', '-1.0'), ('nan', 'nan'), ('inf', 'inf'), ('1e7', '10000000.0'), ('9e-7', '9e-07')):
        assert answer(['--mosaic', 'results', '--mosaic-surface', bad]) == \
            f'--mosaic-surface: T must be a finite tolerance within [1e-06, 1e+06] metres, not {shown}'
    assert answer(['--mosaic', 'results', '--mosaic-surface', '0.05']) == 'accepted'
    assert answer(['--mosaic', 'results', '--mosaic-surface', '1e6', '--mosaic-blend', '0.5', '--mosaic-bands', '2']) == 'accepted'
    assert answer(['--mosaic', 'results', '--mosaic-surface', '0.05', '--shared-water']).startswith('--mosaic: --shared-water does not combine')


# ---- the pictures ---------------------------------------------------------------------------------------------------------------------

def test_the_surface_picture():
    s = np.array([[NAN, 1.0, 3.0], [2.0, 1.5, NAN]], np.float32)
    got = sucre.mosaic_surface_picture(s)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert got.tolist() == [[0, 255, 1], [128, 1 + int(np.rint(254 * 1.5 / 2.0)), 0]]      # the highest ground (smallest value) white
    assert sucre.mosaic_surface_picture(np.array([[2.0, NAN, 2.0]], np.float32)).tolist() == [[255, 0, 255]]      # flat
    assert sucre.mosaic_surface_picture(np.full((2, 2), NAN, np.float32)).tolist() == [[0, 0], [0, 0]]
    g = np.random.default_rng(1).uniform(-3, 5, (9, 11)).astype(np.float32)
    pic = sucre.mosaic_surface_picture(g).astype(int)
    assert pic.min() == 1 and pic.max() == 255 and pic.reshape(-1)[g.argmin()] == 255 and pic.reshape(-1)[g.argmax()] == 1
    lo, hi = float(g.min()), float(g.max())
    assert np.array_equal(pic, 1 + np.rint(254.0 * (hi - g.astype(np.float64)) / (hi - lo)).astype(int))


def test_the_culled_picture():
    c = np.array([[0, 3, 1], [2, 0, 3]], np.int32)
    got = sucre.mosaic_culled_picture(c)
    assert got.dtype == np.uint8 and got.tolist() == [[0, 255, 85], [170, 0, 255]]
    assert sucre.mosaic_culled_picture(np.zeros((2, 3), np.int32)).tolist() == [[0, 0, 0], [0, 0, 0]]
    big = np.array([[2 ** 30, 1]], np.int32)       # 255 x 2^30 passes int32: the product is formed in int64
    assert sucre.mosaic_culled_picture(big).tolist() == [[255, 0]]


# ---- the order of the phases ----------------------------------------------------------------------------------------------------------

class Recorder(engine.Mosaic):
    log, begun = [], []

    def __init__(self, axes, gsd, device):
        self._held = {}

    def add_bounds(self, views, Js):
        self.log.append(('add_bounds', None, len(views)))

    def begin(self, bounds=None, blend=None, feather=None, bands=None, surface=None):
        self.log.append(('begin', None, None))
        self.begun.append((blend, feather, bands, surface))

    def add_surface(self, views, Js, first_ordinal, plain_atomic=False):
        self.log.append(('add_surface', first_ordinal, len(views)))

    def culled_images(self, views, Js, first_ordinal, count=False):
        self.log.append(('culled_images', first_ordinal, count))
        return ['culled'] * len(views)

    def normalize(self, check=True):
        self.log.append(('normalize', None, None))


for _name in ('splat', 'resolve', 'gather', 'accumulate'):
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


def test_run_takes_the_surface_over_every_batch_before_the_splat(recorder):
    m = engine.mosaic_of(VIEWS, [object()] * 3, torch.eye(3), 0.25, batch=2, blend=0.5, surface=0.05)
    assert recorder.begun == [(np.float32(0.5), None, None, np.float32(0.05))] and type(recorder.begun[0][3]) is np.float32
    phase = lambda name: [(name, 0, 2, None), (name, 2, 1, None)]
    assert recorder.log == [('add_bounds', None, 2), ('add_bounds', None, 1), ('begin', None, None), ('add_surface', 0, 2),
                            ('add_surface', 2, 1)] + phase('splat') + phase('resolve') + phase('gather') + phase('accumulate') \
        + [('normalize', None, None)]
    assert m._held == {}


def test_a_single_batch_is_culled_once_and_counted_then(recorder):
    held = ['culled'] * 3
    m = engine.mosaic_of(VIEWS, [object()] * 3, torch.eye(3), 0.25, surface=0.05)
    assert recorder.log == [('add_bounds', None, 3), ('begin', None, None), ('add_surface', 0, 3), ('culled_images', 0, True),
                            ('splat', 0, 3, held), ('resolve', 0, 3, held), ('gather', 0, 3, held)]
    assert m._held == {}       # nothing of one run is left for the next


def test_without_the_flag_begin_is_not_given_it(recorder):
    engine.mosaic_of(VIEWS, [object()] * 3, torch.eye(3), 0.25, batch=2)
    assert recorder.begun == [(None, None, None, None)]
    assert [r[0] for r in recorder.log] == ['add_bounds'] * 2 + ['begin'] + ['splat'] * 2 + ['resolve'] * 2 + ['gather'] * 2
