"""Host tests of the order in which ``engine.mosaic_of`` drives the phases of ``engine.Mosaic``: a subclass that only records its
calls stands in for the class, and every recorded sequence is written out here.  No GPU, and nothing of the library is called."""
from types import SimpleNamespace

import pytest
import torch

from sucre_amd import engine


class Recorder(engine.Mosaic):
    """Records ``(name, ordinal of the batch's first image or None, number of images or None)``; ``plain`` collects the phases that
    were asked for their plain-atomic form, ``begun`` what ``begin`` was given."""
    log, plain, begun, filled = [], [], [], []

    def __init__(self, axes, gsd, device):
        self.log.append(('Mosaic', None, None))

    def add_bounds(self, views, Js):
        assert len(views) == len(Js)
        self.log.append(('add_bounds', None, len(views)))

    def begin(self, bounds=None, blend=None, feather=None):
        self.log.append(('begin', None, None))
        self.begun.append((bounds, blend, feather))
        self.Hm, self.Wm = 3, 4
        return 3, 4

    def splat(self, views, Js, first_ordinal, plain_atomic=False):
        assert len(views) == len(Js)
        self.log.append(('splat', first_ordinal, len(views)))
        if plain_atomic:
            self.plain.append('splat')

    def resolve(self, views, Js, first_ordinal):
        assert len(views) == len(Js)
        self.log.append(('resolve', first_ordinal, len(views)))

    def gather(self, views, Js, first_ordinal):
        assert len(views) == len(Js)
        self.log.append(('gather', first_ordinal, len(views)))

    def accumulate(self, views, Js, first_ordinal, plain=False):
        assert len(views) == len(Js)
        self.log.append(('accumulate', first_ordinal, len(views)))
        if plain:
            self.plain.append('accumulate')

    def normalize(self, check=True):
        assert check
        self.log.append(('normalize', None, None))

    def fill(self, R):
        self.log.append(('fill', None, None))
        self.filled.append(R)
        return 1


@pytest.fixture
def recorder(monkeypatch):
    for name in ('log', 'plain', 'begun', 'filled'):
        monkeypatch.setattr(Recorder, name, [])
    monkeypatch.setattr(engine, 'Mosaic', Recorder)
    return Recorder


VIEWS = [SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')), name=f'v{i}') for i in range(5)]
JS = [object() for _ in VIEWS]

NEW = [('Mosaic', None, None)]
BOUNDS = [('add_bounds', None, 2), ('add_bounds', None, 2), ('add_bounds', None, 1)]
BEGIN = [('begin', None, None)]
SPLAT = [('splat', 0, 2), ('splat', 2, 2), ('splat', 4, 1)]
RESOLVE = [('resolve', 0, 2), ('resolve', 2, 2), ('resolve', 4, 1)]
GATHER = [('gather', 0, 2), ('gather', 2, 2), ('gather', 4, 1)]
ACCUMULATE = [('accumulate', 0, 2), ('accumulate', 2, 2), ('accumulate', 4, 1)]
NORMALIZE = [('normalize', None, None)]
FILL = [('fill', None, None)]
BEST_VIEW = NEW + BOUNDS + BEGIN + SPLAT + RESOLVE + GATHER


def run(**kw):
    return engine.mosaic_of(VIEWS, JS, torch.eye(3), 0.25, batch=2, **kw)


def test_the_best_view_alone(recorder):
    m = run()
    assert isinstance(m, recorder)
    assert recorder.log == BEST_VIEW
    assert recorder.begun == [(None, None, None)] and not recorder.plain and not recorder.filled


def test_every_batch_holds_its_own_views_and_images(recorder, monkeypatch):
    seen = []
    monkeypatch.setattr(recorder, 'gather', lambda self, views, Js, first: seen.append((first, [v.name for v in views], [JS.index(J) for J in Js])))
    run()
    assert seen == [(0, ['v0', 'v1'], [0, 1]), (2, ['v2', 'v3'], [2, 3]), (4, ['v4'], [4])]


def test_with_a_blend(recorder):
    run(blend=0.5)
    assert recorder.log == BEST_VIEW + ACCUMULATE + NORMALIZE
    assert recorder.begun == [(None, 0.5, None)] and not recorder.plain


def test_with_a_blend_and_a_feather(recorder):
    run(blend=0.5, feather=8)
    assert recorder.log == BEST_VIEW + ACCUMULATE + NORMALIZE
    assert recorder.begun == [(None, 0.5, 8)]


def test_with_a_fill(recorder):
    run(fill=0.75)
    assert recorder.log == BEST_VIEW + FILL
    assert recorder.begun == [(None, None, None)] and recorder.filled == [0.75]


def test_with_all_three(recorder):
    run(blend=0.5, feather=8, fill=0.75)
    assert recorder.log == BEST_VIEW + ACCUMULATE + NORMALIZE + FILL
    assert recorder.begun == [(None, 0.5, 8)] and recorder.filled == [0.75]


def test_given_bounds_take_the_place_of_the_bounds_phase(recorder):
    bounds = (0.0, 0.0, 1.0, 2.0)
    run(bounds=bounds, blend=0.5)
    assert recorder.log == NEW + BEGIN + SPLAT + RESOLVE + GATHER + ACCUMULATE + NORMALIZE
    assert recorder.begun == [(bounds, 0.5, None)]


def test_plain_atomic_reaches_the_splat_and_the_accumulate(recorder):
    run(blend=0.5, plain_atomic=True)
    assert recorder.log == BEST_VIEW + ACCUMULATE + NORMALIZE
    assert recorder.plain == ['splat'] * 3 + ['accumulate'] * 3
    recorder.plain.clear()
    run(plain_atomic=True)
    assert recorder.plain == ['splat'] * 3


@pytest.mark.parametrize('kw, text', [
    ({'blend': 0.0}, 'mosaic blend depth H must be finite and within [1e-06, 1e+06] metres, not 0.0'),
    ({'blend': float('nan')}, 'mosaic blend depth H must be finite and within [1e-06, 1e+06] metres, not nan'),
    ({'fill': 2e6}, 'mosaic fill reach R must be finite and within [1e-06, 1e+06] metres, not 2000000.0'),
    ({'blend': 0.5, 'feather': 1025}, 'mosaic feather width F must be an integer within [1, 1024] source pixels, not 1025'),
    ({'blend': 0.5, 'feather': 2.5}, 'mosaic feather width F must be an integer within [1, 1024] source pixels, not 2.5'),
    ({'feather': 8}, 'mosaic_of: a feather is a factor of the blend\'s weight; give the blend depth too (blend=H)'),
    # the order: blend, fill, the feather's value, then a feather without a blend
    ({'blend': 0.0, 'fill': 0.0, 'feather': 0}, 'mosaic blend depth H must be finite and within [1e-06, 1e+06] metres, not 0.0'),
    ({'fill': 0.0, 'feather': 0}, 'mosaic fill reach R must be finite and within [1e-06, 1e+06] metres, not 0.0'),
    ({'feather': 0}, 'mosaic feather width F must be an integer within [1, 1024] source pixels, not 0'),
])
def test_a_bad_value_is_refused_before_a_mosaic_is_made(recorder, kw, text):
    with pytest.raises(ValueError) as e:
        run(**kw)
    assert str(e.value) == text
    assert recorder.log == []


def test_no_view_and_too_many_are_refused_before_a_mosaic_is_made(recorder):
    with pytest.raises(ValueError, match='mosaic_of: no view'):
        engine.mosaic_of([], [], torch.eye(3), 0.25)
    many = [VIEWS[0]] * (engine.MAX_VIEWS + 1)
    with pytest.raises(ValueError, match=f'mosaic_of: {engine.MAX_VIEWS + 1} images, at most {engine.MAX_VIEWS}'):
        engine.mosaic_of(many, many, torch.eye(3), 0.25)
    assert recorder.log == []
