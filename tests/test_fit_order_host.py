"""The order in which the fit stage calls the engine, on a recording fake in place of the restoration: ``adam`` with its refit
rounds and the quality pass, and the survey's enqueue for one image, for a chunk whose images run different numbers of rounds
and for a light-model image next to plain ones.  The expected sequences are literals, recorded from this test body before the
four copies of the refit loop and the two ways to enqueue a fit were merged; printed lines are part of them.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sucre_amd import engine, sucre

T = 3   # iterations per fit


class Recorder:
    """A workspace that only writes down what it is asked, with the image it belongs to, and returns small CPU tensors."""

    def __init__(self, name, log, light=False):
        self.name, self.log, self.light, self.float_colour = name, log, light, False
        self.H, self.W, self.obs_format = 6, 8, 'f32'

    def fit(self, n, lr=0.05, use_closed_form=False, keep_J=False):
        self.log.append(('fit', self.name, n))
        return torch.zeros((n, 10), dtype=torch.float64)

    def residuals(self):
        self.log.append(('residuals', self.name))
        return torch.zeros((6, 8), dtype=torch.int32), torch.zeros((6, 8, 3)), torch.zeros((2, 4), dtype=torch.float64)

    def trim_outliers(self, k, residuals=None):
        self.log.append(('trim_outliers', self.name, k, residuals is not None))
        return torch.zeros((6, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(3)

    def view_gains(self, limit):
        self.log.append(('view_gains', self.name, limit))
        return torch.ones((2, 3), dtype=torch.float64), torch.ones((2, 3)), torch.zeros((2, 6), dtype=torch.float64)

    def apply_view_gains(self, inv):
        self.log.append(('apply_view_gains', self.name))
        return torch.zeros(2, dtype=torch.int64)

    def view_keep(self):
        self.log.append(('view_keep', self.name))
        return torch.ones(2, dtype=torch.int32)

    def n_obs_device(self):
        self.log.append(('n_obs_device', self.name))
        return torch.zeros(1, dtype=torch.int64)


@pytest.fixture
def log(monkeypatch):
    """The engine's side of the fit stage replaced by the recorder; ``begin`` tells whether the start came with the call
    (the survey: ``params0``) or is read from the module (``adam``: two positional arguments)."""
    log = []

    def begin(model, matches_data, **kw):
        assert set(kw) <= {'params0'}
        log.append(('begin', model.resto.name, 'params0' if kw.get('params0') is not None else 'module'))
        return model.resto

    def fit_batch(restorations, num_iter=200, lr=0.05, use_closed_form=False, **kw):
        log.append(('fit_batch', tuple(r.name for r in restorations), num_iter))
        return [torch.zeros((num_iter, 10), dtype=torch.float64) for _ in restorations]

    monkeypatch.setattr(sucre, '_adam_begin', begin)
    monkeypatch.setattr(engine, 'fit_batch', fit_batch)
    monkeypatch.setattr(sucre, '_pull_results', lambda model, resto: log.append(('pull', resto.name)))
    monkeypatch.setattr(sucre, '_log_trace', lambda trace, first: log.append(('trace', len(trace), first)))
    return log


def model_of(name, log, light=False):
    return SimpleNamespace(resto=Recorder(name, log, light), use_closed_form=False, light_model=light)


def job_of(name, log, light=False, **extras):
    return sucre._Job(image=SimpleNamespace(name=name + '.png'), sucre=model_of(name, log, light), matches_data=None, num_iter=T, lr=0.05,
                      params0=np.full(9, 0.1, np.float32), extras=sucre._Extras(**extras))


def lines(capsys):
    return capsys.readouterr().out.splitlines()


FIRST = 'Solve least squares with Adam optimizer (3 iterations).'


def trim_round(name, k=3.0):
    return [('n_obs_device', name), ('view_keep', name), ('residuals', name), ('trim_outliers', name, k, True)]


def gain_round(name, limit=2.0):
    return [('view_keep', name), ('view_gains', name, limit), ('apply_view_gains', name)]


def quality(name):
    return [('residuals', name), ('view_keep', name)]


# ---- adam ------------------------------------------------------------------------------------------------------------------
def test_adam_with_two_trim_rounds(log, capsys):
    model = model_of('a', log)
    sucre.adam(model, None, num_iter=T, trim_outliers=3.0, trim_rounds=2)
    assert log == ([('begin', 'a', 'module'), ('fit', 'a', 3), ('trace', 3, 0)]
                   + trim_round('a') + [('begin', 'a', 'module'), ('fit', 'a', 3), ('trace', 3, 0)]
                   + trim_round('a') + [('begin', 'a', 'module'), ('fit', 'a', 3), ('trace', 3, 0)]
                   + [('pull', 'a')])
    assert lines(capsys) == [FIRST, 'Solve least squares with Adam optimizer (3 iterations) after trim round 1.',
                             'Solve least squares with Adam optimizer (3 iterations) after trim round 2.']
    assert len(model._trim) == 2 and not hasattr(model, '_gains')


def test_adam_with_two_gain_rounds(log, capsys):
    model = model_of('a', log)
    sucre.adam(model, None, num_iter=T, view_gains=True, gain_rounds=2, gain_limit=1.5, verbose=False)
    assert log == ([('begin', 'a', 'module'), ('fit', 'a', 3)]
                   + gain_round('a', 1.5) + [('begin', 'a', 'module'), ('fit', 'a', 3)]
                   + gain_round('a', 1.5) + [('begin', 'a', 'module'), ('fit', 'a', 3)]
                   + [('pull', 'a')])
    assert lines(capsys) == [FIRST, 'Solve least squares with Adam optimizer (3 iterations) after gain round 1.',
                             'Solve least squares with Adam optimizer (3 iterations) after gain round 2.']
    assert len(model._gains) == 2 and not hasattr(model, '_trim')


def test_adam_with_the_quality_pass(log, capsys):
    model, job = model_of('a', log), sucre._Job(extras=sucre._Extras(save_quality=True, trim_outliers=2.5))
    sucre.adam(model, None, num_iter=T, _job=job)
    assert log == ([('begin', 'a', 'module'), ('fit', 'a', 3), ('trace', 3, 0)]
                   + trim_round('a', 2.5) + [('begin', 'a', 'module'), ('fit', 'a', 3), ('trace', 3, 0)]
                   + quality('a') + [('pull', 'a')])
    assert lines(capsys) == [FIRST, 'Solve least squares with Adam optimizer (3 iterations) after trim round 1.']
    assert len(job.quality) == 4 and len(job.trim) == 1 and job.trim is model._trim and job.gains is None


# ---- the survey's enqueue --------------------------------------------------------------------------------------------------
ONE_JOB = {
    'plain': (dict(), [('begin', 'a', 'params0'), ('fit', 'a', 3)]),
    'trim': (dict(trim_outliers=3.0, trim_rounds=2, save_quality=True),
             [('begin', 'a', 'params0'), ('fit', 'a', 3)] + trim_round('a') + [('begin', 'a', 'params0'), ('fit', 'a', 3)]
             + trim_round('a') + [('begin', 'a', 'params0'), ('fit', 'a', 3)] + quality('a')),
    'gains': (dict(view_gains=True, gain_rounds=2, save_quality=True),
              [('begin', 'a', 'params0'), ('fit', 'a', 3)] + gain_round('a') + [('begin', 'a', 'params0'), ('fit', 'a', 3)]
              + gain_round('a') + [('begin', 'a', 'params0'), ('fit', 'a', 3)] + quality('a')),
}


@pytest.mark.parametrize('case', list(ONE_JOB))
def test_one_image_alone_and_as_a_chunk_of_one(log, capsys, case):
    """Recorded while the code had two entries, one for an image -- which the survey took for a chunk of one -- and one for a
    chunk: both made these calls and left these records for a chunk of one.  The lines differed: the entry for one image
    announced the fit once, the entry for a chunk every refit too.  A chunk of one keeps what the survey printed for it."""
    extras, calls = ONE_JOB[case]
    job = job_of('a', log, **extras)
    sucre._restore_enqueue_fits([job])
    assert lines(capsys) == [FIRST]
    assert (log, job.trace.shape, job.quality is not None, None if job.trim is None else len(job.trim),
            None if job.gains is None else len(job.gains)) == (calls, (3, 10), case != 'plain', 2 if case == 'trim' else None,
                                                               2 if case == 'gains' else None)


def test_a_chunk_whose_images_trim_different_numbers_of_rounds(log, capsys):
    """Three images of one size in one launch; c stops a round early, so the second round's launch holds two."""
    jobs = [job_of(n, log, trim_outliers=3.0, trim_rounds=r, save_quality=(n == 'b')) for n, r in (('a', 2), ('b', 2), ('c', 1))]
    sucre._restore_enqueue_fits(jobs)
    assert log == ([('begin', n, 'params0') for n in 'abc'] + [('fit_batch', ('a', 'b', 'c'), 3)]
                   + trim_round('a') + [('begin', 'a', 'params0')] + trim_round('b') + [('begin', 'b', 'params0')]
                   + trim_round('c') + [('begin', 'c', 'params0')] + [('fit_batch', ('a', 'b', 'c'), 3)]
                   + trim_round('a') + [('begin', 'a', 'params0')] + trim_round('b') + [('begin', 'b', 'params0')]
                   + [('fit_batch', ('a', 'b'), 3)] + quality('b'))
    assert lines(capsys) == ['Solve least squares with Adam optimizer (3 iterations), 3 images per launch.'] * 2 \
        + ['Solve least squares with Adam optimizer (3 iterations), 2 images per launch.']
    assert [len(j.trim) for j in jobs] == [2, 2, 1] and [j.gains for j in jobs] == [None] * 3
    assert [j.quality is not None for j in jobs] == [False, True, False] and all(j.trace.shape == (3, 10) for j in jobs)


def test_a_chunk_whose_last_gain_round_is_left_to_one_image(log, capsys):
    """Three images of one size, one of them without gains at all: the round that only a runs is fitted by itself."""
    jobs = [job_of('a', log, view_gains=True, gain_rounds=2, gain_limit=1.5), job_of('b', log, view_gains=True), job_of('c', log)]
    sucre._restore_enqueue_fits(jobs)
    assert log == ([('begin', n, 'params0') for n in 'abc'] + [('fit_batch', ('a', 'b', 'c'), 3)]
                   + gain_round('a', 1.5) + [('begin', 'a', 'params0')] + gain_round('b') + [('begin', 'b', 'params0')]
                   + [('fit_batch', ('a', 'b'), 3)]
                   + gain_round('a', 1.5) + [('begin', 'a', 'params0'), ('fit', 'a', 3)])
    assert lines(capsys) == ['Solve least squares with Adam optimizer (3 iterations), 3 images per launch.',
                             'Solve least squares with Adam optimizer (3 iterations), 2 images per launch.', FIRST]
    assert [None if j.gains is None else len(j.gains) for j in jobs] == [2, 1, None] and [j.trim for j in jobs] == [None] * 3


def test_a_light_model_image_next_to_two_plain_ones(log, capsys):
    """The light model is fitted by itself, behind the launch the two plain images share; every image trims one round."""
    jobs = [job_of(n, log, light=(n == 'l'), trim_outliers=3.0, save_quality=True) for n in ('l', 'a', 'b')]
    sucre._restore_enqueue_fits(jobs)
    assert log == ([('begin', n, 'params0') for n in 'lab'] + [('fit_batch', ('a', 'b'), 3)]
                   + trim_round('a') + [('begin', 'a', 'params0')] + trim_round('b') + [('begin', 'b', 'params0')]
                   + [('fit_batch', ('a', 'b'), 3)] + quality('a') + quality('b')
                   + [('fit', 'l', 3)] + trim_round('l') + [('begin', 'l', 'params0'), ('fit', 'l', 3)] + quality('l'))
    assert lines(capsys) == ['Solve least squares with Adam optimizer (3 iterations), 2 images per launch.'] * 2 + [FIRST] * 2
    assert [len(j.trim) for j in jobs] == [1, 1, 1]
