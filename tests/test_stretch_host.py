"""CPU tier of the common colour stretch (--common-stretch, --stretch-from): the float64 percentile plan of a pool, the stretch
file, the refusals of the command line and SUCRe.plot_J with a fixed stretch on a host J.  Every comparison is exact; the
yardstick is numpy, written out here."""
import builtins
import io
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from sucre_amd import sucre
from sucre_amd.engine import _lerp64

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def same(a, b):
    """== on float32 values (-0.0 == 0.0 counts as equal: np.sort does not order the two zeros)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and bool(np.all(a == b))


@pytest.mark.parametrize('n', [1, 2, 3, 100, 101, 9999])
def test_plan64_and_the_float64_lerp_equal_numpy(n):
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * np.float32(2.0) ** rng.integers(-6, 4, n)).astype(np.float32)
    s = np.sort(a)
    for q in (0, 1, 50, 99, 100):
        want = np.percentile(a.astype(np.float64), q).astype(np.float32)
        below, above, t = sucre.percentile_plan64(n, q)
        assert 0 <= below <= above <= n - 1 and above - below <= 1 and 0.0 <= t < 1.0
        got = np.float32(_lerp64(s[below], s[above], t))
        assert same(got, want), (n, q, got, want)


@pytest.mark.parametrize('n', [2 ** 24 + 3, 2 ** 33])
def test_plan64_on_pools_past_float32_indices(n):
    """No array: the ranks are the exact integers (float32 index arithmetic rounds them from 2^24 on), and t is exactly the
    distance of the float64 virtual index from the rank below."""
    for q in (0, 1, 25, 50, 75, 99, 100):
        below, above, t = sucre.percentile_plan64(n, q)
        exact = Fraction(n - 1) * Fraction(q, 100)
        assert below == exact.numerator // exact.denominator, (n, q)
        assert above == min(below + 1, n - 1)
        virtual = float(n - 1) * (q / 100.0)          # Python floats: float64
        assert Fraction(t) == Fraction(virtual) - below and abs(Fraction(t) - (exact - below)) < Fraction(1, 10 ** 6)
    assert sucre.percentile_plan64(2 ** 24 + 3, 99)[0] != int(np.floor(np.float32(2 ** 24 + 2) * np.float32(0.99))), \
        'float32 arithmetic would have rounded this rank'
    with pytest.raises(ValueError):
        sucre.percentile_plan64(0, 50)


def good():
    return {'lo': torch.tensor([0.05, 0.06, 0.07]), 'hi': torch.tensor([0.9, 1.0, 1.1])}


def test_stretch_file_accepted(tmp_path):
    torch.save(good(), tmp_path / 'a.pt')
    lo, hi = sucre.read_stretch_file(tmp_path / 'a.pt')
    assert same(lo, np.float32([0.05, 0.06, 0.07])) and same(hi, np.float32([0.9, 1.0, 1.1]))
    # extra keys (what --common-stretch writes) and float64 values
    torch.save({'lo': good()['lo'].double(), 'hi': good()['hi'].double(), 'q': torch.tensor([1., 99.]), 'n_valid': 7, 'images': ['a.png']},
               tmp_path / 'b.pt')
    lo2, hi2 = sucre.read_stretch_file(tmp_path / 'b.pt')
    assert same(lo2, lo) and same(hi2, hi)
    lo3, hi3 = sucre.check_stretch((lo, hi))
    assert same(lo3, lo) and same(hi3, hi)


@pytest.mark.parametrize('change, words', [
    (lambda s: s.pop('hi'), ["'hi'"]),
    (lambda s: s.update(hi=s['hi'].view(3, 1)), ["'hi'", '(3, 1)']),
    (lambda s: s.update(lo=torch.tensor([0.05, float('nan'), 0.07])), ["'lo'", 'channel G']),
    (lambda s: s.update(hi=torch.tensor([0.9, 1.0, float('inf')])), ["'hi'", 'channel B']),
    (lambda s: s.update(hi=torch.tensor([0.05, 1.0, 1.1])), ['channel R']),      # hi == lo
    (lambda s: s.update(hi=torch.tensor([0.9, 1.0, 0.01])), ['channel B']),      # hi < lo
], ids=['missing-hi', 'shape-3x1', 'nan', 'inf', 'hi-equals-lo', 'hi-below-lo'])
def test_stretch_file_rejected(tmp_path, change, words):
    s = good()
    change(s)
    path = tmp_path / 'bad.pt'
    torch.save(s, path)
    with pytest.raises(SystemExit) as e:
        sucre.read_stretch_file(path)
    msg = str(e.value.code)
    assert '--stretch-from' in msg and str(path) in msg and all(w in msg for w in words), msg
    with pytest.raises(ValueError):
        sucre.check_stretch(s, where='x')


def test_stretch_file_unreadable(tmp_path):
    with pytest.raises(SystemExit) as e:
        sucre.read_stretch_file(tmp_path / 'none.pt')
    assert 'cannot read' in str(e.value.code) and 'none.pt' in str(e.value.code)
    with pytest.raises(ValueError, match='holds no stretch'):
        sucre.check_stretch(5)


def test_flags_parse_and_leave_the_reference_table_alone():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'common_stretch' not in vars(off) and 'stretch_from' not in vars(off)
    on = p.parse_args(BASE + ['--common-stretch'])
    assert on.common_stretch is True and vars(off) == {k: v for k, v in vars(on).items() if k != 'common_stretch'}
    on = p.parse_args(BASE + ['--stretch-from', 's.pt'])
    assert on.stretch_from == Path('s.pt') and vars(off) == {k: v for k, v in vars(on).items() if k != 'stretch_from'}
    text = p.format_help()
    assert '--common-stretch' in text and '--stretch-from PATH' in text
    assert all(a.dest not in ('common_stretch', 'stretch_from') for a in p._actions)


@pytest.mark.parametrize('extra, words', [
    (['--common-stretch'], ['--shared-water', '--apply-water', '--stretch-from']),
    (['--common-stretch', '--shared-water', '--stretch-from', 's.pt'], ['--stretch-from']),
    (['--common-stretch', '--apply-water', 'w.pt', '--stretch-from', 's.pt'], ['--stretch-from']),
    (['--common-stretch', '--shared-water', '--save-interval', '5'], ['--save-interval']),
    (['--common-stretch', '--apply-water', 'w.pt', '--save-interval', '5'], ['--save-interval']),
], ids=['per-image-water', 'with-stretch-from', 'with-stretch-from-apply', 'save-interval', 'save-interval-apply'])
def test_refusals_fire_before_any_file_is_opened(extra, words, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    opened = []
    real_open = builtins.open
    spy = lambda *a, **k: (opened.append(a[0]), real_open(*a, **k))[1]   # noqa: E731
    monkeypatch.setattr(builtins, 'open', spy)
    monkeypatch.setattr(io, 'open', spy)
    monkeypatch.setattr(torch, 'load', lambda *a, **k: opened.append(a[0]))
    out = tmp_path / 'out'
    argv = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
            '--output-dir', str(out), '--image-name', 'x.png'] + extra
    with pytest.raises(SystemExit) as e:
        sucre.main(argv)
    msg = str(e.value.code)
    assert e.value.code != 0 and msg.startswith('--common-stretch') and all(w in msg for w in words), msg
    assert not opened and not out.exists()


def test_a_bad_stretch_file_stops_the_run_before_the_model_is_touched(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    torch.save({'lo': torch.zeros(3), 'hi': torch.zeros(3)}, tmp_path / 's.pt')
    with pytest.raises(SystemExit) as e:
        sucre.main(['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
                    '--output-dir', str(tmp_path / 'out'), '--image-name', 'x.png', '--stretch-from', str(tmp_path / 's.pt')])
    assert '--stretch-from' in str(e.value.code) and 'channel R' in str(e.value.code) and not (tmp_path / 'out').exists()


class _Image:   # what SUCRe.__init__ needs of an image when J is closed-form
    name = 'x.png'


def host_model(J):
    s = sucre.SUCRe(image=_Image(), use_closed_form=True)
    s.J = torch.from_numpy(J)
    return s


def some_J():
    rng = np.random.default_rng(5)
    J = (rng.random((37, 29, 3)) * 1.6 - 0.1).astype(np.float32)
    J[3, 4, 1] = np.nan            # one channel: the whole pixel is invalid
    J[10:13, 7] = np.nan
    J[20, 20] = [0.0, -0.0, 2.5]
    return J


def test_plot_J_with_a_fixed_stretch_on_a_host_J():
    J = some_J()
    lo, hi = np.float32([0.05, 0.1, 0.0]), np.float32([1.2, 0.9, 1.4])
    s = host_model(J.copy())
    s.stretch = (lo, hi)
    got = np.asarray(s.plot_J())
    ok = ~np.isnan(J).any(axis=2)
    want = np.zeros(J.shape, np.uint8)
    for c in range(3):
        x = np.minimum(np.maximum(J[..., c][ok], lo[c]), hi[c])
        assert x.dtype == np.float32
        want[..., c][ok] = np.uint8(((x - lo[c]) / (hi[c] - lo[c])) * np.float32(255))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert not got[3, 4].any() and want[ok].min() == 0 and want[ok].max() == 255
    assert np.array_equal(got, sucre.stretch_picture(J, lo, hi))


def test_plot_J_without_a_stretch_is_the_reference_picture():
    """sucre.py:84-94 restated: per-image percentiles, minimum and maximum."""
    J = some_J()
    s = host_model(J.copy())
    assert s.stretch is None and sucre.SUCRe.stretch is None
    got = np.asarray(s.plot_J())
    ref = J.copy()
    valid = np.all(~np.isnan(ref), axis=2)
    vals = ref[valid]
    vals = np.clip(vals, np.percentile(vals, 1, axis=0), np.percentile(vals, 99, axis=0))
    vals -= vals.min(axis=0)
    vals /= vals.max(axis=0)
    ref[~valid] = 0
    ref[valid] = vals
    assert np.array_equal(got, np.uint8(ref * 255))
