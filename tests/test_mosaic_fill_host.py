"""CPU tier of the mosaic's hole filling: the oracle of the GPU tests (tests/mosaic_fill_ref.py) on grids filled by hand and on
random masks (the two distance properties of the tap pattern), the sign of a zero, ``engine.mosaic_fill_levels``, the --mosaic-fill
flag and what is refused before any file is opened, the three library entries and their argument validation (nothing is launched)."""
import builtins
import ctypes as C
import io
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_fill_ref as fref
from sucre_amd import _lib, engine, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']
NAN = float('nan')


def grid(H, W, cells):
    """An H x W mosaic that is empty but for ``cells``: {(y, x): (J triple, raw triple)}."""
    J = np.full((H, W, 3), NAN, np.float32)
    raw = np.zeros((H, W, 3), np.uint8)
    source = np.full((H, W), -1, np.int32)
    for (y, x), (j, r) in cells.items():
        J[y, x], raw[y, x], source[y, x] = j, r, 0
    return J, raw, source


# ---- the oracle on grids filled by hand -----------------------------------------------------------------------------------------

def test_oracle_on_a_3x3_grid_with_one_valid_cell():
    """Level 1 is 2x2 and only its cell (0,0) -- the parent of (1,1) -- holds anything: Wt = 1, c = the cell's values, w = 0.25.
    Every other cell of level 0 has that parent among its taps (the clamp folds the taps of the border onto it), and with one
    colour among the taps S / A = (A c) / A, exact here: every A is a sum of sixteenths and every value a small dyadic number.
    The whole grid takes the one colour.  At L = 2 level 2 is 1x1 and fills the other three cells of level 1
    with g = 2, which the cells with such a tap report."""
    J, raw, source = grid(3, 3, {(1, 1): ((0.25, 0.5, -1.0), (10, 20, 250))})
    one = fref.fill(J, raw, source, 1)
    assert one['fill_level'].tolist() == [[1, 1, 1], [1, 0, 1], [1, 1, 1]]
    assert np.array_equal(one['J_filled'], np.broadcast_to(np.float32([0.25, 0.5, -1.0]), (3, 3, 3)))
    assert np.array_equal(one['raw_filled'], np.broadcast_to(np.uint8([10, 20, 250]), (3, 3, 3)))
    assert one['pyramid'][0].tolist() == [[0.25, 0.5, -1.0, 10.0, 20.0, 250.0, 0.25, 1.0]] + [[0.0] * 8] * 3
    two = fref.fill(J, raw, source, 2)
    assert two['fill_level'].tolist() == [[1, 2, 2], [2, 0, 2], [2, 2, 2]]
    assert np.array_equal(two['J_filled'], one['J_filled']) and np.array_equal(two['raw_filled'], one['raw_filled'])
    assert two['pyramid'][1].tolist() == [[0.25, 0.5, -1.0, 10.0, 20.0, 250.0, 0.0625, 2.0]]
    assert [r[6:] for r in two['pyramid'][0].tolist()] == [[0.25, 1.0], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0]]
    assert one['J_filled'].dtype == np.float32 and one['raw_filled'].dtype == np.uint8 and one['fill_level'].dtype == np.int32


def test_oracle_on_a_4x4_grid_computed_by_hand():
    """Valid: (0,0) with J_0 = 1, raw_0 = 10 and (0,1) with J_0 = 3, raw_0 = 15.  Level 1 (2x2): cell (0,0) has Wt = 2,
    S = 1 + 3 = 4, c = 2, raw 12.5, w = 0.5, g = 1; its other cells are empty.  L = 1: a cell of level 0 is filled when (0,0) of
    level 1 is among its taps.  Row 3 and column 3 have py = ny = 1 (px = nx = 1) after the clamp: they stay empty; cell (0,2) has
    the taps (0,1), (0,0), (0,1), (0,0): A = 3/16 + 1/16, S = 3/8 + 1/8, c = 2; cell (2,2) has (0,0) as its last tap alone:
    (2 / 16) / (1 / 16) = 2.  raw: rintf(12.5) = 12, halves to even.  L = 2: level 2 (1x1) has Wt = 0.5, S = 0.5 x 2 = 1, c = 2,
    w = 0.125; the push gives the three empty cells of level 1 c = 2 and g = 2, and every empty cell of level 0 has one of them
    among its taps."""
    J, raw, source = grid(4, 4, {(0, 0): ((1.0, -8.0, 0.5), (10, 0, 255)), (0, 1): ((3.0, -4.0, 0.5), (15, 1, 255))})
    one = fref.fill(J, raw, source, 1)
    assert one['fill_level'].tolist() == [[0, 0, 1, -1], [1, 1, 1, -1], [1, 1, 1, -1], [-1, -1, -1, -1]]
    filled = one['fill_level'] > 0
    assert np.array_equal(one['J_filled'][filled], np.broadcast_to(np.float32([2.0, -6.0, 0.5]), (7, 3)))
    assert np.array_equal(one['raw_filled'][filled], np.broadcast_to(np.uint8([12, 0, 255]), (7, 3)))    # 12.5 -> 12, 0.5 -> 0
    empty = one['fill_level'] < 0
    assert np.isnan(one['J_filled'][empty]).all() and not one['raw_filled'][empty].any()
    assert one['J_filled'][empty].view(np.uint32).tolist() == [[0x7fc00000] * 3] * 7
    assert one['J_filled'][0, :2].tolist() == [[1.0, -8.0, 0.5], [3.0, -4.0, 0.5]] and one['raw_filled'][0, :2].tolist() == [[10, 0, 255], [15, 1, 255]]
    assert one['pyramid'][0].tolist() == [[2.0, -6.0, 0.5, 12.5, 0.5, 255.0, 0.5, 1.0]] + [[0.0] * 8] * 3
    two = fref.fill(J, raw, source, 2)
    assert two['fill_level'].tolist() == [[0, 0, 2, 2], [2, 2, 2, 2], [2, 2, 2, 2], [2, 2, 2, 2]]
    assert np.array_equal(two['J_filled'][two['fill_level'] > 0], np.broadcast_to(np.float32([2.0, -6.0, 0.5]), (14, 3)))
    assert two['pyramid'][1].tolist() == [[2.0, -6.0, 0.5, 12.5, 0.5, 255.0, 0.125, 2.0]]


def test_a_measured_cell_without_a_finite_colour_contributes_nothing_and_is_kept():
    inf = float('inf')
    J, raw, source = grid(2, 2, {(0, 0): ((0.5, 0.25, 1.0), (1, 2, 3)), (0, 1): ((inf, 0.0, 0.0), (9, 9, 9)), (1, 0): ((0.0, NAN, 0.0), (7, 7, 7))})
    out = fref.fill(J, raw, source, 1)
    assert out['fill_level'].tolist() == [[0, 0], [0, 1]]
    assert out['J_filled'][1, 1].tolist() == [0.5, 0.25, 1.0] and out['raw_filled'][1, 1].tolist() == [1, 2, 3]
    assert np.array_equal(out['J_filled'][:, :1].view(np.uint32), J[:, :1].view(np.uint32)) and out['J_filled'][0, 1, 0] == inf
    assert np.isnan(out['J_filled'][1, 0, 1]) and out['raw_filled'][0, 1].tolist() == [9, 9, 9]
    assert out['pyramid'][0].tolist() == [[0.5, 0.25, 1.0, 1.0, 2.0, 3.0, 0.25, 1.0]]


@pytest.mark.parametrize('where', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_a_negative_zero_enters_the_sums_as_a_positive_one(where):
    """All four terms are always added, and an empty record holds +0.0f: -0.0f + 0.0f = +0.0f in any position, so the pyramid and
    the filled cells hold +0.0f while the measured cell keeps its bits."""
    J, raw, source = grid(2, 2, {where: ((-0.0, 0.0, -0.0), (0, 0, 0))})
    out = fref.fill(J, raw, source, 1)
    assert out['pyramid'][0].view(np.uint32).tolist() == [[0, 0, 0, 0, 0, 0, np.float32(0.25).view(np.uint32), np.float32(1).view(np.uint32)]]
    filled = out['fill_level'] > 0
    assert int(filled.sum()) == 3 and not out['J_filled'][filled].view(np.uint32).any()
    assert out['J_filled'][where].view(np.uint32).tolist() == [0x80000000, 0, 0x80000000]
    # and the rule itself, which numpy shares with the device: IEEE round-to-nearest
    assert not np.signbit(np.float32(-0.0) + np.float32(0.0)) and np.signbit(np.float32(1) * np.float32(-0.0))


def random_case(H, W, seed, share=0.02):
    rng = np.random.default_rng(seed)
    valid = rng.random((H, W)) < share
    J = rng.random((H, W, 3), dtype=np.float32)
    raw = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    J[~valid], raw[~valid] = NAN, 0
    return J, raw, np.where(valid, rng.integers(0, 7, (H, W)), -1).astype(np.int32)


@pytest.mark.parametrize('L', [2, 3, 4])
@pytest.mark.parametrize('H, W', [(37, 53), (200, 300)])
def test_the_two_distance_properties_on_random_masks(H, W, L):
    """2 % of the cells valid: every empty cell within 2^(L-1) cells (Chebyshev) of a valid one is filled, none at 3 x 2^L or
    more from every valid one -- asserted by the reference itself (``check_distances``) and once more here, by brute force over the
    valid cells."""
    J, raw, source = random_case(H, W, 100 * L + H)
    out = fref.fill(J, raw, source, L)     # check=True: the reference asserts both
    valid = source >= 0
    ys, xs = np.nonzero(valid)
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.full((H, W), 1 << 30)
    for y, x in zip(ys, xs):
        d = np.minimum(d, np.maximum(np.abs(yy - y), np.abs(xx - x)))
    filled = out['fill_level'] > 0
    assert np.array_equal(out['fill_level'] == 0, valid)
    assert filled[(d <= 1 << (L - 1)) & ~valid].all()
    assert not filled[d >= 3 * (1 << L)].any()
    assert np.isfinite(out['J_filled'][filled]).all() and np.isnan(out['J_filled'][out['fill_level'] < 0]).all()
    # a filled value is a mean with positive weights of valid values: inside their range (to a few roundings)
    assert out['J_filled'][filled].min() >= J[valid].min() - 1e-5 and out['J_filled'][filled].max() <= J[valid].max() + 1e-5


def test_the_distance_checks_can_fail():
    valid = np.zeros((9, 9), bool)
    valid[4, 4] = True
    nothing = np.zeros((9, 9), bool)
    with pytest.raises(AssertionError, match='stayed empty'):
        fref.check_distances(valid, valid, nothing, 1)
    everything = ~valid
    with pytest.raises(AssertionError, match='was filled'):
        fref.check_distances(np.pad(valid, 8), np.pad(valid, 8), np.pad(everything, 8, constant_values=True), 1)


# ---- the levels ---------------------------------------------------------------------------------------------------------------------

def test_levels_at_exact_powers_of_two_and_at_the_cap():
    f = engine.mosaic_fill_levels
    # gsd 0.5 m: gsd 2^L >= R first holds at L = 1 for R <= 1, L = 2 for R <= 2, ...
    assert [f(R, 0.5, 1000, 1000) for R in (1e-6, 0.5, 1.0, 1.0000001, 2.0, 2.0000001, 4.0, 8.0, 8.5, 16.0)] == [1, 1, 1, 2, 2, 3, 3, 4, 5, 5]
    assert f(0.75, np.float32(0.1), 1000, 1000) == 3 and f(0.8, np.float32(0.1), 1000, 1000) == 3    # float32(0.1) > 0.1: 8 gsd >= 0.8
    assert f(0.8, 0.1, 1000, 1000) == 3 and f(0.8000001, 0.1, 1000, 1000) == 4
    # the cap: the first level that is 1x1, and at least 1
    assert f(1e6, 0.5, 64, 64) == 6 and f(1e6, 0.5, 65, 64) == 7 and f(1e6, 0.5, 1, 9) == 4 and f(1e6, 0.5, 5, 1) == 3
    assert f(1e6, 0.5, 1, 1) == 1 and f(1e6, 0.5, 2, 2) == 1 and f(1e6, 0.5, 3, 2) == 2
    assert f(1e6, 1e-6, 1 << 24, 1 << 24) == 24     # the most the library takes
    for R, gsd, H, W in ((1.0, 0.5, 1000, 1000), (3.0, 0.07, 37, 53), (1e6, 0.5, 64, 64), (1e6, 0.5, 257, 129), (5.0, 0.01, 1, 1), (1e6, 1.0, 5, 1)):
        assert f(R, gsd, H, W) == fref.levels_for(R, gsd, H, W), (R, gsd, H, W)
    assert fref.level_sizes(257, 129, 4) == [(257, 129), (129, 65), (65, 33), (33, 17), (17, 9)]
    for bad in (0.0, -1.0, NAN, float('inf'), 9e-7, 1.1e6, 'wide'):
        with pytest.raises(ValueError, match='fill reach R'):
            f(bad, 0.5, 10, 10)
    with pytest.raises(ValueError, match='gsd'):
        f(1.0, 0.0, 10, 10)


# ---- the flag and what it refuses -----------------------------------------------------------------------------------------------

def test_flag_lives_in_extras_and_leaves_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'mosaic_fill' not in vars(off)
    on = p.parse_args(BASE + ['--mosaic', 'results', '--mosaic-fill', '0.5'])
    assert on.mosaic_fill == 0.5
    assert vars(off) == {k: v for k, v in vars(on).items() if k not in ('mosaic', 'mosaic_fill')}
    assert vars(p.parse_args(BASE + ['--mosaic', 'results'])) == {k: v for k, v in vars(on).items() if k != 'mosaic_fill'}
    assert all(a.dest != 'mosaic_fill' for a in p._actions)
    assert '--mosaic-fill R' in p.format_help() and 'mosaic_filled.png' in p.format_help()


def run_refused(argv, tmp_path, monkeypatch):
    opened = []
    real_open = builtins.open
    spy = lambda *a, **k: (opened.append(a[0]), real_open(*a, **k))[1]   # noqa: E731
    monkeypatch.setattr(builtins, 'open', spy)
    monkeypatch.setattr(io, 'open', spy)   # (pathlib's read_text / open)
    monkeypatch.setattr(torch, 'load', lambda *a, **k: opened.append(a[0]))
    out = tmp_path / 'out'
    base = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
            '--output-dir', str(out), '--image-name', 'x.png']
    with pytest.raises(SystemExit) as e:
        sucre.main(base + argv)
    assert e.value.code != 0 and not opened and not out.exists()
    return str(e.value.code)


def test_mosaic_fill_needs_mosaic(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert '--mosaic-fill: only with --mosaic' in run_refused(['--mosaic-fill', '0.1'], tmp_path, monkeypatch)


@pytest.mark.parametrize('R', ['0', '-1', 'nan', 'inf', '9e-7', '1.1e6'])
def test_a_reach_outside_the_range_is_refused_before_any_file_is_opened(R, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-fill', R], tmp_path, monkeypatch)
    assert message.startswith('--mosaic-fill: R must be a finite reach within [1e-06, 1e+06] metres, not ')


REFUSED = [(['--shared-water'], '--shared-water'), (['--apply-water', 'w.pt'], '--apply-water'), (['--check-consistency', 'r'], '--check-consistency'),
           (['--common-stretch'], '--common-stretch'), (['--image-scale', '0.5'], '--image-scale'), (['--mosaic-gsd', '0'], '--mosaic-gsd'),
           (['--mosaic-blend', '0'], '--mosaic-blend')]


@pytest.mark.parametrize('extra, named', REFUSED, ids=[' '.join(e) for e, _ in REFUSED])
def test_what_mosaic_refuses_stays_refused_with_a_fill(extra, named, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-fill', '0.5'] + extra, tmp_path, monkeypatch)
    assert '--mosaic' in message and named in message and '--mosaic-fill' not in message


def test_a_world_above_one_stays_refused_with_a_fill(tmp_path, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-fill', '0.5'], tmp_path, monkeypatch)
    assert '--mosaic' in message and 'world size of 2' in message


def test_the_reach_is_checked_by_the_functions_too(tmp_path, monkeypatch):
    for bad in (0.0, -1.0, NAN, float('inf'), 9e-7, 1.1e6, 'wide'):
        with pytest.raises(ValueError, match='fill reach R'):
            engine.mosaic_fill_reach(bad)
        with pytest.raises(ValueError, match='fill reach R'):
            engine.mosaic_of([SimpleNamespace()], [None], torch.eye(3), 0.1, fill=bad)   # before the device is looked at
    assert engine.mosaic_fill_reach(1e-6) == 1e-6 and engine.mosaic_fill_reach(1e6) == 1e6 and engine.mosaic_fill_reach(2) == 2.0
    assert engine.MOSAIC_FILL_RANGE == engine.MOSAIC_BLEND_RANGE
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda *a, **k: None)
    with pytest.raises(SystemExit) as e:
        sucre.mosaic([SimpleNamespace(name='a.png')], None, tmp_path / 'results', tmp_path / 'out', fill=0.0)
    assert str(e.value.code).startswith('--mosaic-fill: ') and not (tmp_path / 'out').exists()


# ---- the library: the entries exist and check their arguments before any launch -------------------------------------------------

def test_abi_has_the_fill_entries_and_keeps_its_version():
    for name in ('sucre_mosaic_fill_bytes', 'sucre_mosaic_fill_pull', 'sucre_mosaic_fill_push'):
        assert name in _lib.SIGNATURES
    assert _lib.load().sucre_version() == 2 == _lib.ABI_VERSION
    header = (Path(__file__).resolve().parent.parent / 'include' / 'sucre_hip.h').read_text()
    assert 'size_t sucre_mosaic_fill_bytes(int Hm, int Wm, int levels);' in header and '0x7fc00000' in header


def test_pyramid_bytes():
    lib = _lib.load()
    assert lib.sucre_mosaic_fill_bytes(1, 1, 1) == 256 and lib.sucre_mosaic_fill_bytes(1, 1, 24) == 24 * 256
    assert lib.sucre_mosaic_fill_bytes(64, 64, 6) == 32 * (1024 + 256 + 64 + 16) + 2 * 256     # 4 and 1 records round up to 256 bytes
    for H, W, L in ((37, 53, 1), (37, 53, 3), (257, 129, 4), (5, 1, 3), (1, 9, 4), (1080, 1920, 7)):
        assert lib.sucre_mosaic_fill_bytes(H, W, L) == fref.pyramid_bytes(H, W, L), (H, W, L)
    for H, W, L, what in ((0, 4, 1, b'cells'), (4, (1 << 24) + 1, 1, b'cells'), (1 << 20, 1 << 20, 1, b'2^39'), (4, 4, 0, b'levels=0'),
                          (4, 4, 25, b'levels=25'), (4, 4, -1, b'levels')):
        assert lib.sucre_mosaic_fill_bytes(H, W, L) == 0 and what in lib.sucre_last_error(), (H, W, L)


def test_argument_validation_happens_before_any_launch():
    lib = _lib.load()
    ERR = -1   # SUCRE_ERR_ARG
    p = C.c_void_p(4096)
    odd = C.c_void_p(4098)

    def pull(Hm=4, Wm=4, levels=2, J=p, raw=p, source=p, pyramid=p):
        return lib.sucre_mosaic_fill_pull(Hm, Wm, levels, J, raw, source, pyramid, None)

    def push(Hm=4, Wm=4, levels=2, J=p, raw=p, source=p, pyramid=p, J_filled=p, raw_filled=p, level_out=p):
        return lib.sucre_mosaic_fill_push(Hm, Wm, levels, J, raw, source, pyramid, J_filled, raw_filled, level_out, None)

    for call in (pull, push):
        assert call(Hm=0) == ERR and b'cells' in lib.sucre_last_error()
        assert call(Wm=(1 << 24) + 1) == ERR and b'cells' in lib.sucre_last_error()
        assert call(Hm=1 << 20, Wm=1 << 20) == ERR and b'2^39' in lib.sucre_last_error()
        for levels in (0, -3, 25):
            assert call(levels=levels) == ERR and b'levels=' in lib.sucre_last_error(), levels
        assert call(J=None) == ERR and b'J is NULL' in lib.sucre_last_error()
        assert call(J=odd) == ERR and b'J is NULL or not 4-byte aligned' in lib.sucre_last_error()
        assert call(raw=None) == ERR and b'raw is NULL' in lib.sucre_last_error()
        assert call(source=None) == ERR and b'source is NULL' in lib.sucre_last_error()
        assert call(source=odd) == ERR and b'source' in lib.sucre_last_error()
        assert call(pyramid=None) == ERR and b'pyramid_dev is NULL' in lib.sucre_last_error()
        assert call(pyramid=C.c_void_p(4096 + 128)) == ERR and b'256-byte aligned' in lib.sucre_last_error()
    assert push(J_filled=None) == ERR and b'J_filled is NULL' in lib.sucre_last_error()
    assert push(J_filled=odd) == ERR and b'J_filled' in lib.sucre_last_error()
    assert push(raw_filled=None) == ERR and b'raw_filled is NULL' in lib.sucre_last_error()
    assert push(level_out=None) == ERR and b'level_out is NULL' in lib.sucre_last_error()
    assert push(level_out=odd) == ERR and b'level_out' in lib.sucre_last_error()
