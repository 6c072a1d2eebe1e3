"""CPU tier of the blended seabed mosaic: the oracle of the GPU tests (tests/mosaic_blend_ref.py) against a blend computed by hand,
the --mosaic-blend flag and what is refused before any file is opened, the two library entries and their argument validation
(nothing is launched)."""
import builtins
import ctypes as C
import io
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_blend_ref as bref
from sucre_amd import _lib, engine, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


# ---- the oracle on a blend computed by hand -------------------------------------------------------------------------------------

def plane_view(depth, J, rgb):
    """A 4x4 camera with K = [[2^20,0,2],[0,2^20,2],[0,0,1]] (its inverse given: dyadic), identity pose, looking at a plane at
    ``depth``: pixel (u, v) is the camera point depth ((u - 1.5) 2^-20, (v - 1.5) 2^-20, 1), and x^2 + y^2 <= 4.5 x 2^-40 x depth^2
    vanishes next to depth^2 in float32 -- the range of every pixel is ``depth`` to the bit."""
    K = torch.tensor([[2.0 ** 20, 0.0, 2.0], [0.0, 2.0 ** 20, 2.0], [0.0, 0.0, 1.0]])
    Kinv = torch.tensor([[2.0 ** -20, 0.0, -(2.0 ** -19)], [0.0, 2.0 ** -20, -(2.0 ** -19)], [0.0, 0.0, 1.0]])
    return SimpleNamespace(depth=torch.full((4, 4), depth), rgb=torch.tensor(rgb, dtype=torch.uint8).expand(4, 4, 3).contiguous(),
                           K=K, Kinv=Kinv, R=torch.eye(3), t=torch.zeros(3, 1)), torch.tensor(J).expand(4, 4, 3).contiguous()


def test_oracle_on_a_blend_computed_by_hand():
    """Two views of one cell (gsd 1 m, footprints of micrometres), ranges 1 and 1.5, H = 1: the near view's 16 pixels have d = 0,
    t = 1, wq = 4096; the far view's d = 0.5, t = 0.5, t^2 = 0.25, wq = 1024.  wsum = 16 x 4096 + 16 x 1024 = 81920, weight = 20,
    32 samples.  Colours J = (0.25, 0.5, -1) near and (1.5, 3, 1.5) far, Jq = J x 2^20:
      acc_0 = 65536 x 262144 + 16384 x 1572864 = 42949672960 = 81920 x 524288        -> J_blend_0 = 524288 x 2^-20 = 0.5
      acc_1 = 65536 x 524288 + 16384 x 3145728 = 85899345920 = 81920 x 1048576       -> 1.0
      acc_2 = -65536 x 1048576 + 16384 x 1572864 = -42949672960                      -> -0.5
    raw (10, 20, 250) near and (63, 25, 0) far: racc = 16384 x (4 near + far) = 16384 x (103, 105, 1000), and
    (2 racc + wsum) / (2 wsum) = (2 x (103, 105, 1000) + 5) / 10 = (21, 21, 200) in integers (20.6 rounds up, 21.0 and 200.0 stay)."""
    near, J_near = plane_view(1.0, [0.25, 0.5, -1.0], [10, 20, 250])
    far, J_far = plane_view(1.5, [1.5, 3.0, 1.5], [63, 25, 0])
    for order in ((near, J_near, far, J_far), (far, J_far, near, J_near)):
        out = bref.blend([order[0], order[2]], [order[1], order[3]], torch.eye(3), 1.0, 1.0)
        assert (out['base']['Hm'], out['base']['Wm']) == (1, 1)
        assert out['base']['range'].tolist() == [[1.0]] and int(out['base']['ties'][0, 0]) == 16
        assert sorted(out['wq'].tolist()) == [1024] * 16 + [4096] * 16
        assert out['acc'].shape == (1, _lib.MOSAIC_ACC_WORDS)     # laid out as the library's accumulator
        assert out['acc'].tolist() == [[42949672960, 85899345920, -42949672960, 16384 * 103, 16384 * 105, 16384 * 1000, 81920, 32]]
        assert out['J_blend'].tolist() == [[[0.5, 1.0, -0.5]]]
        assert out['raw_blend'].tolist() == [[[21, 21, 200]]]
        assert out['weight'].tolist() == [[20.0]] and out['samples'].tolist() == [[32]]
        assert out['J_blend'].dtype == torch.float32 and out['raw_blend'].dtype == torch.uint8 and out['samples'].dtype == torch.int32
    # H = 0.25: the far view lies beyond the blend depth (t = max(1 - 2, 0) = 0), contributes nothing and is not counted
    out = bref.blend([near, far], [J_near, J_far], torch.eye(3), 1.0, 0.25)
    assert out['acc'].tolist() == [[65536 * 262144, 65536 * 524288, -65536 * 1048576, 65536 * 10, 65536 * 20, 65536 * 250, 65536, 16]]
    assert out['J_blend'].tolist() == [[[0.25, 0.5, -1.0]]] and out['raw_blend'].tolist() == [[[10, 20, 250]]]
    assert out['weight'].tolist() == [[16.0]] and out['samples'].tolist() == [[16]]


def test_oracle_rounds_to_even_and_clamps():
    assert bref.weights(np.float32([1.0, 1.5, 3.0]), np.float32([1.0, 1.0, 1.0]), 1.0).tolist() == [4096, 1024, 0]
    # numpy's rint is the device's rintf: halves go to the even neighbour
    assert np.rint(np.float32([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0]
    inf = float('inf')
    assert bref.quantised(np.float32([inf, -inf, 1e6, -5000.0, 0.5, -0.25, 1024.0])).tolist() == \
        [1 << 30, -(1 << 30), 1 << 30, -(1 << 30), 1 << 19, -(1 << 18), 1 << 30]
    n = engine.MOSAIC_MAX_SAMPLES     # the bound: 2^20 samples in a cell are not summed up silently, one fewer are
    assert n == 1 << 20
    with pytest.raises(AssertionError):
        bref.normalise(np.array([[0, 0, 0, 0, 0, 0, 4096 * n, n]], np.int64), 1, 1)
    assert bref.normalise(np.array([[0, 0, 0, 0, 0, 0, 4096 * (n - 1), n - 1]], np.int64), 1, 1)['samples'].tolist() == [[n - 1]]


# ---- the flag and what it refuses -----------------------------------------------------------------------------------------------

def test_flag_lives_in_extras_and_leaves_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'mosaic_blend' not in vars(off)
    on = p.parse_args(BASE + ['--mosaic', 'results', '--mosaic-blend', '0.5'])
    assert on.mosaic_blend == 0.5
    assert vars(off) == {k: v for k, v in vars(on).items() if k not in ('mosaic', 'mosaic_blend')}
    assert vars(p.parse_args(BASE + ['--mosaic', 'results'])) == {k: v for k, v in vars(on).items() if k != 'mosaic_blend'}
    assert all(a.dest != 'mosaic_blend' for a in p._actions)
    assert '--mosaic-blend H' in p.format_help()


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


def test_mosaic_blend_needs_mosaic(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert '--mosaic-blend: only with --mosaic' in run_refused(['--mosaic-blend', '0.1'], tmp_path, monkeypatch)


@pytest.mark.parametrize('H', ['0', '-1', 'nan', 'inf', '9e-7', '1.1e6'])
def test_a_blend_depth_outside_the_range_is_refused_before_any_file_is_opened(H, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', H], tmp_path, monkeypatch)
    assert message.startswith('--mosaic-blend: H must be a finite depth within [1e-06, 1e+06] metres, not ')


REFUSED = [(['--shared-water'], '--shared-water'), (['--apply-water', 'w.pt'], '--apply-water'), (['--check-consistency', 'r'], '--check-consistency'),
           (['--common-stretch'], '--common-stretch'), (['--image-scale', '0.5'], '--image-scale'), (['--mosaic-gsd', '0'], '--mosaic-gsd')]


@pytest.mark.parametrize('extra, named', REFUSED, ids=[' '.join(e) for e, _ in REFUSED])
def test_what_mosaic_refuses_stays_refused_with_a_blend(extra, named, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', '0.5'] + extra, tmp_path, monkeypatch)
    assert '--mosaic' in message and named in message and '--mosaic-blend' not in message


def test_a_world_above_one_stays_refused_with_a_blend(tmp_path, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', '0.5'], tmp_path, monkeypatch)
    assert '--mosaic' in message and 'world size of 2' in message and 'all-reduce is not built' in message


def test_the_blend_depth_is_checked_by_the_functions_too(tmp_path, monkeypatch):
    for bad in (0.0, -1.0, float('nan'), float('inf'), 9e-7, 1.1e6, 'deep'):
        with pytest.raises(ValueError, match='blend depth H'):
            engine.mosaic_blend_depth(bad)
        with pytest.raises(ValueError, match='blend depth H'):
            engine.mosaic_of([SimpleNamespace()], [None], torch.eye(3), 0.1, blend=bad)   # before the device is looked at
    assert engine.mosaic_blend_depth(1e-6) == np.float32(1e-6) and engine.mosaic_blend_depth(1e6) == np.float32(1e6)
    assert isinstance(engine.mosaic_blend_depth(2), np.float32)
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda *a, **k: None)
    with pytest.raises(SystemExit) as e:
        sucre.mosaic([SimpleNamespace(name='a.png')], None, tmp_path / 'results', tmp_path / 'out', blend=0.0)
    assert str(e.value.code).startswith('--mosaic-blend: ') and not (tmp_path / 'out').exists()


# ---- the library: the entries exist and check their arguments before any launch -------------------------------------------------

def good_image():
    im = _lib.MosaicImage()
    im.depth, im.rgb, im.J, im.H, im.W = 256, 512, 1024, 8, 16
    return im


def good_grid():
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 0.5, 0.0, 0.0, 4, 4
    return g


def test_abi_has_the_blend_entries_and_keeps_its_version():
    assert 'sucre_mosaic_accumulate' in _lib.SIGNATURES and 'sucre_mosaic_normalize' in _lib.SIGNATURES
    assert _lib.load().sucre_version() == 2 == _lib.ABI_VERSION
    assert _lib.MOSAIC_ACC_WORDS == 8 == bref.ACC_WORDS
    header = (Path(__file__).resolve().parent.parent / 'include' / 'sucre_hip.h').read_text()
    assert '#define SUCRE_MOSAIC_ACC_WORDS 8' in header and '2^20' in header and '2^62' in header


def test_argument_validation_happens_before_any_launch():
    lib = _lib.load()
    ERR = -1   # SUCRE_ERR_ARG
    p = C.c_void_p(4096)
    one = (_lib.MosaicImage * 1)(good_image())
    grid = good_grid()
    g = C.byref(grid)

    def accumulate(table=p, n=1, images=one, first=0, grid=g, key=p, inv_h=1.0, acc=p, flags=0):
        return lib.sucre_mosaic_accumulate(table, n, images, first, grid, key, inv_h, acc, flags, None)

    assert accumulate(table=None) == ERR and b'table' in lib.sucre_last_error()
    assert accumulate(n=0) == ERR and accumulate(n=engine.MAX_VIEWS + 1) == ERR and b'n_images=4097' in lib.sucre_last_error()
    assert accumulate(images=None) == ERR and b'images is NULL' in lib.sucre_last_error()
    assert accumulate(first=engine.MAX_VIEWS) == ERR and b'ordinals' in lib.sucre_last_error()
    assert accumulate(first=-1) == ERR
    bad = good_image()
    bad.J = None
    assert accumulate(images=(_lib.MosaicImage * 1)(bad)) == ERR and b'NULL' in lib.sucre_last_error()
    assert accumulate(grid=None) == ERR and b'grid is NULL' in lib.sucre_last_error()
    for field, value, what in (('gsd', 0.0, b'gsd'), ('gsd', float('nan'), b'gsd'), ('lo_t', float('inf'), b'lo='), ('Hm', 0, b'cells'),
                               ('Wm', (1 << 24) + 1, b'cells')):
        worse = good_grid()
        setattr(worse, field, value)
        assert accumulate(grid=C.byref(worse)) == ERR and what in lib.sucre_last_error(), (field, value)
        assert lib.sucre_mosaic_normalize(C.byref(worse), p, p, p, p, p, None) == ERR and what in lib.sucre_last_error(), (field, value)
    assert accumulate(key=None) == ERR and b'key_dev' in lib.sucre_last_error()
    assert accumulate(key=C.c_void_p(4100)) == ERR
    for inv_h in (0.0, -1.0, float('nan'), float('inf')):
        assert accumulate(inv_h=inv_h) == ERR and b'inv_h' in lib.sucre_last_error(), inv_h
    assert accumulate(acc=None) == ERR and b'acc_dev' in lib.sucre_last_error()
    assert accumulate(acc=C.c_void_p(4100)) == ERR and b'acc_dev' in lib.sucre_last_error()
    assert accumulate(flags=2) == ERR and b'flags' in lib.sucre_last_error()
    assert lib.sucre_mosaic_normalize(None, p, p, p, p, p, None) == ERR and b'grid is NULL' in lib.sucre_last_error()
    assert lib.sucre_mosaic_normalize(g, None, p, p, p, p, None) == ERR and b'acc_dev' in lib.sucre_last_error()
    for k in range(4):
        outs = [None if i == k else p for i in range(4)]
        assert lib.sucre_mosaic_normalize(g, p, *outs, None) == ERR and b'samples_out is NULL' in lib.sucre_last_error(), k
    assert lib.sucre_mosaic_normalize(g, p, C.c_void_p(4098), p, p, p, None) == ERR and b'aligned' in lib.sucre_last_error()
    huge = good_grid()
    huge.Hm = huge.Wm = 1 << 20
    assert lib.sucre_mosaic_normalize(C.byref(huge), p, p, p, p, p, None) == ERR and b'2^39' in lib.sucre_last_error()
