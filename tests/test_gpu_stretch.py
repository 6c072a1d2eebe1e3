"""GPU tests of the common colour stretch: the pooled radix select (sucre_pool_select_*, engine.PoolSelect,
engine.pooled_percentiles), sucre.common_stretch, and --common-stretch / --stretch-from on the command line.

Every comparison is exact -- integer equality on pictures, == on float32 values (-0.0 == 0.0 counts as equal: np.sort does not
order the two zeros, the key order does).  The yardstick is numpy on the CPU, written out here:
    P_c(q) = float32(np.percentile(pool_c.astype(float64), q))         over the valid pixels of all images together
    picture = uint8(((min(max(J, lo), hi) - lo) / (hi - lo)) * 255)     in float32, invalid pixels 0
"""
import contextlib
import ctypes as C
import io
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

from sucre_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def valid_pixels(Js):
    rows = [np.asarray(J, np.float32).reshape(-1, 3) for J in Js]
    return np.concatenate([r[~np.isnan(r).any(axis=1)] for r in rows])


def numpy_percentiles(Js, q):
    pool = valid_pixels(Js)
    P = np.stack([np.percentile(pool[:, c].astype(np.float64), q).astype(np.float32) for c in range(3)])
    return P, len(pool)


def formula_picture(J, lo, hi):
    J = np.asarray(J, np.float32)
    ok = ~np.isnan(J).any(axis=2)
    out = np.zeros(J.shape, np.uint8)
    for c in range(3):
        x = np.minimum(np.maximum(J[..., c][ok], np.float32(lo[c])), np.float32(hi[c]))
        out[..., c][ok] = np.uint8(((x - np.float32(lo[c])) / (np.float32(hi[c]) - np.float32(lo[c]))) * np.float32(255))
    return out


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and bool(np.all(a == b))


def on_device(Js):
    return [torch.from_numpy(J).to(DEV) for J in Js]


# ---- the mixed pool -----------------------------------------------------------------------------------------------------------
_POOL = {}


def mixed_pool():
    """Host images, made once and never changed: 5x3 (less than one lane group), 47x33 (n_px % 4 != 0), 75x52, 640x480 (the
    lanes' loops wrap), one all NaN, one without rows.  Values: negatives, exact zeros of both signs, eight binades; in channel 0
    eighty per cent of the large image differ only in the lowest mantissa byte, in channel 1 only in the second lowest, so the
    25th and 75th percentile are decided by passes 3 and 2; NaN in ONE channel of some pixels."""
    if not _POOL:
        def img(h, w, seed):
            r = np.random.default_rng(seed)
            return (r.standard_normal((h, w, 3)) * np.float32(2.0) ** r.integers(-5, 3, (h, w, 3))).astype(np.float32)
        a, b, c, big = img(5, 3, 1), img(47, 33, 2), img(75, 52, 3), img(480, 640, 4)
        b[0:3, 0:5] = 0.0
        b[3, 0:5, 1] = -0.0
        r = np.random.default_rng(9)
        cluster = r.random((480, 640)) < 0.8
        n = int(cluster.sum())
        base = int(np.float32(0.05).view(np.uint32)) & 0xffff0000
        big[..., 0][cluster] = (np.uint32(base | 0x5a00) | r.integers(0, 256, n).astype(np.uint32)).view(np.float32)
        big[..., 1][cluster] = (np.uint32(base | 0x0033) | (r.integers(0, 256, n).astype(np.uint32) << 8)).view(np.float32)
        a[1, 1, 0] = np.nan
        b[5, 5, 2] = np.nan
        c[1, 1, 1] = np.nan
        c[40:44, 9, 2] = np.nan
        big[100:120, 7, 0] = np.nan
        big[300, 11:400, 1] = np.nan
        big[479, 639] = np.nan
        nan_image = np.full((6, 7, 3), np.nan, np.float32)
        no_rows = np.zeros((0, 9, 3), np.float32)
        host = [a, nan_image, b, no_rows, c, big]
        _POOL['host'] = host
        _POOL['dev'] = on_device(host)
        _POOL['want'] = {q: numpy_percentiles(host, list(q)) for q in ((1.0, 99.0), (0.0, 25.0, 75.0, 100.0))}
        # what the construction is for, shown on the yardstick alone: the quartiles of channels 0 and 1 lie inside the clusters
        P = _POOL['want'][(0.0, 25.0, 75.0, 100.0)][0]
        for c_, keep in ((0, 0xffffff00), (1, 0xffff00ff)):
            bits = P[c_, 1:3].view(np.uint32)
            assert bits[0] != bits[1] and (bits[0] & keep) == (bits[1] & keep), (c_, [hex(x) for x in bits])
        pool = valid_pixels(host)
        assert (pool < 0).any() and (pool == 0).any() and len(pool) > 256 * 1024
    return _POOL


@pytest.mark.parametrize('q', [(1.0, 99.0), (0.0, 25.0, 75.0, 100.0)], ids=['q1-99', 'q0-25-75-100'])
def test_mixed_pool_equals_numpy(q):
    pool = mixed_pool()
    want, n_want = pool['want'][q]
    P, n = engine.pooled_percentiles(pool['dev'], q=q)
    print(f'n = {n} (numpy {n_want})\nP =\n{P}\nnumpy =\n{want}')
    assert isinstance(n, int) and n == n_want
    assert P.shape == (3, len(q)) and same(P, want)


def test_ties():
    """Ninety per cent of channel G are one number: every rank of its quartiles falls into the tie."""
    from sucre_amd import sucre
    r = np.random.default_rng(17)
    J = (r.random((64, 50, 3)) * 1.5).astype(np.float32)
    tie = r.random((64, 50)) < 0.9
    J[..., 1][tie] = np.float32(0.4321)
    J[7, 7, 0] = np.nan
    want, n_want = numpy_percentiles([J], [25.0, 75.0])
    assert want[1, 0] == want[1, 1] == np.float32(0.4321) and want[0, 0] < want[0, 1]
    dev = on_device([J])
    P, n = engine.pooled_percentiles(dev, q=(25.0, 75.0))
    assert n == n_want == 64 * 50 - 1 and same(P, want)
    P199, _ = engine.pooled_percentiles(dev, q=(1.0, 99.0))
    assert same(P199, numpy_percentiles([J], [1.0, 99.0])[0])
    with pytest.raises(ValueError, match='channel G'):
        sucre.common_stretch(dev, q=(25, 75))
    lo, hi, n = sucre.common_stretch(dev)   # the 1st and 99th percentile lie outside the tie: a stretch
    assert same(lo, P199[:, 0]) and same(hi, P199[:, 1]) and n == n_want


def test_empty_pool_is_an_error():
    from sucre_amd import sucre
    dev = on_device([np.full((6, 7, 3), np.nan, np.float32), np.zeros((0, 9, 3), np.float32)])
    with pytest.raises(ValueError, match='no valid pixel'):
        engine.pooled_percentiles(dev)
    with pytest.raises(ValueError, match='no valid pixel'):
        sucre.common_stretch(dev)


@pytest.mark.parametrize('index, cuts', [(4, (0, 20, 21, 75)), (2, (0, 10, 31, 47))], ids=['75x52', '47x33-misaligned-blocks'])
def test_pool_of_one_image_equals_the_pool_of_its_row_blocks(index, cuts):
    """(the row blocks of the 47x33 image do not start on 16 bytes: the engine pools copies of them)"""
    J = mixed_pool()['dev'][index]
    q = (0.0, 1.0, 50.0, 99.0)
    whole, n = engine.pooled_percentiles([J], q=q)
    blocks = [J[a:b] for a, b in zip(cuts, cuts[1:])]
    assert all(b.is_contiguous() for b in blocks)
    parts, n_parts = engine.pooled_percentiles(blocks, q=q)
    assert n == n_parts and same(whole, parts)
    assert same(whole, numpy_percentiles([J.cpu().numpy()], list(q))[0])


def run_select(lists, q, n_ranks=None):
    """The phases driven by hand over len(lists) emulated ranks: every state adds its own images, the histograms are summed on
    the host of the test and written into every state, all locate.  Returns every state's values and the pooled count."""
    from sucre_amd.sucre import percentile_plan64
    states = [engine.PoolSelect(DEV) for _ in lists]
    for s in states:
        s.begin()
    n = None
    for p in range(4):
        for s, Js in zip(states, lists):
            if isinstance(Js, tuple):   # one add per image
                for J in Js:
                    s.add([J], p, n_ranks=2 * len(q))
            else:
                s.add(Js, p, n_ranks=2 * len(q))
        total = sum(s.hist.clone() for s in states)
        assert total.dtype == torch.int64 and total.shape == (3, 8, 256)
        for s in states:
            s.hist.copy_(total)
        if p == 0:
            n = int(total[0, 0].sum())
            assert n == int(total[1, 0].sum()) == int(total[2, 0].sum()) and not bool(total[:, 1:].any())
            plans = [percentile_plan64(n, x) for x in q]
            for s in states:
                s.locate(0, [r for below, above, _ in plans for r in (below, above)])
        else:
            for s in states:
                s.locate(p)
        assert all(not bool(s.hist.any()) for s in states), 'locate zeroes the histograms'
    return [s.values().cpu().numpy() for s in states], n


def test_split_phases_are_ranks():
    pool = mixed_pool()
    q = (1.0, 99.0)
    (single,), n1 = run_select([pool['dev']], q)
    halves, n2 = run_select([pool['dev'][0::2], pool['dev'][1::2], []], q)   # the third rank holds no image
    assert n1 == n2 == pool['want'][q][1]
    for v in halves:
        assert same(v, single)
    # the order statistics themselves, against numpy's sort
    host = valid_pixels(pool['host'])
    from sucre_amd.sucre import percentile_plan64
    ranks = [r for x in q for r in percentile_plan64(n1, x)[:2]]
    assert same(single, np.stack([np.sort(host[:, c])[ranks] for c in range(3)]))


def test_chunked_add():
    pool = mixed_pool()
    q = (0.0, 25.0, 75.0, 100.0)
    (together,), n1 = run_select([pool['dev']], q)
    (one_by_one,), n2 = run_select([tuple(pool['dev'])], q)
    assert n1 == n2 and same(together, one_by_one)


def test_abi_argument_checks():
    lib = _lib.load()
    state = torch.zeros(lib.sucre_pool_select_bytes() // 8 + 1, dtype=torch.int64, device=DEV)
    J = torch.zeros((4, 4, 3), dtype=torch.float32, device=DEV)
    table = torch.zeros(lib.sucre_pool_table_bytes(1), dtype=torch.uint8, device=DEV)
    sp, tp = C.c_void_p(state.data_ptr()), C.c_void_p(table.data_ptr())
    arr = (_lib.PoolImage * 1)()
    arr[0].J, arr[0].n_px = J.data_ptr(), 16
    assert lib.sucre_pool_select_bytes() >= 8 * _lib.POOL_HIST_WORDS and lib.sucre_pool_select_bytes() % 8 == 0
    assert lib.sucre_pool_table_bytes(-1) == 0 and lib.sucre_pool_table_bytes(4097) == 0 and lib.sucre_pool_table_bytes(0) > 0
    with torch.cuda.device(DEV):
        assert lib.sucre_pool_select_begin(sp, engine._stream_ptr()) == 0
        assert lib.sucre_pool_select_pass(sp, 4, tp, 1, arr, 4, None) == -1 and b'pass' in lib.sucre_last_error()
        assert lib.sucre_pool_select_pass(sp, -1, tp, 1, arr, 4, None) == -1
        assert lib.sucre_pool_select_pass(sp, 0, tp, 1, arr, 9, None) == -1 and b'n_ranks' in lib.sucre_last_error()
        assert lib.sucre_pool_select_pass(sp, 0, tp, 1, arr, 0, None) == -1
        assert lib.sucre_pool_select_pass(sp, 0, tp, -1, arr, 4, None) == -1 and b'n_images' in lib.sucre_last_error()
        assert lib.sucre_pool_select_pass(sp, 0, tp, 4097, arr, 4, None) == -1
        assert lib.sucre_pool_select_pass(None, 0, tp, 1, arr, 4, None) == -1
        assert lib.sucre_pool_select_pass(sp, 0, None, 1, arr, 4, None) == -1 and b'table' in lib.sucre_last_error()
        assert lib.sucre_pool_select_pass(sp, 0, tp, 1, None, 4, None) == -1
        arr[0].J = J.data_ptr() + 4
        assert lib.sucre_pool_select_pass(sp, 0, tp, 1, arr, 4, None) == -1 and b'16-byte' in lib.sucre_last_error()
        arr[0].J, arr[0].n_px = J.data_ptr(), -1
        assert lib.sucre_pool_select_pass(sp, 0, tp, 1, arr, 4, None) == -1 and b'negative' in lib.sucre_last_error()
        ranks = (C.c_uint64 * 4)(0, 1, 2, 3)
        assert lib.sucre_pool_select_locate(sp, 4, 4, ranks, None, None) == -1
        assert lib.sucre_pool_select_locate(sp, 0, 9, ranks, None, None) == -1
        assert lib.sucre_pool_select_locate(sp, 0, 4, None, None, None) == -1 and b'ranks' in lib.sucre_last_error()
        assert lib.sucre_pool_select_locate(sp, 3, 4, None, None, None) == -1 and b'out_dev' in lib.sucre_last_error()
        torch.cuda.synchronize()
    assert not bool(state.any()), 'nothing was launched: the state is as begin left it'


# ---- the command line ---------------------------------------------------------------------------------------------------------
def _base(root):
    return ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model')]


def _merge(root_a, root_b, root):
    """One COLMAP text model of two single-camera ones: camera 2 and the image ids behind A's for B."""
    for sub in ('images', 'depth'):
        shutil.copytree(root_a / sub, root / sub)
        for f in (root_b / sub).iterdir():
            shutil.copy(f, root / sub / f.name)
    data = lambda p: [l for l in p.read_text().splitlines() if l.strip() and not l.startswith('#')]   # noqa: E731
    cam_b = data(root_b / 'model' / 'cameras.txt')[0].split()
    cam_b[0] = '2'
    (root / 'model').mkdir()
    (root / 'model' / 'cameras.txt').write_text('\n'.join(data(root_a / 'model' / 'cameras.txt') + [' '.join(cam_b)]) + '\n')
    lines = data(root_a / 'model' / 'images.txt')
    n_a = len(lines)
    for l in data(root_b / 'model' / 'images.txt'):
        tok = l.split()
        tok[0], tok[8] = str(int(tok[0]) + n_a), '2'
        lines.append(' '.join(tok))
    (root / 'model' / 'images.txt').write_text('# Image list with two lines of data per image:\n' + ''.join(l + '\n\n' for l in lines))
    (root / 'model' / 'points3D.txt').write_text('# 3D point list (empty)\n')


def _main(argv):
    from sucre_amd import sucre
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        sucre.main(argv)
    return buf.getvalue()


@pytest.fixture(scope='module')
def survey(tmp_path_factory):
    """A 48x32 survey of five images (root), the same plus three 47x33 images under a second camera (mixed), and the two
    --shared-water runs over images 1..3 that the tests below read: with --common-stretch and without."""
    import copy
    from test_gpu_api import write_scene
    top = tmp_path_factory.mktemp('stretch')
    root, other, mixed = top / 'a', top / 'b', top / 'mixed'
    scene = synth.make_scene(48, 32, 4, seed=3)
    write_scene(scene, root)
    small = synth.make_scene(47, 33, 2, seed=5)
    small.views = [copy.copy(v) for v in small.views]
    for v in small.views:
        v.name = 'b_' + v.name
    write_scene(small, other)
    mixed.mkdir()
    _merge(root, other, mixed)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv('WORLD_SIZE', raising=False)
        shared = ['--image-ids', '1', '4', '--num-iter', '5', '--shared-water']
        printed = _main(_base(root) + ['--output-dir', str(top / 'common')] + shared + ['--common-stretch'])
        _main(_base(root) + ['--output-dir', str(top / 'plain')] + shared)
    return dict(top=top, root=root, mixed=mixed, scene=scene, small=small, printed=printed)


def _png(path):
    from PIL import Image as PILImage
    return np.asarray(PILImage.open(path))


def _check_common(out, names, printed):
    """stretch.pt of ``out`` against the numpy pool of the J in the <name>.pt files, and every _rgb.png against the formula."""
    st = torch.load(out / 'stretch.pt')
    assert list(st) == ['lo', 'hi', 'q', 'n_valid', 'images']
    assert st['lo'].dtype == st['hi'].dtype == torch.float32 and st['lo'].shape == st['hi'].shape == (3,)
    assert st['q'].tolist() == [1.0, 99.0] and st['images'] == names
    Js = [torch.load(out / f'{Path(n).stem}.pt')['J'].numpy() for n in names]
    want, n_valid = numpy_percentiles(Js, [1.0, 99.0])
    lo, hi = st['lo'].numpy(), st['hi'].numpy()
    assert st['n_valid'] == n_valid and same(lo, want[:, 0]) and same(hi, want[:, 1])
    for n, J in zip(names, Js):
        assert np.array_equal(_png(out / f'{Path(n).stem}_rgb.png'), formula_picture(J, lo, hi)), n
    line = [l for l in printed.splitlines() if l.startswith('common stretch over')]
    assert len(line) == 1 and line[0].startswith(f'common stretch over {len(names)} images, {n_valid} valid pixels: R lo ')
    assert ', G lo ' in line[0] and ', B lo ' in line[0] and ' hi ' in line[0]
    return lo, hi, Js


def test_cli_shared_water_common_stretch(survey):
    names = survey['scene'].names[0:3]
    common, plain = survey['top'] / 'common', survey['top'] / 'plain'
    lo, hi, Js = _check_common(common, names, survey['printed'])
    assert sorted(p.name for p in common.iterdir()) == sorted([p.name for p in plain.iterdir()] + ['stretch.pt'])
    differ = 0
    for n in names:
        stem = Path(n).stem
        for f in (f'{stem}_reconstruction.png', f'{stem}.pt'):
            assert (common / f).read_bytes() == (plain / f).read_bytes(), f
        differ += not np.array_equal(_png(common / f'{stem}_rgb.png'), _png(plain / f'{stem}_rgb.png'))
    assert (common / 'shared_water.pt').read_bytes() == (plain / 'shared_water.pt').read_bytes()
    assert differ, 'the per-image pictures are another stretch'


def test_cli_apply_water_stretch_from(survey, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    common = survey['top'] / 'common'
    out = tmp_path / 'applied'
    _main(_base(survey['root']) + ['--output-dir', str(out), '--apply-water', str(common / 'shared_water.pt'), '--stretch-from',
                                   str(common / 'stretch.pt'), '--image-ids', '4', '6'])
    names = survey['scene'].names[3:5]
    st = torch.load(common / 'stretch.pt')
    assert sorted(p.name for p in out.iterdir()) == sorted([f'{Path(n).stem}_rgb.png' for n in names] + [f'{Path(n).stem}.pt' for n in names])
    for n in names:
        J = torch.load(out / f'{Path(n).stem}.pt')['J'].numpy()
        assert np.array_equal(_png(out / f'{Path(n).stem}_rgb.png'), formula_picture(J, st['lo'].numpy(), st['hi'].numpy())), n


def test_cli_apply_water_common_stretch_two_sizes(survey, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    names = [survey['scene'].names[4], survey['small'].names[0], survey['scene'].names[0], survey['small'].names[2]]
    (tmp_path / 'list.txt').write_text('\n'.join(names) + '\n')
    water = str(survey['top'] / 'common' / 'shared_water.pt')
    first, second = tmp_path / 'first', tmp_path / 'second'
    args = _base(survey['mixed']) + ['--apply-water', water, '--image-list', str(tmp_path / 'list.txt')]
    printed = _main(args + ['--output-dir', str(first), '--common-stretch'])
    lo, hi, Js = _check_common(first, names, printed)
    assert {J.shape for J in Js} == {(32, 48, 3), (33, 47, 3)}
    _main(args + ['--output-dir', str(second), '--stretch-from', str(first / 'stretch.pt')])
    assert not (second / 'stretch.pt').exists()
    for n in names:
        stem = Path(n).stem
        assert (first / f'{stem}_rgb.png').read_bytes() == (second / f'{stem}_rgb.png').read_bytes(), n
        assert (first / f'{stem}.pt').read_bytes() == (second / f'{stem}.pt').read_bytes(), n


def test_cli_plain_run_with_and_without_stretch_from(survey, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    name = survey['scene'].names[survey['scene'].target]
    stem = Path(name).stem
    st = torch.load(survey['top'] / 'common' / 'stretch.pt')
    run = _base(survey['root']) + ['--image-name', name, '--num-iter', '5']
    fixed, own = tmp_path / 'fixed', tmp_path / 'own'
    _main(run + ['--output-dir', str(fixed), '--stretch-from', str(survey['top'] / 'common' / 'stretch.pt')])
    _main(run + ['--output-dir', str(own)])
    assert (fixed / f'{stem}.pt').read_bytes() == (own / f'{stem}.pt').read_bytes()
    assert (fixed / f'{stem}_reconstruction.png').read_bytes() == (own / f'{stem}_reconstruction.png').read_bytes()
    J = torch.load(own / f'{stem}.pt')['J'].numpy()
    assert np.array_equal(_png(fixed / f'{stem}_rgb.png'), formula_picture(J, st['lo'].numpy(), st['hi'].numpy()))
    # without the flag: the reference's plot_J (sucre.py:84-94), restated
    ref = J.copy()
    valid = np.all(~np.isnan(ref), axis=2)
    vals = ref[valid]
    vals = np.clip(vals, np.percentile(vals, 1, axis=0), np.percentile(vals, 99, axis=0))
    vals -= vals.min(axis=0)
    vals /= vals.max(axis=0)
    ref[~valid] = 0
    ref[valid] = vals
    assert np.array_equal(_png(own / f'{stem}_rgb.png'), np.uint8(ref * 255))


def test_cli_common_stretch_refused_when_the_images_do_not_fit(survey, tmp_path, monkeypatch):
    from sucre_amd import loader, sucre
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sucre, '_free_device_memory', lambda device: 2 * 32 * 48 * 12)   # 0.8 of it holds less than two images
    decoded = []
    for fn in ('_imread_rgb_u8', '_imread_depth_u16'):
        real = getattr(loader, fn)
        monkeypatch.setattr(loader, fn, lambda path, real=real: (decoded.append(Path(path).name), real(path))[1])
    with pytest.raises(SystemExit) as e:
        sucre.main(_base(survey['root']) + ['--output-dir', str(tmp_path / 'out'), '--apply-water', str(survey['top'] / 'common' / 'shared_water.pt'),
                                            '--common-stretch', '--image-ids', '1', '3'])
    assert '--stretch-from' in str(e.value.code) and '--common-stretch' in str(e.value.code)
    assert not decoded and not (tmp_path / 'out' / 'stretch.pt').exists()


def test_cli_apply_water_common_stretch_two_ranks_equal_one_process(survey, tmp_path, monkeypatch):
    """The pool spans the ranks: three images of two sizes under WORLD_SIZE=2 (two and one; gloo on the box's one GPU) give the
    files of the one-process run byte for byte -- the histograms are integers, their all-reduce is the in-process sum."""
    import os
    import socket
    import subprocess
    import sys
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    root = Path(__file__).resolve().parent.parent
    names = [survey['small'].names[1], survey['scene'].names[2], survey['scene'].names[3]]
    (tmp_path / 'list.txt').write_text('\n'.join(names) + '\n')
    args = _base(survey['mixed']) + ['--apply-water', str(survey['top'] / 'common' / 'shared_water.pt'), '--image-list',
                                     str(tmp_path / 'list.txt'), '--common-stretch']
    printed = _main(args + ['--output-dir', str(tmp_path / 'one')])
    _check_common(tmp_path / 'one', names, printed)
    clean = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    clean['PYTHONPATH'] = str(root) + os.pathsep + clean.get('PYTHONPATH', '')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'sucre_amd.sucre'] + args + ['--output-dir', str(tmp_path / 'two')]
    procs = [subprocess.Popen(cmd, env=dict(clean, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                                            MASTER_PORT=str(port), SUCRE_DIST_BACKEND='gloo'),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=root) for k in range(2)]
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    assert sum('common stretch over 3 images' in so for so, _ in outs) == 1, 'rank 0 alone reports'
    files = sorted(f.name for f in (tmp_path / 'one').iterdir())
    assert files == sorted(f.name for f in (tmp_path / 'two').iterdir()) and 'stretch.pt' in files
    for f in files:
        assert (tmp_path / 'one' / f).read_bytes() == (tmp_path / 'two' / f).read_bytes(), f
