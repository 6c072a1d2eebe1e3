"""Host tests of the multi-band mosaic blend (csrc/bands.h): the band stack of tests/mosaic_bands_ref.py against plain per-pixel
loops over the definition; what a constant image and the sum of a stack give; ``engine.mosaic_band_plan`` and
``engine.mosaic_band_count``; what --mosaic-bands refuses before any file is opened; that the options record is what it was; and
the frequency property on the crafted pair, by the restatement alone.  No GPU."""
import builtins
import dataclasses
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_bands_ref as mref
import mosaic_blend_ref as bref
from sucre_amd import engine, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']
NAN = np.float32(np.nan)


def stack_by_loops(depth, J, K):
    """The definition, pixel by pixel and tap by tap: Python loops over numpy float32 scalars, one IEEE operation per statement."""
    H, W = depth.shape
    two, zero = np.float32(2), np.float32(0)
    member = [[bool(depth[v, u] > 0) and not any(np.isnan(J[v, u, c]) for c in range(3)) for u in range(W)] for v in range(H)]
    S = np.full((H, W, 3), NAN, np.float32)
    for v in range(H):
        for u in range(W):
            if member[v][u]:
                for c in range(3):
                    S[v, u, c] = min(max(J[v, u, c], np.float32(-1024)), np.float32(1024))

    def a(u, v, c):
        return S[v, u, c] if 0 <= u < W and 0 <= v < H and member[v][u] else zero

    def m(u, v):
        return 1 if 0 <= u < W and 0 <= v < H and member[v][u] else 0

    out = []
    for j in range(K):
        s = 1 << j
        nxt = np.full((H, W, 3), NAN, np.float32)
        D = np.full((H, W, 3), NAN, np.float32)
        for v in range(H):
            for u in range(W):
                if not member[v][u]:
                    continue
                Ah = [(m(u - s, vv) + 2 * m(u, vv)) + m(u + s, vv) for vv in (v - s, v, v + s)]
                A = (Ah[0] + 2 * Ah[1]) + Ah[2]
                assert 4 <= A <= 16
                for c in range(3):
                    Nh = []
                    for vv in (v - s, v, v + s):
                        t = two * a(u, vv, c)
                        l = a(u - s, vv, c) + t
                        Nh.append(l + a(u + s, vv, c))
                    t = two * Nh[1]
                    l = Nh[0] + t
                    N = l + Nh[2]
                    nxt[v, u, c] = N / np.float32(A)
                    D[v, u, c] = S[v, u, c] - nxt[v, u, c]
        out.append(D)
        S = nxt
    return out + [S]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_image(H, W, seed, holes):
    rng = np.random.default_rng(seed)
    depth = (rng.random((H, W)) + 0.5).astype(np.float32)
    J = (rng.random((H, W, 3)) * 4 - 1).astype(np.float32)
    depth[rng.random((H, W)) < holes] = 0
    J[rng.random((H, W, 3)) < holes / 3] = NAN
    if H * W > 3:
        J[0, 0] = (np.inf, -np.inf, 5000.0)
        J[-1, -1] = (-0.0, -2000.0, 0.0)
    return depth, J


@pytest.mark.parametrize('K', [1, 2, 3, 4, 5, 6])
def test_the_stack_equals_plain_loops_over_the_definition(K):
    for i, (H, W, holes) in enumerate([(1, 1, 0.0), (1, 7, 0.2), (5, 1, 0.2), (9, 11, 0.3), (9, 11, 0.0), (7, 10, 0.7), (4, 6, 1.0)]):
        depth, J = random_image(H, W, 100 * K + i, holes)
        got, want = mref.stack(depth, J, K), stack_by_loops(depth, J, K)
        assert len(got) == K + 1 == len(want)
        for j, (x, y) in enumerate(zip(got, want)):
            assert same_bits(x, y), (H, W, holes, j)


def test_a_constant_image_has_no_detail():
    depth = np.ones((9, 11), np.float32)
    depth[2:4, 3:9] = 0
    depth[7, 0] = -1
    J = np.full((9, 11, 3), 0.5, np.float32)
    J[5, 5, 1] = NAN
    for K in (1, 4, 6):
        *D, S = mref.stack(depth, J, K)
        member = mref.fref.members(depth, J)
        assert 0 < member.sum() < member.size
        for band in D:
            assert bool((band[member] == 0).all()) and bool(np.isnan(band[~member]).all())
        assert bool((S[member] == np.float32(0.5)).all()) and bool(np.isnan(S[~member]).all())


@pytest.mark.parametrize('K', [1, 4, 6])
def test_the_stack_adds_up_to_the_clamped_image(K):
    """S_K + sum of D_j, added in float32 from the coarse end, returns S_0 up to rounding.  With M = max |S_0| every |S_j| <= M (an
    average) and |D_j| <= 2 M; with u = 2^-24 each of the K subtractions errs by at most 2 M u and each of the K additions by at
    most u times a partial sum of at most M (1 + 3 K u): 3 K M u in all to first order, 4 K M u allowed."""
    depth, J = random_image(9, 11, 5, 0.2)
    stack = mref.stack(depth, J, K)
    member = mref.fref.members(depth, J)
    S0 = mref.clamped(J)[member]
    total = stack[-1][member]
    for D in stack[-2::-1]:
        total = total + D[member]
    assert total.dtype == np.float32
    M = float(np.abs(S0).max())
    assert M == 1024.0
    err = float(np.abs(total.astype(np.float64) - S0.astype(np.float64)).max())
    print(f'K = {K}: largest |S_K + sum D_j - S_0| = {err:.3g}, bound {4 * K * M * 2.0 ** -24:.3g}')
    assert err <= 4 * K * M * 2.0 ** -24


def test_the_plan_halves_depth_and_feather_with_every_finer_band():
    f32 = np.float32
    assert engine.mosaic_band_plan(0.5, 8, 4) == [(f32(0.03125), 1), (f32(0.0625), 1), (f32(0.125), 2), (f32(0.25), 4), (f32(0.5), 8)]
    assert engine.mosaic_band_plan(0.5, None, 1) == [(f32(0.25), None), (f32(0.5), None)]
    assert engine.mosaic_band_plan(2.0, 1024, 6) == [(f32(2.0 ** (1 + j - 6)), 1024 >> (6 - j)) for j in range(6)] + [(f32(2.0), 1024)]
    assert engine.mosaic_band_plan(3e-6, 5, 3) == [(f32(1e-6), 1), (f32(1e-6), 1), (f32(3e-6) * f32(0.5), 2), (f32(3e-6), 5)]     # both floors
    assert engine.mosaic_band_plan(1e-6, 1, 2) == [(f32(1e-6), 1)] * 3
    for H, F, K in ((0.5, 8, 4), (0.3, None, 6), (1e-6, 3, 2), (1e6, 1024, 6), (0.7, 100, 5)):
        got, want = engine.mosaic_band_plan(H, F, K), mref.plan(H, F, K)
        assert got == want and len(got) == K + 1
        for (h, f), (hw, fw) in zip(got, want):
            assert type(h) is np.float32 and h.tobytes() == hw.tobytes() and (f is None or type(f) is int)
            inv = np.float32(1) / h
            assert np.isfinite(inv) and inv > 0      # what the accumulate entry takes
        assert got[-1] == (np.float32(H), F)
        assert all(a[0] <= b[0] and (F is None or a[1] <= b[1]) for a, b in zip(got, got[1:]))
    for bad in ((0.0, 8, 4), (0.5, 0, 4), (0.5, 8, 0), (0.5, 8, 7), (0.5, 2.5, 4)):
        with pytest.raises(ValueError):
            engine.mosaic_band_plan(*bad)


def test_mosaic_band_count_takes_integral_numbers_in_range():
    assert engine.MOSAIC_BANDS_RANGE == (1, 6)
    for good, K in ((1, 1), (6, 6), (4.0, 4), ('3', 3), (np.int64(2), 2), (np.float32(5), 5)):
        got = engine.mosaic_band_count(good)
        assert got == K and type(got) is int
    for bad in (0, 7, -1, 2.5, float('nan'), float('inf'), 'many', None, True, False, 1e9):
        with pytest.raises(ValueError) as e:
            engine.mosaic_band_count(bad)
        assert str(e.value) == f'mosaic band count K must be an integer within [1, 6] bands, not {bad}' and e.value.field == 'bands'


def test_the_functions_refuse_bands_without_a_blend_and_a_bad_count(tmp_path, monkeypatch):
    for bad in (0, 7, 2.5, float('nan'), True):
        with pytest.raises(ValueError, match='band count K'):
            engine.mosaic_of([SimpleNamespace()], [None], torch.eye(3), 0.1, blend=0.5, bands=bad)   # before the device is looked at
    with pytest.raises(ValueError) as e:
        engine.mosaic_of([SimpleNamespace()], [None], torch.eye(3), 0.1, bands=4)
    assert str(e.value) == 'mosaic_of: the bands are blended with the blend\'s weights; give the blend depth too (blend=H)' and e.value.field == 'bands'
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda *a, **k: None)
    for kwargs, text in (({'bands': 4}, '--mosaic-bands: only with --mosaic-blend H'),
                         ({'bands': 0, 'blend': 0.5}, '--mosaic-bands: mosaic band count K must be an integer within [1, 6] bands, not 0')):
        with pytest.raises(SystemExit) as e:
            sucre.mosaic([SimpleNamespace(name='a.png')], None, tmp_path / 'results', tmp_path / 'out', **kwargs)
        assert str(e.value.code) == text and not (tmp_path / 'out').exists()


def test_the_options_record_and_its_table_hold_the_bands():
    assert [f.name for f in dataclasses.fields(engine.MosaicOptions)][:4] == ['blend', 'feather', 'fill', 'bands']
    assert list(engine.MOSAIC_VALUES)[:4] == ['blend', 'fill', 'feather', 'bands']
    assert engine.MOSAIC_VALUES['feather'] == ('feather width F', (1, 1024), True, 'source pixels', int, 'F', 'an integer')
    assert engine.MOSAIC_VALUES['bands'] == ('band count K', (1, 6), True, 'bands', int, 'K', 'an integer')
    assert engine.MOSAIC_VALUES['bands'][1] is engine.MOSAIC_BANDS_RANGE and engine.MosaicOptions().bands is None
    assert ('bands', 'blend') in [row[:2] for row in engine.MOSAIC_NEEDS]
    assert list(engine.MOSAIC_OUTPUTS)[:9] == ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples']
    group, tail, dtype, empty, png, how = engine.MOSAIC_OUTPUTS['J_multiband']
    assert (group, tail, dtype, png, how) == ('bands', (3,), torch.float32, 'mosaic_multiband.png', 'stretch') and np.isnan(empty)
    assert engine.MOSAIC_OUTPUTS['J_multiband_filled'] == ('bands_fill', (3,), torch.float32, None, 'mosaic_multiband_filled.png', 'stretch')
    assert sucre._MOSAIC_FLAG['bands'] == '--mosaic-bands' and ('--mosaic-bands', '--mosaic-blend', 'H') in sucre._ONLY_WITH


# ---- the flag -------------------------------------------------------------------------------------------------------------------------

def test_flag_lives_in_extras_and_leaves_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'mosaic_bands' not in vars(off)
    on = p.parse_args(BASE + ['--mosaic', 'results', '--mosaic-blend', '0.5', '--mosaic-bands', '4'])
    assert on.mosaic_bands == 4
    assert vars(off) == {k: v for k, v in vars(on).items() if k not in ('mosaic', 'mosaic_blend', 'mosaic_bands')}
    assert all(a.dest != 'mosaic_bands' for a in p._actions)
    assert '--mosaic-bands K' in p.format_help()


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


def test_the_flag_without_a_blend_is_refused(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-bands', '4'], tmp_path, monkeypatch) == '--mosaic-bands: only with --mosaic-blend H'
    assert run_refused(['--mosaic-bands', '4'], tmp_path, monkeypatch) == '--mosaic-bands: only with --mosaic-blend H'


def test_the_flag_without_a_mosaic_is_refused(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert run_refused(['--mosaic-blend', '0.5', '--mosaic-bands', '4'], tmp_path, monkeypatch) == '--mosaic-blend: only with --mosaic DIR'


@pytest.mark.parametrize('K', ['0', '7', '2.5', 'nan', '-1'])
def test_a_count_outside_the_range_is_refused_before_any_file_is_opened(K, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', '0.5', '--mosaic-bands', K], tmp_path, monkeypatch)
    assert message == f'--mosaic-bands: K must be an integer within [1, 6] bands, not {float(K):g}'
    if K == '2.5':
        assert message == '--mosaic-bands: K must be an integer within [1, 6] bands, not 2.5'


def test_what_mosaic_refuses_stays_refused_with_bands(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', '0.5', '--mosaic-bands', '4', '--shared-water'], tmp_path, monkeypatch)
    assert '--shared-water' in message and '--mosaic-bands' not in message


# ---- the frequency property, by the restatement alone ---------------------------------------------------------------------------------

def test_multiband_has_the_detail_of_the_best_view_and_the_colour_of_the_blend():
    """One plane from 2.0 m (clean) and from 2.5 m (0.2 too bright, +-0.15 of pixel noise), one sample of each per cell, H = 2 m,
    K = 4.  The blend carries the far view's noise into every cell; the multi-band blend keeps the blend's colour -- the offset
    lives in the residual alone -- and draws its fine bands on the near view."""
    views, Js = mref.frequency_pair()
    axes, gsd = torch.eye(3), mref.PAIR_GSD
    base = mref.ref.mosaic(views, Js, axes, gsd, bounds=mref.PAIR_BOUNDS)
    assert (base['Hm'], base['Wm']) == mref.PAIR_HW and bool((base['source'] == 0).all())
    plain = bref.blend(views, Js, axes, gsd, mref.PAIR_H, base=base)
    assert bool((plain['samples'] == 2).all())                      # both views cover every cell, once each
    z = [mref.ref.pixels(v, J, axes)[1] for v, J in zip(views, Js)]
    assert float((z[1] - z[0]).max()) < mref.PAIR_H                # H is larger than the range difference
    got = mref.multiband(views, Js, axes, gsd, mref.PAIR_H, None, mref.PAIR_K, base=base)
    assert torch.equal(got['acc_bands'][-1, :, 3:], plain['acc'][:, 3:])     # the residual has the blend's own weights
    h, l, ok = mref.frequency_conditions(base['J'].numpy(), plain['J_blend'].numpy(), got['J_multiband'].numpy())
    print(f'fine detail: best view {h[0]:.5f}, blend {h[1]:.5f}, multi-band {h[2]:.5f}; colour: {l[0]:.4f}, {l[1]:.4f}, {l[2]:.4f}')
    assert ok[0], h
    assert ok[1], l
