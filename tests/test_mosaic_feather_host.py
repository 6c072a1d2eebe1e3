"""Host tests of the feathered mosaic blend (csrc/mosaic.h, "The feather"): the brute-force distance map of
tests/mosaic_feather_ref.py against the separable form the kernels compute, written out here in numpy; the properties of the
feathered weight; ``engine.mosaic_feather_px``; what --mosaic-feather refuses before any file is opened; and the seam property on
the crafted pair, by the restatement alone.  No GPU."""
import builtins
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_blend_ref as bref
import mosaic_feather_ref as fref
from sucre_amd import engine, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']
WIDTHS = (1, 2, 3, 7, 40, 1024)


def separable(member, F):
    """The form of csrc/mosaic.h: g = min(F, distance along the column to the nearest non-member, rows -1 and H counting as such),
    then dist2 = min(F^2, min over |dx| < F of dx^2 + g(u + dx, v)^2) with g = 0 for a column outside the image."""
    member, F = np.asarray(member, bool), int(F)
    H, W = member.shape
    g = np.zeros((H, W), np.int64)
    run = np.zeros(W, np.int64)
    for v in range(H):                       # down: rows since the last non-member
        run = np.where(member[v], np.minimum(run + 1, F), 0)
        g[v] = run
    run = np.zeros(W, np.int64)
    for v in range(H - 1, -1, -1):           # up
        run = np.where(member[v], np.minimum(run + 1, F), 0)
        g[v] = np.minimum(g[v], run)
    wide = np.zeros((H, W + 2 * W + 2), np.int64)    # W + 1 columns of g = 0 on either side
    wide[:, W + 1:2 * W + 1] = g
    best = np.minimum(g * g, F * F)
    # (|dx| above W reaches no column of the image from any pixel: those terms are dx^2 + 0, larger than the one at |dx| = W)
    for dx in range(1, min(F - 1, W) + 1):
        for sign in (-1, 1):
            there = wide[:, W + 1 + sign * dx:2 * W + 1 + sign * dx]
            best = np.minimum(best, dx * dx + there * there)
    return best


def random_masks():
    rng = np.random.default_rng(20)
    sizes = [(1, 1), (33, 40), (1, 40), (33, 1), (2, 2)]
    for i in range(200):
        H, W = sizes[i] if i < len(sizes) else (int(rng.integers(1, 34)), int(rng.integers(1, 41)))
        density = (0.0, 0.05, 0.5, 1.0)[i % 4]      # the share of non-members
        yield i, rng.random((H, W)) >= density


def test_the_separable_form_equals_the_brute_force_on_200_random_masks():
    """Sizes from 1x1 to 40x33 (W x H), densities of non-members 0, 0.05, 0.5 and 1, every width: exact equality."""
    seen = set()
    for i, member in random_masks():
        near = fref.nearest2(member)
        assert bool((near[member] >= 1).all()) and not near[~member].any()
        for F in WIDTHS:
            want = np.minimum(near, F * F)
            assert np.array_equal(fref.dist2(member, F), want)
            assert np.array_equal(separable(member, F), want), (i, member.shape, F)
        seen.add(member.shape)
    assert {(1, 1), (33, 40)} <= seen


def test_the_two_brute_forces_agree():
    """The literal one (shifted masks under a false frame of width F) against the pairwise one, where the former is affordable."""
    for i, member in random_masks():
        if i >= 24:
            break
        for F in (1, 2, 3, 7):
            assert np.array_equal(fref.dist2_shifted(member, F), fref.dist2(member, F)), (i, F)
    member = next(m for i, m in random_masks() if i == 6)
    assert np.array_equal(fref.dist2_shifted(member, 40), fref.dist2(member, 40))


def test_a_pixel_of_the_first_row_is_one_pixel_from_the_frame():
    d = fref.dist2(np.ones((5, 7), bool), 1024)
    assert d.tolist() == [[1, 1, 1, 1, 1, 1, 1], [1, 4, 4, 4, 4, 4, 1], [1, 4, 9, 9, 9, 4, 1], [1, 4, 4, 4, 4, 4, 1], [1, 1, 1, 1, 1, 1, 1]]
    hole = np.ones((5, 7), bool)
    hole[2, 3] = False
    assert fref.dist2(hole, 1024)[1].tolist() == [1, 4, 2, 1, 2, 4, 1] and fref.dist2(hole, 1024)[2, 3] == 0
    assert fref.dist2(hole, 1)[hole].tolist() == [1] * 34


# ---- the weight ---------------------------------------------------------------------------------------------------------------------

def test_the_weight_stays_within_0_and_4096_and_the_winner_keeps_at_least_4():
    rng = np.random.default_rng(3)
    zmin = rng.uniform(0.5, 5.0, 20000).astype(np.float32)
    z = (zmin + np.where(rng.random(20000) < 0.3, 0, rng.uniform(0, 1.0, 20000))).astype(np.float32)
    z = np.maximum(z, zmin)
    for F in WIDTHS:
        d2 = rng.integers(1, F * F + 2, 20000)
        d2[:4] = (1, F * F, F * F + 1, max(1, F * F - 1))
        for H in (1e-6, 0.05, 0.5, 1e6):
            wq = fref.weights(z, zmin, H, d2, F)
            assert wq.min() >= 0 and wq.max() <= 4096
    # the winner of a cell: z == zmin, so t = 1; at the widest feather and one pixel from the edge
    for H in (1e-6, 0.5, 1e6):
        assert fref.weights(zmin, zmin, H, np.ones(20000, np.int64), 1024).tolist() == [4] * 20000
        assert int(fref.weights(zmin, zmin, H, np.arange(1, 20001), 1024).min()) == 4
    assert fref.weights(zmin[:1], zmin[:1], 0.5, [1], 1023)[0] == 4 and fref.weights(zmin[:1], zmin[:1], 0.5, [1], 16)[0] == 256


def test_a_feather_of_one_pixel_is_the_unfeathered_weight():
    rng = np.random.default_rng(4)
    zmin = rng.uniform(0.5, 5.0, 50000).astype(np.float32)
    z = (zmin + rng.uniform(0, 0.6, 50000)).astype(np.float32)
    for H in (0.05, 0.5, 1e6):
        for d2 in (np.ones(50000, np.int64), rng.integers(1, 5000, 50000)):      # (every member has dist2 >= 1 = F^2)
            assert np.array_equal(fref.weights(z, zmin, H, d2, 1), bref.weights(z, zmin, H))


# ---- engine.mosaic_feather_px -------------------------------------------------------------------------------------------------------

def test_mosaic_feather_px_takes_integral_numbers_in_range():
    assert engine.MOSAIC_FEATHER_RANGE == (1, 1024)
    for good, F in ((1, 1), (1024, 1024), (8.0, 8), ('16', 16), (np.int64(3), 3), (np.float32(64), 64)):
        got = engine.mosaic_feather_px(good)
        assert got == F and type(got) is int
    for bad in (0, 1025, -3, 2.5, float('nan'), float('inf'), 'wide', None, True, 1e9):
        with pytest.raises(ValueError, match=r'feather width F must be an integer within \[1, 1024\]'):
            engine.mosaic_feather_px(bad)


def test_the_functions_refuse_a_feather_without_a_blend_and_a_bad_width(tmp_path, monkeypatch):
    for bad in (0, 1025, 2.5, float('nan')):
        with pytest.raises(ValueError, match='feather width F'):
            engine.mosaic_of([SimpleNamespace()], [None], torch.eye(3), 0.1, blend=0.5, feather=bad)   # before the device is looked at
    with pytest.raises(ValueError, match='blend'):
        engine.mosaic_of([SimpleNamespace()], [None], torch.eye(3), 0.1, feather=8)
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda *a, **k: None)
    for kwargs, text in (({'feather': 8}, '--mosaic-feather: only with --mosaic-blend H'), ({'feather': 0, 'blend': 0.5}, '--mosaic-feather: ')):
        with pytest.raises(SystemExit) as e:
            sucre.mosaic([SimpleNamespace(name='a.png')], None, tmp_path / 'results', tmp_path / 'out', **kwargs)
        assert str(e.value.code).startswith(text) and not (tmp_path / 'out').exists()


# ---- the flag -------------------------------------------------------------------------------------------------------------------------

def test_flag_lives_in_extras_and_leaves_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'mosaic_feather' not in vars(off)
    on = p.parse_args(BASE + ['--mosaic', 'results', '--mosaic-blend', '0.5', '--mosaic-feather', '8'])
    assert on.mosaic_feather == 8
    assert vars(off) == {k: v for k, v in vars(on).items() if k not in ('mosaic', 'mosaic_blend', 'mosaic_feather')}
    assert all(a.dest != 'mosaic_feather' for a in p._actions)
    assert '--mosaic-feather F' in p.format_help()


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
    assert run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-feather', '8'], tmp_path, monkeypatch) == '--mosaic-feather: only with --mosaic-blend H'
    assert run_refused(['--mosaic-feather', '8'], tmp_path, monkeypatch) == '--mosaic-feather: only with --mosaic-blend H'


def test_the_flag_without_a_mosaic_is_refused(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert run_refused(['--mosaic-blend', '0.5', '--mosaic-feather', '8'], tmp_path, monkeypatch) == '--mosaic-blend: only with --mosaic DIR'


@pytest.mark.parametrize('F', ['0', '1025', '2.5', 'nan'])
def test_a_width_outside_the_range_is_refused_before_any_file_is_opened(F, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', '0.5', '--mosaic-feather', F], tmp_path, monkeypatch)
    assert message == f'--mosaic-feather: F must be an integer within [1, 1024] source pixels, not {float(F):g}'


def test_what_mosaic_refuses_stays_refused_with_a_feather(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results'), '--mosaic-blend', '0.5', '--mosaic-feather', '8', '--shared-water'], tmp_path, monkeypatch)
    assert '--shared-water' in message and '--mosaic-feather' not in message


# ---- the seam property, by the restatement alone ------------------------------------------------------------------------------------

def test_the_feather_takes_the_step_out_of_a_footprint_edge():
    """A covers the grid with J = 0.2, B its left half with 0.8, equal ranges.  Unfeathered, the blend steps by 0.3 where B ends;
    with F = 16 no two neighbours along a row differ by more than 0.6 (c + 1) / F + 2^-19, c = 1 source pixel per cell."""
    views, Js = fref.seam_pair()
    axes, gsd, F = torch.eye(3), fref.SEAM_GSD, fref.SEAM_F
    plain = bref.blend(views, Js, axes, gsd, 0.5)
    assert (plain['base']['Hm'], plain['base']['Wm']) == fref.SEAM_HW
    assert torch.equal(plain['samples'][:, :32], torch.full((48, 32), 2, dtype=torch.int32)) and bool((plain['samples'][:, 32:] == 1).all())
    assert bool((plain['wq'] == 4096).all())      # the ranges tie: the weights of the feathered run are the feather alone
    assert abs(fref.largest_row_step(plain['J_blend']) - 0.3) <= 2.0 ** -19
    got = fref.blend(views, Js, axes, gsd, 0.5, F, base=plain['base'])
    step = fref.largest_row_step(got['J_blend'])
    print(f'largest step along a row: {fref.largest_row_step(plain["J_blend"]):.6f} unfeathered, {step:.6f} at F = {F}; bound {fref.seam_bound():.6f}')
    assert step <= fref.seam_bound()
    assert torch.equal(got['samples'], plain['samples']) and bool((got['samples'][plain['samples'] > 0] >= 1).all())
    one = fref.blend(views, Js, axes, gsd, 0.5, 1, base=plain['base'])
    assert torch.equal(one['acc'], plain['acc'])
