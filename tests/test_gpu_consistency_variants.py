"""The consistency check (sucre_view_consistency, engine.view_consistency, --check-consistency) at real tile counts, with general
camera matrices and in every mode of the command line.

The yardstick is tests/consistency_ref.py evaluated on the match lists of the CPU ORACLE (oracle.match_view on the matrices the
reference derives, as tools/camera_sweep.py does) -- not on the engine's own match map, so a wrong match set would show.  The
bars are those of tests/test_gpu_consistency.py, derived in its docstring: matches, valid pairs and ``count`` exactly; each of
the 24 sums of a view within 2^-15 of the sum of its terms' magnitudes (per (16x16 tile, view) in float32; the float64 sum over
the tiles adds nothing visible); ``ssd`` within n_views x 2^-23 relative and exactly 0 where ``count`` is 0.  Everything else is
bit equality.  Every case first asserts, on the oracle's lists alone, that its scene holds the edge it was chosen for.

Tile counts pinned here: 306 tiles (275x259: 18 x 17, partial tiles on both axes; threads 0..49 of consistency_view_sum_kernel
take two tiles, 39 tiles per XCD band, 6 of the 312 workgroups idle), 24 tiles (96x64, against views of 128x80), 2 tiles (17x5)
with engine.MAX_VIEWS views.
"""
import contextlib
import io
import os
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import consistency_ref as ref
import helpers
from oracle import oracle
from sucre_amd import engine, synth
from test_gpu_consistency import DEV, abi_call, restored_like, same_bits

pytestmark = pytest.mark.gpu

_MADE = {}


def made(key, make):
    """Scenes, oracle lists and references are made once, shared and never changed."""
    if key not in _MADE:
        _MADE[key] = make()
    return _MADE[key]


# ---- the yardstick: the oracle's matches, the float64 reference on them -----------------------------------------------------
def spec(view, K):
    """(view, K, H, W): a synthetic view with the camera matrix it is seen through."""
    H, W = view.depth_u16.shape
    return view, K, int(H), int(W)


def oracle_lists(target, views):
    """(u1, v1, u2, v2) of the target with every view, by the CPU oracle."""
    tv, tK, tH, tW = target
    cam1 = oracle.make_cam(tH, tW, **helpers.cam_matrices(tK, tv.R, tv.t))
    d1 = tv.depth_f32().numpy()
    out = []
    for v, K, h, w in views:
        cam2 = oracle.make_cam(h, w, **helpers.cam_matrices(K, v.R, v.t))
        m = oracle.match_view(d1, cam1, v.depth_f32().numpy(), cam2)
        out.append(tuple(x.astype(np.int64) for x in (m.u1, m.v1, m.u2, m.v2)))
    return out


def device_view(s):
    v, K, _, _ = s
    return engine.DeviceView(depth=v.depth_f32().to(DEV).contiguous(), rgb=v.rgb_u8.to(DEV).contiguous(), K=K, R=v.R, t=v.t, name=v.name)


def reference_of(lists, target, J_A, views, Js, raw_target=True):
    return ref.reference(J_A.cpu().numpy(), target[0].rgb_u8.numpy() if raw_target else None,
                         [(l, None if J is None else J.cpu().numpy(), s[0].rgb_u8.numpy()) for l, J, s in zip(lists, Js, views)])


def same_pattern(x, y):
    """NaN, +inf and -inf at the same entries."""
    return all(np.array_equal(f(x), f(y)) for f in (np.isnan, np.isposinf, np.isneginf))


def compare(label, got, want, lists, Js):
    """The bars of test_gpu_consistency.check_against_reference, on the oracle's lists; entries that are not finite in the
    reference must be the same non-finite value in the result, all others keep the bars."""
    count64, ssd64, stats64, stats_abs, valids = want
    count, ssd, stats = (x.cpu().numpy() for x in got)
    n_views = len(lists)
    assert count.dtype == np.int32 and ssd.dtype == np.float32 and stats.dtype == np.float64 and stats.shape == (n_views, 26)
    for k, l in enumerate(lists):   # the matches are the ORACLE's
        assert stats[k, 0] == (0 if Js[k] is None else len(l[0])), (label, k, stats[k, 0], len(l[0]))
    assert np.array_equal(stats[:, :2], stats64[:, :2]), (label, stats[:, :2].tolist(), stats64[:, :2].tolist())
    assert np.array_equal(count, count64), (label, int((count != count64).sum()))
    assert same_pattern(stats, stats64) and same_pattern(ssd, ssd64), label
    with np.errstate(invalid='ignore'):
        fin = np.isfinite(stats64[:, 2:])
        err = np.where(fin, np.abs(stats[:, 2:] - stats64[:, 2:]), 0.0)
        bar = np.where(fin, 2.0 ** -15 * stats_abs[:, 2:], 0.0)
        worst = (err / np.where(bar > 0, bar, 1.0)).max()
        print(f'{label}: largest |sum - sum64| / (2^-15 sum |term|) = {worst:.3e} over {n_views} views, pairs per view '
              f'{stats[:, 1].astype(int).tolist() if n_views <= 16 else int(stats[:, 1].sum())}')
        assert (err <= bar).all(), (label, np.argwhere(err > bar)[:5], worst)
        assert np.array_equal(ssd[count64 == 0], np.zeros_like(ssd[count64 == 0]))
        finp = np.isfinite(ssd64)
        rel = np.where(finp, np.abs(ssd - ssd64), 0.0)
        ssd_bar = np.where(finp, n_views * 2.0 ** -23 * ssd64, 0.0)
        worst_px = (rel / np.where(finp & (ssd64 > 0), ssd64, 1.0)).max()
        print(f'{label}: largest |ssd - ssd64| / ssd64 = {worst_px:.3e}, bar {n_views * 2.0 ** -23:.3e}')
        assert (rel <= ssd_bar).all(), (label, worst_px)
    return stats, count, ssd


def differs(a, b):
    return [not all(np.array_equal(x, y) for x, y in zip(la, lb)) for la, lb in zip(a, b)]


# ---- a. more tiles than threads, ragged on both axes; b. general camera matrices ------------------------------------------
def skewed(K, s):
    K = K.clone()
    K[0, 1] = s   # (K[2][2] stays 1: the reference's unprojection is not invariant under a scaling of K)
    return K


def big(variant='pinhole'):
    """make_scene(275, 259, 3, seed=7, far_views=1), target view 2: 18 x 17 = 306 tiles.  ``variant``: 'pinhole'; 'target' -- a
    skewed K on the target only (every view takes the general chains); 'views' -- a skew on views 0 and 3 only (one launch mixes
    pinhole and general views); 'both'."""
    def make():
        scene = made('scene275', lambda: synth.make_scene(275, 259, 3, seed=7, far_views=1))
        assert scene.target == 2 and len(scene.views) == 5
        tK = skewed(scene.K, 1.5) if variant in ('target', 'both') else scene.K
        vK = lambda i: skewed(scene.K, -0.8) if variant in ('views', 'both') and i in (0, 3) else scene.K   # noqa: E731
        target = spec(scene.views[2], tK)
        views = [spec(v, vK(i)) for i, v in enumerate(scene.views) if i != 2]
        lists = oracle_lists(target, views)
        n = [len(l[0]) for l in lists]
        assert min(n[:3]) > 0 and n[3] == 0, n   # three neighbours and the far view
        return target, views, lists
    target, views, lists = made(('big', variant), make)
    dev = made(('big dev', variant), lambda: (device_view(target), [device_view(s) for s in views]))
    Js = made('big J', lambda: (restored_like(dev[0], 100), [restored_like(dev[1][0], 200), None, restored_like(dev[1][2], 202),
                                                              restored_like(dev[1][3], 203)]))
    want = made(('big ref', variant), lambda: reference_of(lists, target, Js[0], views, Js[1]))
    return dev[0], Js[0], dev[1], Js[1], lists, want


def test_more_tiles_than_threads_against_the_oracle():
    """306 tiles: threads 0..49 of consistency_view_sum_kernel take a second tile, the scratch index view * n_tiles + tile runs
    past 256, the XCD bands hold 39 tiles and six workgroups of the 312 have none."""
    target, J_A, views, Js, lists, want = big()
    H, W = target.depth.shape
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert tiles == 18 * 17 == 306 > 256 and W % 16 and H % 16 and tiles % 8 and 8 * ((tiles + 7) // 8) - tiles == 6
    assert Js[1] is None and len(lists[1][0]) > 0
    valids = want[4]
    assert all(0 < valids[k].sum() < len(valids[k]) for k in (0, 2))   # NaNs make pairs invalid, not all of them
    # valid pairs in the partial tiles of the right edge and in tiles beyond the 256th; no neighbour sees the target's last rows
    # (the partial tiles of the bottom edge must come back zero here; the target among its own views fills them)
    u1, v1 = (np.concatenate([lists[k][i][valids[k]] for k in (0, 2)]) for i in (0, 1))
    assert (u1 >= 272).any() and ((v1 // 16) * 18 + u1 // 16 >= 256).any() and v1.max() < 256 < H
    stats, _, _ = compare('275x259, 306 tiles', engine.view_consistency(target, J_A, views, Js), want, lists, Js)
    assert np.array_equal(stats[1], np.zeros(26)) and np.array_equal(stats[3], np.zeros(26))


def test_more_tiles_than_threads_two_calls_and_dirty_scratch_give_the_same_bits():
    target, J_A, views, Js, _, _ = big()
    a = engine.view_consistency(target, J_A, views, Js)
    b = engine.view_consistency(target, J_A, views, Js)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert same_bits(x, y)
    for fill in (0xFF, 0x00):
        rc, count, ssd, stats = abi_call(target, J_A, views, Js, fill)
        assert rc == 0
        for x, y in zip(a, (count, ssd, stats)):
            assert same_bits(x, y), fill


@pytest.mark.parametrize('variant', ['target', 'views', 'both'])
def test_general_camera_matrices_against_the_oracle(variant):
    """``pin`` is formed per view: a skewed target switches every view to the general chains, skewed views 0 and 3 mix general
    and pinhole views in one launch."""
    target, J_A, views, Js, lists, want = big(variant)
    moved = differs(big()[4], lists)
    assert any(moved), 'the skew must move a match, or the general path proves nothing'
    if variant == 'views':
        assert moved[0] and moved[2] and not moved[1]
    compare(f'275x259, skew on {variant}', engine.view_consistency(target, J_A, views, Js), want, lists, Js)


# ---- c. other cameras -------------------------------------------------------------------------------------------------------
def test_other_camera_sizes_a_camera_looking_away_and_a_twisted_one():
    """The layout of test_gpu_parity's test_views_with_other_camera_sizes_and_cameras_looking_away: views larger than the target
    (128x80 against 96x64, their own K and their own J), the target flipped to look up, a neighbour rolled by 1.5 rad."""
    def make():
        a = synth.make_scene(96, 64, 3, seed=31)
        b = synth.make_scene(128, 80, 3, seed=31)
        tgt = a.views[a.target]
        near = [v for i, v in enumerate(a.views) if i != a.target]
        flipped = synth.SynthView(name='flip.png', R=(tgt.R @ torch.diag(torch.tensor([1.0, -1.0, -1.0]))).contiguous(), t=tgt.t,
                                  depth_u16=tgt.depth_u16, rgb_u8=tgt.rgb_u8)
        roll = torch.tensor(synth._rodrigues(np.array([0.0, 0.0, 1.5])), dtype=torch.float32)
        twisted = synth.SynthView(name='twist.png', R=(near[0].R @ roll).contiguous(), t=near[0].t, depth_u16=near[0].depth_u16,
                                  rgb_u8=near[0].rgb_u8)
        target = spec(tgt, a.K)
        views = [spec(v, a.K) for v in near] + [spec(v, b.K) for v in b.views] + [spec(flipped, a.K), spec(twisted, a.K)]
        return target, views, oracle_lists(target, views)
    target, views, lists = made('other cameras', make)
    n = [len(l[0]) for l in lists]
    assert [s[2:] for s in views[3:7]] == [(80, 128)] * 4 and min(n[:3]) > 0 and min(n[3:7]) > 0, n
    assert any((l[2] >= 96).any() or (l[3] >= 64).any() for l in lists[3:7])   # partners beyond the target's own size
    assert n[7] > 0 and n[8] > 0   # no in-front-of-camera test: the flipped target matches; so does the rolled neighbour
    tv, dv = device_view(target), [device_view(s) for s in views]
    J_A = restored_like(tv, 300)
    Js = [restored_like(v, 310 + k) for k, v in enumerate(dv)]
    assert tuple(Js[3].shape) == (80, 128, 3)
    want = reference_of(lists, target, J_A, views, Js)
    stats, _, _ = compare('96x64 against 128x80, flipped and twisted views', engine.view_consistency(tv, J_A, dv, Js), want, lists, Js)
    assert (stats[3:7, 1] > 0).all(), 'the larger views contribute valid pairs'
    print(f'matches per view {n}')


# ---- d. the target among its own views; e. a target without raw colours ----------------------------------------------------
def test_the_target_among_its_own_views():
    target, J_A, views, Js, _, _ = big()
    scene = made('scene275', None)
    tspec, nspec = spec(scene.views[2], scene.K), spec(scene.views[0], scene.K)
    lists = made('self lists', lambda: oracle_lists(tspec, [tspec, nspec]))
    depth_ok = scene.views[2].depth_u16.numpy() > 0
    u1, v1, u2, v2 = lists[0]
    on = np.zeros_like(depth_ok)
    on[v1, u1] = True
    assert np.array_equal(on, depth_ok) and np.array_equal(u1, u2) and np.array_equal(v1, v2)   # every pixel with a depth, with itself
    both, both_J = [target, views[0]], [J_A, Js[0]]
    want = reference_of(lists, tspec, J_A, [tspec, nspec], both_J)
    self_pair = np.zeros_like(depth_ok)
    self_pair[v1[want[4][0]], u1[want[4][0]]] = True   # the reference's valid pairs of view 0
    assert np.array_equal(self_pair, depth_ok & ~np.isnan(J_A.cpu().numpy()).any(axis=2))
    # whole waves of valid lanes: a 4-row x 16-column block of a tile, fully valid in the view-0 row
    blocks = self_pair[:256, :272].reshape(64, 4, 17, 16).all(axis=(1, 3))
    assert blocks.any() and not blocks.all() and self_pair[256:].any() and self_pair[:, 272:].any()   # (and both ragged edges)
    stats, count, ssd = compare('275x259, the target among its views', engine.view_consistency(target, J_A, both, both_J), want, lists, both_J)
    assert stats[0, 0] == depth_ok.sum() and stats[0, 1] == self_pair.sum() < depth_ok.sum()
    assert np.array_equal(stats[0, 2:5], np.zeros(3)) and np.array_equal(stats[0, 14:17], np.zeros(3))     # sum d^2: exactly 0.0
    for o in (5, 17):                                                                                        # a^2 = b^2 = a b, by bits
        assert stats[0, o:o + 3].tobytes() == stats[0, o + 3:o + 6].tobytes() == stats[0, o + 6:o + 9].tobytes() and (stats[0, o:o + 3] > 0).all()
    alone = engine.view_consistency(target, J_A, [views[0]], [Js[0]])
    assert same_bits(torch.from_numpy(ssd), alone[1])
    assert np.array_equal(count, alone[0].cpu().numpy() + self_pair)


def test_a_target_without_raw_colours():
    target, J_A, views, Js, _, _ = big()
    bare = target.as_float_colour()
    assert bare.rgb.dtype == torch.float32 and all(v.rgb.dtype == torch.uint8 for v in views)
    with_raw = engine.view_consistency(target, J_A, views, Js)
    without = engine.view_consistency(bare, J_A, views, Js)
    assert bool((with_raw[2][:, 14:17] > 0).any()) and np.array_equal(without[2][:, 14:].cpu().numpy(), np.zeros((len(views), 12)))
    assert same_bits(with_raw[2][:, :14], without[2][:, :14]) and same_bits(with_raw[0], without[0]) and same_bits(with_raw[1], without[1])


# ---- f. the view limit ------------------------------------------------------------------------------------------------------
def test_the_view_limit():
    """engine.MAX_VIEWS views of a 17x5 image (2 tiles): the scratch sizing and the n_views-workgroup grid at the cap."""
    n = engine.MAX_VIEWS
    assert n == 4096
    scene = synth.make_scene(17, 5, 3, seed=3)
    four = [spec(v, scene.K) for v in scene.views]
    target = four[scene.target]
    lists4 = oracle_lists(target, four)
    assert len(four) == 4 and all(len(l[0]) > 0 for l in lists4), [len(l[0]) for l in lists4]
    tv, dv4 = device_view(target), [device_view(s) for s in four]
    J_A = restored_like(tv, 400)
    J4 = [restored_like(v, 410 + k) for k, v in enumerate(dv4)]
    cyc = lambda x: [x[k % 4] for k in range(n)]   # noqa: E731
    views, lists, dv, Js = cyc(four), cyc(lists4), cyc(dv4), cyc(J4)
    want = reference_of(lists, target, J_A, views, Js)
    got = engine.view_consistency(tv, J_A, dv, Js)
    stats, count, _ = compare(f'17x5 against {n} views', got, want, lists, Js)     # (ssd: within 4096 x 2^-23)
    for k in range(4):
        assert (stats[k::4].view(np.uint64) == stats[k].view(np.uint64)).all(), k
    one = engine.view_consistency(tv, J_A, dv4, J4)
    assert same_bits(one[2], got[2][:4]) and np.array_equal(count, one[0].cpu().numpy() * (n // 4)) and count.max() > 1024
    with pytest.raises(ValueError, match='1..4096'):   # refused on the host, before any launch
        engine.view_consistency(tv, J_A, dv + dv[:1], Js + Js[:1])


# ---- g. infinities in J -----------------------------------------------------------------------------------------------------
def test_infinities_in_the_restored_images():
    """Closed-form overflow can write +-inf into a J file.  A pair stays valid (only NaN makes it invalid); inf - inf is NaN."""
    def make():
        scene = synth.make_scene(37, 21, 2, seed=3)
        target = spec(scene.views[scene.target], scene.K)
        views = [spec(v, scene.K) for i, v in enumerate(scene.views) if i != scene.target]
        return target, views, oracle_lists(target, views)
    target, views, lists = made('infinities', make)
    assert len(views) == 2 and all(len(l[0]) > 10 for l in lists)
    tv, dv = device_view(target), [device_view(s) for s in views]
    J_A = restored_like(tv, 500).cpu()
    Js = [restored_like(v, 510 + k).cpu() for k, v in enumerate(dv)]
    nan_free = lambda J, v, u: not bool(torch.isnan(J[v, u]).any())   # noqa: E731
    # a matched target pixel and its partner in view 0, both without a NaN: +inf in channel 1 of both
    (u1, v1, u2, v2), (p1, q1, p2, q2) = lists
    i = next(i for i in range(len(u1)) if nan_free(J_A, v1[i], u1[i]) and nan_free(Js[0], v2[i], u2[i]))
    J_A[v1[i], u1[i], 1] = float('inf')
    Js[0][v2[i], u2[i], 1] = float('inf')
    # a pixel of view 1 whose partner is finite (another target pixel): -inf in channel 2
    j = next(j for j in range(len(p1)) if (p1[j], q1[j]) != (u1[i], v1[i]) and nan_free(J_A, q1[j], p1[j]) and nan_free(Js[1], q2[j], p2[j]))
    Js[1][q2[j], p2[j], 2] = float('-inf')
    J_A, Js = J_A.to(DEV), [J.to(DEV) for J in Js]
    want = reference_of(lists, target, J_A, views, Js)
    count64, ssd64, stats64 = want[:3]
    # what the reference says the planted values do: the pairs stay valid, d is NaN in one sum and +inf in another
    assert want[4][0][i] and want[4][1][j] and count64[v1[i], u1[i]] >= 1
    assert np.isnan(stats64[0, 2 + 1]) and np.isposinf(stats64[0, 5 + 1]) and np.isposinf(stats64[0, 8 + 1]) and np.isposinf(stats64[0, 11 + 1])
    assert np.isposinf(stats64[1, 2 + 2]) and np.isposinf(stats64[1, 8 + 2]) and np.isneginf(stats64[1, 11 + 2]) and np.isfinite(stats64[1, 5 + 2])
    assert np.isnan(ssd64[v1[i], u1[i], 1]) and np.isposinf(ssd64[q1[j], p1[j], 2])
    assert np.isfinite(stats64[:, 14:]).all() and np.isfinite(stats64).sum() > 40
    compare('37x21 with infinities', engine.view_consistency(tv, J_A, dv, Js), want, lists, Js)


# ---- the command line -------------------------------------------------------------------------------------------------------
CACHE_GB = 'SUCRE_CONSISTENCY_CACHE_GB'
N_IMAGES = 8
IMAGE_BYTES = 96 * 64 * 12


def run_cli(argv, env=None):
    """sucre.main in this process with ``env`` set on top of a clean environment.  Returns what it printed, the files the
    non-lazy ``_read_restored`` calls read and the names the restored-image cache dropped, both in order."""
    from types import SimpleNamespace
    from sucre_amd import sucre
    keys = ('WORLD_SIZE', CACHE_GB, 'SUCRE_CULL_VIEWS')
    saved = {k: os.environ.pop(k) for k in keys if k in os.environ}
    os.environ.update(env or {})
    run = SimpleNamespace(printed='', reads=[], evicted=[])
    real_read, real_get = sucre._read_restored, sucre._RestoredCache.get

    def read(path, image, lazy=False):
        if not lazy:
            run.reads.append(Path(path).name)
        return real_read(path, image, lazy)

    def get(self, image, pinned):
        before = list(self.entries)
        J = real_get(self, image, pinned)
        run.evicted.extend(n for n in before if n not in self.entries)
        return J

    sucre._read_restored, sucre._RestoredCache.get = read, get
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            sucre.main([str(a) for a in argv])
    finally:
        sucre._read_restored, sucre._RestoredCache.get = real_read, real_get
        run.printed = printed.getvalue()
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(saved)
    return run


@pytest.fixture(scope='module')
def strip(tmp_path_factory):
    """make_survey(96, 64, 8, 1, seed=5, spacing=0.5) on disk -- a strip of 8 images that see at most two images along --,
    restored with the renderer's true water, then checked once with default knobs: the baseline directory."""
    root = tmp_path_factory.mktemp('consistency_strip')
    survey = synth.make_survey(96, 64, N_IMAGES, 1, seed=5, spacing=0.5)
    synth.write_to_disk(survey, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    names = [v.name for v in survey.views]
    base = ['--image-dir', root / 'images', '--depth-dir', root / 'depth', '--model-dir', root / 'model']
    every = ['--image-ids', '1', str(N_IMAGES + 1)]
    restored, baseline = root / 'restored', root / 'baseline'
    run_cli(base + every + ['--output-dir', restored, '--apply-water', root / 'true_water.pt'])
    run = run_cli(base + every + ['--output-dir', baseline, '--check-consistency', restored])
    return dict(root=root, survey=survey, names=names, base=base, every=every, restored=restored, baseline=baseline, printed=run.printed,
                reads=run.reads, evicted=run.evicted)


def check(strip, out, extra=(), targets=None, env=None, restored=None):
    targets = strip['every'] if targets is None else targets
    return run_cli(strip['base'] + list(targets) + ['--output-dir', out, '--check-consistency', restored or strip['restored']] + list(extra), env)


def same_value(a, b, where):
    """Tensors by bits, everything else by ==."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and same_bits(a, b), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            same_value(a[k], b[k], f'{where}[{k}]')
    else:
        assert type(a) is type(b) and a == b, where


def same_file(a: Path, b: Path):
    if a.suffix == '.pt':
        same_value(torch.load(a), torch.load(b), a.name)
    else:
        from PIL import Image as PILImage
        x, y = np.asarray(PILImage.open(a)), np.asarray(PILImage.open(b))
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), a.name


def files_of(d: Path):
    return sorted(p.name for p in d.iterdir())


def target_files(names):
    return sorted(f'{Path(n).stem}_consistency.{ext}' for n in names for ext in ('pt', 'png'))


def per_target(d: Path, name):
    return torch.load(d / f'{Path(name).stem}_consistency.pt')


def rows_by_view(rec):
    return {v: rec['stats'][k] for k, v in enumerate(rec['views'])}


def test_cli_baseline_is_the_strip_the_cases_below_need(strip):
    """What the oracle says about the strip (on the CPU): matches only between images at most two apart, 14 between 4 and 6, 543
    between 2 and 4 -- and the baseline run found exactly those, caching every restored image."""
    names, baseline = strip['names'], strip['baseline']
    assert files_of(baseline) == sorted(target_files(names) + ['consistency.pt'])
    # the cameras as the command line reads them back from the COLMAP text model (the poses pass through a quaternion in text:
    # not the renderer's bits, and one match of 6 <-> 7 moves with them)
    from types import SimpleNamespace
    from sucre_amd import sfm
    model = sfm.COLMAPModel(strip['root'] / 'model', strip['root'] / 'images', strip['root'] / 'depth')
    specs = [spec(SimpleNamespace(R=model[v.name].pose.R, t=model[v.name].pose.t.view(3, 1), depth_f32=v.depth_f32, depth_u16=v.depth_u16),
                  model[v.name].camera.K) for v in strip['survey'].views]
    n = np.array([[len(l[0]) for l in oracle_lists(s, specs)] for s in specs])
    far = np.abs(np.subtract.outer(np.arange(N_IMAGES), np.arange(N_IMAGES))) > 2
    assert (n[far] == 0).all() and n[4, 6] == n[6, 4] == 14 and n[2, 4] == n[4, 2] == 543 and (n.diagonal() > 0).all()
    kept_views = []
    for i, name in enumerate(names):
        rec = per_target(baseline, name)
        kept_views.append(len(rec['views']))
        assert name not in rec['views']
        for k, v in enumerate(rec['views']):
            assert int(rec['stats'][k, 0]) == n[i, names.index(v)], (name, v)
        assert all(n[i, j] == 0 for j, v in enumerate(names) if v not in rec['views'] and j != i)   # the cull dropped no match
    assert kept_views == [2, 3, 4, 4, 4, 4, 3, 2], kept_views
    assert sorted(strip['reads']) == sorted(Path(n).with_suffix('.pt').name for n in names)   # the default budget caches: 8 reads
    assert f'pairs of {N_IMAGES} images' in strip['printed']


def test_cli_eviction_changes_no_bit(strip, tmp_path):
    """A budget of five images: every target and its (at most four) neighbours fit, the eight images do not.  Walking the strip
    in order the cache drops images 0, 1 and 2 when 5, 6 and 7 arrive and never needs them again (8 reads: measured, and what the
    LRU order gives on paper), so the targets are also taken in an order that comes back to what was dropped: there an image is
    read more than once, and every per-target file and every row of consistency.pt is still the baseline's."""
    budget = 5 * IMAGE_BYTES
    gb = repr(budget / 2 ** 30)
    assert int(float(gb) * 2 ** 30) == budget == 368640 < N_IMAGES * IMAGE_BYTES == 589824
    names, baseline = strip['names'], strip['baseline']
    assert len(strip['reads']) == N_IMAGES and not strip['evicted']            # the default budget caches everything
    run = check(strip, tmp_path / 'out', env={CACHE_GB: gb})
    print(f'in order: {len(run.reads)} reads, dropped {run.evicted}')
    assert run.evicted == ['img_0000.png', 'img_0001.png', 'img_0002.png'] and set(run.reads) == set(strip['reads'])
    assert files_of(tmp_path / 'out') == files_of(baseline)
    for f in files_of(baseline):
        same_file(tmp_path / 'out' / f, baseline / f)
    # ... and in an order that returns to dropped images
    order = [names[i] for i in (0, 4, 1, 5, 2, 6, 3, 7)]
    (tmp_path / 'order.txt').write_text('\n'.join(order) + '\n')
    run = check(strip, tmp_path / 'back', targets=['--image-list', tmp_path / 'order.txt'], env={CACHE_GB: gb})
    print(f'back and forth: {len(run.reads)} reads, dropped {run.evicted}')
    assert len(run.reads) > N_IMAGES and set(run.reads) == set(strip['reads']) and 0 < len(run.reads) - len(run.evicted) <= 5
    assert files_of(tmp_path / 'back') == files_of(baseline)
    for f in target_files(names):
        same_file(tmp_path / 'back' / f, baseline / f)
    a, b = torch.load(tmp_path / 'back' / 'consistency.pt'), torch.load(baseline / 'consistency.pt')
    assert a['targets'] == order and a['pooled_n'] == b['pooled_n']
    row = {p: i for i, p in enumerate(zip(b['a'], b['b']))}
    assert sorted(zip(a['a'], a['b'])) == sorted(row)
    at = [row[p] for p in zip(a['a'], a['b'])]
    for key in ('n', 'rms_restored', 'rms_raw', 'gain', 'rms_restored_gain'):
        assert same_bits(a[key], b[key][at]), key


def test_cli_a_target_that_cannot_fit_is_refused_not_attempted(strip, tmp_path):
    budget = 4 * IMAGE_BYTES
    gb = repr(budget / 2 ** 30)
    assert int(float(gb) * 2 ** 30) == budget == 294912
    out = tmp_path / 'out'
    with pytest.raises(SystemExit) as e:
        check(strip, out, env={CACHE_GB: gb})
    said = str(e.value.code)
    assert CACHE_GB in said and 'img_0002.png' in said and '--filter-images-path' in said, said
    done = target_files(strip['names'][:2])   # targets 0 and 1 have two and three neighbours
    assert files_of(out) == done
    for f in done:
        same_file(out / f, strip['baseline'] / f)


def test_cli_two_ranks_equal_one_process(strip, tmp_path):
    import socket
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    clean = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT',
                                                              CACHE_GB, 'SUCRE_CULL_VIEWS')}
    clean['PYTHONPATH'] = str(root) + os.pathsep + clean.get('PYTHONPATH', '')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = tmp_path / 'two'
    cmd = [sys.executable, '-m', 'sucre_amd.sucre'] + [str(a) for a in strip['base'] + strip['every']] + [
        '--output-dir', str(out), '--check-consistency', str(strip['restored'])]
    procs = [subprocess.Popen(cmd, env=dict(clean, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                                            MASTER_PORT=str(port), SUCRE_DIST_BACKEND='gloo'),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=root) for k in range(2)]
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    line = f'pairs of {N_IMAGES} images'
    assert sum(('consistency over ' in so and line in so) for so, _ in outs) == 1, 'rank 0 alone reports'
    assert all(sum(f'{n}: consistency with ' in so for so, _ in outs) == 1 for n in strip['names'])   # every target on one rank
    assert files_of(out) == files_of(strip['baseline'])
    for f in files_of(out):
        same_file(out / f, strip['baseline'] / f)


def seven(strip, tmp_path):
    """The restored directory without img_0003.pt, and a list of the other seven as targets."""
    part = tmp_path / 'restored_without_3'
    part.mkdir()
    for p in strip['restored'].iterdir():
        if p.name != 'img_0003.pt':
            shutil.copy(p, part / p.name)
    names = [n for n in strip['names'] if n != 'img_0003.png']
    (tmp_path / 'seven.txt').write_text('\n'.join(names) + '\n')
    return part, names, ['--image-list', tmp_path / 'seven.txt']


def rows_equal_the_baselines(strip, out, names, gone='img_0003.png'):
    shared = 0
    for name in names:
        rec, base = per_target(out, name), per_target(strip['baseline'], name)
        assert gone not in rec['views'] and rec['views'] == [v for v in base['views'] if v != gone], name
        have, want = rows_by_view(rec), rows_by_view(base)
        for v in rec['views']:
            assert same_bits(have[v], want[v]), (name, v)   # rows are independent per view
            shared += 1
    return shared


def test_cli_images_without_a_restored_image_are_skipped_and_counted(strip, tmp_path):
    from sucre_amd import loader
    part, names, listed = seven(strip, tmp_path)
    run = check(strip, tmp_path / 'out', targets=listed, restored=part)
    assert f'1 of {N_IMAGES} images have no restored image' in run.printed
    assert files_of(tmp_path / 'out') == sorted(target_files(names) + ['consistency.pt'])
    assert rows_equal_the_baselines(strip, tmp_path / 'out', names) == sum(len(per_target(strip['baseline'], n)['views']) for n in names) - 4
    merged = torch.load(tmp_path / 'out' / 'consistency.pt')
    assert merged['targets'] == names and 'img_0003.png' not in merged['a'] + merged['b']
    # among the targets it is an error, before any image is decoded
    decoded = []
    real = {fn: getattr(loader, fn) for fn in ('_imread_rgb_u8', '_imread_depth_u16')}
    try:
        for fn, f in real.items():
            setattr(loader, fn, lambda path, f=f: (decoded.append(Path(path).name), f(path))[1])
        with pytest.raises(SystemExit) as e:
            check(strip, tmp_path / 'refused', restored=part)
    finally:
        for fn, f in real.items():
            setattr(loader, fn, f)
    assert 'img_0003.pt' in str(e.value.code) and 'missing' in str(e.value.code) and not decoded
    assert not (tmp_path / 'refused').exists() or not files_of(tmp_path / 'refused')


def test_cli_cull_off(strip, tmp_path):
    names = strip['names']
    check(strip, tmp_path / 'out', env={'SUCRE_CULL_VIEWS': '0'})
    for name in names:
        rec, base = per_target(tmp_path / 'out', name), per_target(strip['baseline'], name)
        assert rec['views'] == [n for n in names if n != name]
        have, want = rows_by_view(rec), rows_by_view(base)
        for v in rec['views']:
            if v in want:
                assert same_bits(have[v], want[v]), (name, v)
            else:
                assert float(have[v][0]) == 0.0 and not bool(have[v].any()), (name, v)   # what the cull drops matches nothing
        assert same_bits(rec['count'], base['count']) and same_bits(rec['ssd'], base['ssd'])
    a, b = torch.load(tmp_path / 'out' / 'consistency.pt'), torch.load(strip['baseline'] / 'consistency.pt')
    for key in ('pooled_n', 'pooled_restored', 'pooled_raw', 'pooled_restored_gain', 'a', 'b', 'n', 'rms_restored', 'rms_raw', 'gain'):
        same_value(a[key], b[key], key)


def test_cli_min_cover_filter_images_path_and_image_name(strip, tmp_path):
    names, baseline = strip['names'], strip['baseline']
    # --min-cover 0.01: more than 61.44 matches are needed; 4 <-> 6 have 14, 2 <-> 4 have 543
    check(strip, tmp_path / 'cover', extra=['--min-cover', '0.01'])
    for t, v, n in ((4, 6, 14), (6, 4, 14), (4, 2, 543)):
        rec, base = per_target(tmp_path / 'cover', names[t]), per_target(baseline, names[t])
        k = rec['views'].index(names[v])
        assert base['views'] == rec['views'] and int(rec['stats'][k, 0]) == n and same_bits(rec['stats'], base['stats'])
        assert bool(base['kept'][k]) and bool(rec['kept'][k]) == (n > 0.01 * 96 * 64) and rec['min_cover'] == 0.01
        assert float(base['stats'][k, 1]) > 0   # (the pair has valid pixel pairs: dropping it changes consistency.pt)
    a, b = torch.load(tmp_path / 'cover' / 'consistency.pt'), torch.load(baseline / 'consistency.pt')
    pairs = lambda m: list(zip(m['a'], m['b']))   # noqa: E731
    lost = [(names[4], names[6]), (names[6], names[4])]
    assert all(p in pairs(b) for p in lost) and pairs(a) == [p for p in pairs(b) if p not in lost]
    keep = [i for i, p in enumerate(pairs(b)) if p not in lost]
    for key in ('n', 'rms_restored', 'rms_raw', 'gain', 'rms_restored_gain'):
        assert same_bits(a[key], b[key][keep]), key
    assert a['pooled_n'] == b['pooled_n'] - int(b['n'][[i for i in range(len(pairs(b))) if i not in keep]].sum())
    # --filter-images-path: the image is no one's neighbour -- the rows of the run without its restored image
    (tmp_path / 'filter.txt').write_text('img_0003.png\n')
    check(strip, tmp_path / 'filtered', extra=['--filter-images-path', tmp_path / 'filter.txt'])
    part, seven_names, listed = seven(strip, tmp_path)
    check(strip, tmp_path / 'skipped', targets=listed, restored=part)
    assert rows_equal_the_baselines(strip, tmp_path / 'filtered', seven_names) > 0
    for name in seven_names:
        for ext in ('pt', 'png'):
            f = f'{Path(name).stem}_consistency.{ext}'
            same_file(tmp_path / 'filtered' / f, tmp_path / 'skipped' / f)
    # --image-name: one target, its baseline files, a consistency.pt of that target alone
    check(strip, tmp_path / 'one', targets=['--image-name', names[4]])
    assert files_of(tmp_path / 'one') == sorted(target_files([names[4]]) + ['consistency.pt'])
    for f in target_files([names[4]]):
        same_file(tmp_path / 'one' / f, baseline / f)
    one = torch.load(tmp_path / 'one' / 'consistency.pt')
    rows = [i for i, p in enumerate(pairs(b)) if p[0] == names[4]]
    assert one['targets'] == [names[4]] and pairs(one) == [pairs(b)[i] for i in rows] and len(rows) == 4
    assert same_bits(one['n'], b['n'][rows]) and same_bits(one['rms_restored'], b['rms_restored'][rows])
