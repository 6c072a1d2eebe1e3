"""GPU tests of the cross-view consistency check (sucre_view_consistency, engine.view_consistency, --check-consistency).

The yardstick is tests/consistency_ref.py, a float64 numpy restatement evaluated on the matches ``Restoration.match_map``
returns: the matched and the valid sets, ``count`` and the two pair counts must agree exactly; each of the 24 float sums of a
view within 2^-15 of the sum of its terms' magnitudes (a 256-term float32 accumulation has gamma = 256 x 2^-24 = 2^-16, and
the float32 difference and square double it); ``ssd`` within n_views x 2^-23 relative (one fmaf per view).
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import consistency_ref as ref
from sucre_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_CASES = {}


def restored_like(view, seed, force_nan_at=None):
    """Random float32 in (0, 1) with a NaN in ONE channel of about 5 % of the pixels."""
    H, W = view.depth.shape
    g = torch.Generator().manual_seed(seed)
    J = torch.rand((H, W, 3), generator=g) * 0.98 + 0.01
    hit = torch.rand((H, W), generator=g) < 0.05
    ch = torch.randint(0, 3, (H, W), generator=g)
    if force_nan_at is not None:
        hit[force_nan_at] = True
    vv, uu = torch.nonzero(hit, as_tuple=True)
    J[vv, uu, ch[vv, uu]] = float('nan')
    assert bool((torch.isnan(J).sum(dim=2) == 1).any()) and not bool((torch.isnan(J).sum(dim=2) > 1).any())
    return J.to(DEV)


def other_size_view(scene, width=48, height=32):
    """A camera of its own (48x32, its own K) next to the target, rendered against the same seabed."""
    tgt = scene.views[scene.target]
    fxy = 0.78 * width
    K = torch.tensor([[fxy, 0.0, width / 2.0], [0.0, fxy, height / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    t = tgt.t + torch.tensor([[0.05], [-0.03], [0.1]])
    depth_mm, rgb = synth.render_view(K, tgt.R.double().numpy(), t.double().numpy().ravel(), width, height, view_id=77,
                                      seed=scene.seed, relief=0.15, invalid_frac=0.01)
    depth = (depth_mm.to(torch.float64) / 1000.0).to(torch.float32)
    return engine.DeviceView(depth=depth.to(DEV).contiguous(), rgb=rgb.to(DEV).contiguous(), K=K, R=tgt.R, t=t, name='other_48x32.png')


def case(key):
    """(target, J_A, views, Js, maps, reference) -- made once and never changed.  '37x21': partial tiles on both axes, 3x2 tiles;
    four neighbours, a far view that matches nothing, a view of another size, a view without a restored image (NULL), and a
    view given with float32 colours (no raw comparison).  '96x64': the plain scene the survey figures of the README quote."""
    if key not in _CASES:
        if key == '37x21':
            scene = synth.make_scene(37, 21, 4, seed=3, far_views=1)
        else:
            scene = synth.make_scene(96, 64, 6)
        dv = engine.device_views_from_scene(scene, DEV)
        target = dv[scene.target]
        views = [v for i, v in enumerate(dv) if i != scene.target]
        if key == '37x21':
            views.append(other_size_view(scene))
            views.append(views[0].as_float_colour())
        H, W = target.depth.shape
        plain = [v if v.rgb.dtype == torch.uint8 else views[0] for v in views]   # (the same pixels: the matcher reads no colour here)
        r = engine.Restoration(H, W, len(views), device=DEV)
        r.match(target, plain, packed=False)
        maps = [r.match_map(k).cpu().numpy() for k in range(len(views))]
        lists = [ref.lists_of_map(m, v.depth.shape[1]) for m, v in zip(maps, views)]
        u1, v1 = lists[0][0], lists[0][1]
        assert len(u1) > 0
        J_A = restored_like(target, 100, force_nan_at=(int(v1[len(v1) // 2]), int(u1[len(u1) // 2])))
        Js = [restored_like(v, 200 + k) for k, v in enumerate(views)]
        if key == '37x21':
            Js[1] = None
        rgb_of = lambda v: v.rgb.cpu().numpy() if v.rgb.dtype == torch.uint8 else None   # noqa: E731
        want = ref.reference(J_A.cpu().numpy(), rgb_of(target),
                             [(l, None if J is None else J.cpu().numpy(), rgb_of(v)) for l, J, v in zip(lists, Js, views)])
        _CASES[key] = (target, J_A, views, Js, maps, want)
    return _CASES[key]


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_against_reference(key):
    target, J_A, views, Js, maps, (count64, ssd64, stats64, stats_abs, valids) = case(key)
    count, ssd, stats = (x.cpu().numpy() for x in engine.view_consistency(target, J_A, views, Js))
    n_views = len(views)
    assert count.dtype == np.int32 and ssd.dtype == np.float32 and stats.dtype == np.float64 and stats.shape == (n_views, 26)
    # the matches are match_map's, the valid pairs the reference's: exactly
    for k, m in enumerate(maps):
        assert stats[k, 0] == (0 if Js[k] is None else int((m >= 0).sum())), k
    assert np.array_equal(stats[:, 1], stats64[:, 1]) and np.array_equal(stats[:, 0], stats64[:, 0])
    assert np.array_equal(count, count64)
    # the 24 sums of every view
    err = np.abs(stats[:, 2:] - stats64[:, 2:])
    bar = 2.0 ** -15 * stats_abs[:, 2:]
    worst = (err / np.where(bar > 0, bar, 1.0)).max()
    print(f'{key}: largest |sum - sum64| / (2^-15 sum |term|) = {worst:.3e} over {n_views} views, pairs per view {stats[:, 1].astype(int).tolist()}')
    assert (err <= bar).all(), (key, np.argwhere(err > bar)[:5], worst)
    # the per-pixel sums
    assert np.array_equal(ssd[count64 == 0], np.zeros_like(ssd[count64 == 0]))
    rel = np.abs(ssd - ssd64)
    worst_px = (rel / np.where(ssd64 > 0, ssd64, 1.0)).max()
    print(f'{key}: largest |ssd - ssd64| / ssd64 = {worst_px:.3e}, bar {n_views * 2.0 ** -23:.3e}')
    assert (rel <= n_views * 2.0 ** -23 * ssd64).all()
    return stats, stats64, valids


def test_against_the_numpy_reference():
    target, J_A, views, Js, maps, _ = case('37x21')
    stats, stats64, valids = check_against_reference('37x21')
    names = [v.name for v in views]
    # the scene holds what it was built for
    matches = [int((m >= 0).sum()) for m in maps]
    assert sum(1 for n in matches if n == 0) == 1, matches          # the far view
    far = matches.index(0)
    assert Js[far] is not None and np.array_equal(stats[far], np.zeros(26))
    assert Js[1] is None and matches[1] > 0 and np.array_equal(stats[1], np.zeros(26))   # no restored image: no part, whatever it matches
    other = names.index('other_48x32.png')
    assert tuple(views[other].depth.shape) == (32, 48) and stats[other, 1] > 100
    # a pixel that is NaN in one channel only makes its pairs invalid, in every view
    assert all(v is None or (0 < v.sum() < len(v)) for k, v in enumerate(valids) if matches[k] > 0)
    # float32 colours: no raw comparison, the J sums as for the same pixels with uint8 colours ... of another restored image, so
    # only the match count and the zeros are pinned here
    assert views[-1].rgb.dtype == torch.float32 and stats[-1, 0] == stats[0, 0] and np.array_equal(stats[-1, 14:], np.zeros(12))
    assert (stats[0, 14:17] > 0).all() and (stats[-1, 2:5] > 0).all()


def test_plain_scene_agrees_with_the_reference():
    """make_scene(96, 64, 6): the raw pictures agree better than the restored ones there (all cameras at one altitude; the
    restoration amplifies the quantisation of the uint8 colours) -- a property of the scene.  Only agreement is asserted."""
    check_against_reference('96x64')


def test_two_calls_give_the_same_bits():
    target, J_A, views, Js, _, _ = case('37x21')
    a = engine.view_consistency(target, J_A, views, Js)
    b = engine.view_consistency(target, J_A, views, Js)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert same_bits(x, y)


def abi_call(target, J_A, views, Js, fill, **bad):
    """Straight on the C ABI, outputs and scratch pre-filled with ``fill``."""
    lib = _lib.load()
    n = len(views)
    H, W = target.depth.shape
    table = (_lib.SucreView * n)(*[v.to_struct() for v in views])
    ptrs = (C.c_void_p * n)(*[None if J is None else J.data_ptr() for J in Js])
    staged = torch.frombuffer(bytearray(bytes(table) + bytes(ptrs)), dtype=torch.uint8).to(DEV)
    count = torch.empty((H, W), dtype=torch.int32, device=DEV)
    ssd = torch.empty((H, W, 3), dtype=torch.float32, device=DEV)
    stats = torch.empty((n, 26), dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib.sucre_consistency_scratch_bytes(H, W, n), dtype=torch.uint8, device=DEV)
    for t in (count, ssd, stats, scratch):
        t.view(torch.uint8).fill_(fill)
    tgt = target.to_struct()
    with torch.cuda.device(DEV):
        rc = lib.sucre_view_consistency(H, W, bad.get('n', n), C.byref(tgt), C.c_void_p(staged.data_ptr()), C.c_void_p(J_A.data_ptr()),
                                        C.c_void_p(staged.data_ptr() + C.sizeof(table)), C.c_void_p(count.data_ptr()),
                                        C.c_void_p(ssd.data_ptr() + bad.get('ssd_offset', 0)), C.c_void_p(stats.data_ptr()),
                                        C.c_void_p(scratch.data_ptr()), engine._stream_ptr())
    torch.cuda.synchronize()
    return rc, count, ssd, stats


def test_dirty_outputs_come_back_fully_written():
    target, J_A, views, Js, _, _ = case('37x21')
    views = views[:-1]   # (the ABI takes uint8 colours or none)
    Js = Js[:-1]
    want = engine.view_consistency(target, J_A, views, Js)
    for fill in (0xFF, 0x00):
        rc, count, ssd, stats = abi_call(target, J_A, views, Js, fill)
        assert rc == 0
        for x, y in zip(want, (count, ssd, stats)):
            assert same_bits(x, y), fill


def test_one_view():
    target, J_A, views, Js, maps, (count64, ssd64, stats64, _, _) = case('37x21')
    full = engine.view_consistency(target, J_A, views, Js)[2]
    for k in (0, len(views) - 2):   # a neighbour, and the view of another size
        count, ssd, stats = engine.view_consistency(target, J_A, [views[k]], [Js[k]])
        assert tuple(stats.shape) == (1, 26) and same_bits(stats[0], full[k])
        assert int(count.sum()) == int(stats64[k, 1]) and int(count.max()) == 1
        one = ref.reference(J_A.cpu().numpy(), target.rgb.cpu().numpy(),
                            [(ref.lists_of_map(maps[k], views[k].depth.shape[1]), Js[k].cpu().numpy(), views[k].rgb.cpu().numpy())])
        assert np.array_equal(count.cpu().numpy(), one[0])
        # one view, one fmaf from zero: the float32 square of the float32 difference -- 2 x 2^-24 from the difference, 2^-24 from
        # the rounding of the square, 1.5 x 2^-23 together, within 2^-22
        assert (np.abs(ssd.cpu().numpy() - one[1]) <= 2.0 ** -22 * one[1]).all()


def test_validation_returns_before_any_launch():
    target, J_A, views, Js, _, _ = case('37x21')
    lib = _lib.load()
    for bad, code, word in ((dict(n=0), -2, b'n_views'), (dict(n=4097), -2, b'n_views'), (dict(ssd_offset=4), -1, b'16-byte aligned')):
        rc, count, ssd, stats = abi_call(target, J_A, views[:2], Js[:2], 0xFF, **bad)
        assert rc == code and word in lib.sucre_last_error(), bad
        for t in (count, ssd, stats):   # nothing ran
            assert bool((t.view(torch.uint8) == 0xFF).all()), bad


# ---- the command line: restore a survey with --apply-water, then check it -------------------------------------------------------
@pytest.fixture(scope='module')
def checked_survey(tmp_path_factory):
    """make_deep_scene(96, 64, 6) on disk, restored with the TRUE water of the renderer, then checked."""
    import contextlib
    import io
    import os
    from sucre_amd import sucre
    root = tmp_path_factory.mktemp('consistency_scene')
    scene = synth.make_deep_scene(96, 64, 6)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored, checked = root / 'restored', root / 'checked'
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            sucre.main(base + ['--output-dir', str(checked), '--check-consistency', str(restored), '--num-iter', '3'])
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, scene, restored, checked, printed.getvalue()


def test_cli_files_and_lines(checked_survey):
    root, scene, restored, checked, printed = checked_survey
    stems = [Path(n).stem for n in scene.names]
    assert sorted(p.name for p in checked.iterdir()) == sorted([f'{s}_consistency.pt' for s in stems] + [f'{s}_consistency.png' for s in stems]
                                                               + ['consistency.pt'])
    assert '--check-consistency' in printed and 'ignored' in printed and 'Solve least squares' not in printed
    for name in scene.names:
        assert f'{name}: consistency with ' in printed and ' pixel pairs: restored RMS R ' in printed and '(raw R ' in printed
    assert 'least consistent with img_' in printed
    merged = torch.load(checked / 'consistency.pt')
    assert f'consistency over {len(merged["a"])} pairs of {len(scene.names)} images: restored RMS' in printed
    assert merged['images'] == scene.names and len(merged['a']) == len(merged['b']) == int(merged['n'].numel()) > len(scene.names)
    assert all(k in merged for k in ('rms_restored', 'rms_raw', 'gain', 'rms_restored_gain', 'pooled_restored', 'pooled_raw'))
    from PIL import Image as PILImage
    from sucre_amd import sucre
    got = torch.load(checked / f'{stems[0]}_consistency.pt')
    assert all(k in got for k in ('views', 'stats', 'kept', 'count', 'ssd', 'min_cover', 'rms_restored', 'rms_raw', 'gain', 'rms_restored_gain'))
    assert np.array_equal(np.asarray(PILImage.open(checked / f'{stems[0]}_consistency.png')),
                          sucre.residual_image(got['count'].numpy(), got['ssd'].numpy()))


def test_cli_stats_are_the_engines_bits(checked_survey):
    from sucre_amd import sfm
    root, scene, restored, checked, _ = checked_survey
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    for name in scene.names:
        got = torch.load(checked / f'{Path(name).stem}_consistency.pt')
        assert name not in got['views'] and len(got['views']) >= 1
        J = lambda n: torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV)   # noqa: E731
        count, ssd, stats = engine.view_consistency(model[name].device_view(DEV), J(name), [model[n].device_view(DEV) for n in got['views']],
                                                    [J(n) for n in got['views']])
        assert same_bits(got['stats'], stats) and same_bits(got['count'], count) and same_bits(got['ssd'], ssd), name


def test_restoration_makes_the_deep_scene_more_consistent(checked_survey):
    """Ranges from 0.7 m to 8 m: the raw colours of one seabed point differ from camera to camera, the restored ones should
    not.  A float64 inversion on the oracle's matches gives margins of 1.6, 4.3 and 2.5 (R, G, B); the inequality is asserted."""
    root, scene, restored, checked, _ = checked_survey
    got = torch.load(checked / f'{Path(scene.names[scene.target]).stem}_consistency.pt')
    r, raw = got['pooled_restored'].numpy(), got['pooled_raw'].numpy()
    print(f'pooled RMS of the target over {got["pooled_n"]} pairs: restored {r}, raw {raw}, ratio {raw / r}')
    assert got['pooled_n'] > 1000 and (r < raw).all(), (r, raw)
