"""CPU tier of the cross-view consistency check: the --check-consistency flag and the combinations refused before any file is
opened, consistency_summary against direct numpy on hand-made rows, the survey merge under every split over ranks, the
refusal of a missing or mis-shaped restored image before anything is decoded, and the library's argument validation (nothing
is launched)."""
import builtins
import ctypes as C
import io
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sucre_amd import _lib, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def test_flag_lives_in_extras_and_leaves_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'check_consistency' not in vars(off)
    on = p.parse_args(BASE + ['--check-consistency', 'results'])
    assert str(on.check_consistency) == 'results'
    assert vars(off) == {k: v for k, v in vars(on).items() if k != 'check_consistency'}
    assert all(a.dest != 'check_consistency' for a in p._actions)
    assert any(a.dest == 'check_consistency' and a.default is sucre.argparse.SUPPRESS for a in p.extras._actions)
    assert '--check-consistency DIR' in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ['--check-consistency'])


REFUSED = [(['--shared-water'], '--shared-water'), (['--apply-water', 'w.pt'], '--apply-water'), (['--trim-outliers', '3'], '--trim-outliers'),
           (['--trim-rounds', '2'], '--trim-outliers'), (['--view-gains'], '--view-gains'), (['--gain-rounds', '2'], '--view-gains'),
           (['--gain-limit', '3'], '--view-gains'), (['--save-quality'], '--save-quality'), (['--save-interval', '5'], '--save-interval'),
           (['--params-path', 'p.pt'], '--params-path'), (['--keep-matches'], '--keep-matches'), (['--common-stretch'], '--common-stretch'),
           (['--stretch-from', 's.pt'], '--stretch-from'), (['--image-scale', '0.5'], '--image-scale')]


@pytest.mark.parametrize('extra, named', REFUSED, ids=[' '.join(e) for e, _ in REFUSED])
def test_refusals_name_both_flags_before_any_file_is_opened(extra, named, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    opened = []
    real_open = builtins.open
    spy = lambda *a, **k: (opened.append(a[0]), real_open(*a, **k))[1]   # noqa: E731
    monkeypatch.setattr(builtins, 'open', spy)
    monkeypatch.setattr(io, 'open', spy)   # (pathlib's read_text / open)
    monkeypatch.setattr(torch, 'load', lambda *a, **k: opened.append(a[0]))
    out = tmp_path / 'out'
    argv = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
            '--output-dir', str(out), '--image-name', 'x.png', '--check-consistency', str(tmp_path / 'results')] + extra
    with pytest.raises(SystemExit) as e:
        sucre.main(argv)
    assert e.value.code != 0 and '--check-consistency' in str(e.value.code) and named in str(e.value.code)
    assert not opened and not out.exists()


def hand_made_stats():
    """Five views of a 10x8 target: an ordinary one, one below min_cover, one with matches but no valid pair, one whose b is zero
    throughout, one that is a pure gain of the target."""
    rng = np.random.default_rng(5)
    rows = np.zeros((5, 26))

    def fill(k, matches, a, b, ra, rb):
        rows[k, 0], rows[k, 1] = matches, len(a)
        for o, (x, y) in ((2, (a, b)), (14, (ra, rb))):
            d = x - y
            rows[k, o:o + 12] = np.concatenate([(d * d).sum(0), (x * x).sum(0), (y * y).sum(0), (x * y).sum(0)])
        return a, b, ra, rb

    data = [fill(0, 40, rng.random((33, 3)), rng.random((33, 3)), rng.random((33, 3)), rng.random((33, 3))),
            fill(1, 2, rng.random((2, 3)), rng.random((2, 3)), rng.random((2, 3)), rng.random((2, 3))),
            fill(2, 17, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))),
            fill(3, 30, rng.random((30, 3)), np.zeros((30, 3)), rng.random((30, 3)), rng.random((30, 3)))]
    b = rng.random((25, 3))
    data.append(fill(4, 25, b * np.array([1.5, 0.5, 2.0]), b, b, b))
    return rows, data


def test_summary_against_direct_numpy():
    rows, data = hand_made_stats()
    H, W, min_cover = 8, 10, 0.03   # a view needs more than 2.4 matches
    s = sucre.consistency_summary(rows, H, W, min_cover)
    assert s['kept'].tolist() == [True, False, True, True, True]
    assert s['n'].tolist() == [33, 2, 0, 30, 25] and s['n_matches'].tolist() == [40, 2, 17, 30, 25]
    for k, (a, b, ra, rb) in enumerate(data):
        n = len(a)
        if n == 0:
            for key in ('rms_restored', 'rms_raw', 'rms_restored_gain'):
                assert np.array_equal(s[key][k], np.zeros(3)), key
            assert np.array_equal(s['gain'][k], np.ones(3))
            continue
        np.testing.assert_allclose(s['rms_restored'][k], np.sqrt(((a - b) ** 2).mean(0)), rtol=1e-12)
        np.testing.assert_allclose(s['rms_raw'][k], np.sqrt(((ra - rb) ** 2).mean(0)), rtol=1e-12)
        if (b * b).sum() > 0:
            g = (a * b).sum(0) / (b * b).sum(0)
            np.testing.assert_allclose(s['gain'][k], g, rtol=1e-12)
            np.testing.assert_allclose(s['rms_restored_gain'][k], np.sqrt(((a - g * b) ** 2).mean(0)), rtol=1e-9, atol=1e-7)
        else:   # sum b^2 = 0: gain 1, and nothing a gain could remove
            assert np.array_equal(s['gain'][k], np.ones(3))
            np.testing.assert_allclose(s['rms_restored_gain'][k], np.sqrt((a * a).mean(0)), rtol=1e-12)
    # the pure gain: a large difference that a gain removes entirely
    assert s['rms_restored'][4].min() > 0.1 and s['rms_restored_gain'][4].max() < 1e-7
    np.testing.assert_allclose(s['gain'][4], [1.5, 0.5, 2.0], rtol=1e-12)
    # pooled over the KEPT views only
    kept = [0, 2, 3, 4]
    n = sum(len(data[k][0]) for k in kept)
    assert s['pooled_n'] == n == 88
    np.testing.assert_allclose(s['pooled_restored'], np.sqrt(sum(((data[k][0] - data[k][1]) ** 2).sum(0) for k in kept) / n), rtol=1e-12)
    np.testing.assert_allclose(s['pooled_raw'], np.sqrt(sum(((data[k][2] - data[k][3]) ** 2).sum(0) for k in kept) / n), rtol=1e-12)
    # nothing kept: zeros, no division by zero
    none = sucre.consistency_summary(rows, H, W, 1.0)
    assert not none['kept'].any() and none['pooled_n'] == 0 and np.array_equal(none['pooled_restored'], np.zeros(3))
    # the cover rule is strict, as sfm.py:136's
    assert sucre.consistency_summary(rows, H, W, 2 / 80)['kept'].tolist() == [True, False, True, True, True]
    assert sucre.consistency_summary(rows, H, W, np.nextafter(2 / 80, 0))['kept'].tolist() == [True] * 5


def records_of_a_survey():
    rows, _ = hand_made_stats()
    names = [f'img_{i:04d}.png' for i in range(6)]
    rng = np.random.default_rng(11)
    records = []
    for i, name in enumerate(names):
        views = [n for n in names if n != name]
        stats = rows[rng.permutation(5)].copy()
        stats[:, 2:] *= 1 + i   # (the sums only: matches and pairs stay whole numbers)
        records.append({'target': name, 'views': views, 'stats': stats, 'H': 8, 'W': 10})
    return names, records


def same_merge(a, b):
    assert list(a) == list(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_merge_does_not_depend_on_the_split_over_ranks():
    names, records = records_of_a_survey()
    whole = sucre.merge_consistency(records, names, 0.03)
    assert whole['images'] == names and whole['targets'] == names
    # one row per directed kept pair with a valid pixel pair: three of the five views of every target
    assert len(whole['a']) == len(whole['b']) == 18 and whole['n'].dtype == torch.int64 and tuple(whole['rms_restored'].shape) == (18, 3)
    assert all(x != y for x, y in zip(whole['a'], whole['b']))
    for world in (2, 3, 4, 6):
        from sucre_amd import dist
        parts = [dist.shard_images(records, rank, world) for rank in range(world)]
        gathered = [r for part in parts for r in part]
        same_merge(whole, sucre.merge_consistency(gathered, names, 0.03))
        same_merge(whole, sucre.merge_consistency([r for part in reversed(parts) for r in part], names, 0.03))
    for perm in itertools.islice(itertools.permutations(records), 0, 720, 97):
        same_merge(whole, sucre.merge_consistency(list(perm), names, 0.03))
    # the pooled figures are those of all rows together
    total = sum(int(round(r['stats'][k, 1])) for r in records for k in range(5) if r['stats'][k, 0] / 80 > 0.03)
    assert whole['pooled_n'] == total == int(whole['n'].sum())
    sd = sum(r['stats'][k, 2:5] for r in records for k in range(5) if r['stats'][k, 0] / 80 > 0.03 and r['stats'][k, 1] > 0)
    np.testing.assert_allclose(whole['pooled_restored'].numpy(), np.sqrt(sd / total), rtol=1e-12)


def fake_image(name, H=6, W=8):
    return SimpleNamespace(name=name, camera=SimpleNamespace(height=H, width=W))


def test_missing_or_misshaped_target_is_refused_before_any_image_is_opened(tmp_path, monkeypatch):
    from sucre_amd import loader
    touched = []
    for fn in ('_imread_rgb_u8', '_imread_depth_u16', 'prefetch_for_targets', 'prefetch_device_views'):
        monkeypatch.setattr(loader, fn, lambda *a, **k: touched.append(a))
    results, out = tmp_path / 'results', tmp_path / 'out'
    results.mkdir()
    a, b = fake_image('a.png'), fake_image('b.png')
    torch.save({'J': torch.zeros(6, 8, 3)}, results / 'a.pt')
    with pytest.raises(SystemExit) as e:
        sucre.check_consistency([a, b], None, results, out, image_list=[a, b])
    assert '--check-consistency' in str(e.value.code) and 'b.pt' in str(e.value.code) and 'missing' in str(e.value.code)
    # a target of another shape than its camera
    torch.save({'J': torch.zeros(8, 6, 3)}, results / 'b.pt')
    with pytest.raises(SystemExit) as e:
        sucre.check_consistency([a, b], None, results, out, image_list=[a, b])
    assert 'b.pt' in str(e.value.code) and '(6, 8, 3)' in str(e.value.code) and '(8, 6, 3)' in str(e.value.code)
    # ... and a NEIGHBOUR of another shape, and a file without J
    c = fake_image('c.png')
    torch.save({'J': torch.zeros(6, 8, 3)}, results / 'b.pt')
    torch.save({'J': torch.zeros(6, 8)}, results / 'c.pt')
    with pytest.raises(SystemExit) as e:
        sucre.check_consistency([a], None, results, out, image_list=[a, b, c])
    assert 'c.pt' in str(e.value.code)
    torch.save({'B': torch.zeros(3, 1)}, results / 'c.pt')
    with pytest.raises(SystemExit) as e:
        sucre.check_consistency([a], None, results, out, image_list=[a, b, c])
    assert 'c.pt' in str(e.value.code) and 'J' in str(e.value.code)
    assert not touched and not out.exists()
    # there is no CPU path
    with pytest.raises(RuntimeError, match='no CPU path'):
        sucre.check_consistency([a], None, results, out, image_list=[a, b], device='cpu')


def view_struct(H=21, W=37):
    s = _lib.SucreView()
    s.depth, s.rgb, s.H, s.W = 4096, 8192, H, W
    return s


def test_library_validates_before_any_launch():
    """No device is needed: every call below returns before a kernel would be launched (the pointers are not memory)."""
    lib = _lib.load()
    assert 'sucre_view_consistency' in _lib.SIGNATURES and lib.sucre_version() == 2
    size = lib.sucre_consistency_scratch_bytes
    tiles = 3 * 2
    assert size(21, 37, 1) == tiles * 4 * (4 + 96) and size(21, 37, 5) == 5 * size(21, 37, 1)   # per wave of a tile: a count word, 24 sums
    for H, W, n in ((0, 37, 1), (21, 0, 1), (32768, 37, 1), (21, 32768, 1), (21, 37, 0), (21, 37, 4097), (-1, 37, 1)):
        assert size(H, W, n) == 0, (H, W, n)
    tgt = view_struct()
    p = lambda x: C.c_void_p(x)   # noqa: E731
    good = dict(H=21, W=37, n=2, target=C.byref(tgt), views=p(1 << 20), J=p(2 << 20), Js=p(3 << 20), count=p(4 << 20), ssd=p(5 << 20),
                stats=p(6 << 20), scratch=p(7 << 20))

    def call(**kw):
        a = {**good, **kw}
        return lib.sucre_view_consistency(a['H'], a['W'], a['n'], a['target'], a['views'], a['J'], a['Js'], a['count'], a['ssd'], a['stats'],
                                          a['scratch'], None)

    for key in ('target', 'views', 'J', 'Js', 'count', 'ssd', 'stats', 'scratch'):
        assert call(**{key: None}) == -1 and b'NULL' in lib.sucre_last_error(), key
    for key in ('count', 'ssd', 'stats', 'scratch'):
        assert call(**{key: p(good[key].value + 8)}) == -1 and b'16-byte aligned' in lib.sucre_last_error(), key
    for H, W in ((0, 37), (21, 0), (-4, 37), (32768, 37), (21, 32768)):
        assert call(H=H, W=W) == -1 and b'invalid image size' in lib.sucre_last_error(), (H, W)
    for n in (0, -1, 4097):
        assert call(n=n) == -2 and b'n_views' in lib.sucre_last_error(), n
    other = view_struct(H=20)
    assert call(target=C.byref(other)) == -1 and b'expected' in lib.sucre_last_error()
    no_depth = view_struct()
    no_depth.depth = None
    assert call(target=C.byref(no_depth)) == -1 and b'depth' in lib.sucre_last_error()


def test_engine_entry_point_refuses_on_the_host():
    from sucre_amd import engine
    v = engine.DeviceView(depth=torch.ones(2, 2), rgb=torch.zeros(2, 2, 3, dtype=torch.uint8), K=torch.eye(3), R=torch.eye(3), t=torch.zeros(3, 1))
    J = torch.zeros(2, 2, 3)
    with pytest.raises(ValueError, match='1..4096'):
        engine.view_consistency(v, J, [], [])
    with pytest.raises(ValueError, match='restored images'):
        engine.view_consistency(v, J, [v, v], [J])
    with pytest.raises(_lib.SucreError, match='no CPU fallback'):
        engine.view_consistency(v, J, [v], [J])


# ---- _RestoredCache on the host: what --check-consistency keeps on the device across targets ------------------------------------
def cache_with_files(tmp_path, monkeypatch, sizes, budget):
    """One restored image per (H, W) of ``sizes`` -- J filled with the image's index, so a tensor names its file --, a cache of
    ``budget`` bytes on the CPU, and the list the non-lazy ``_read_restored`` calls append their file name to."""
    images = [fake_image(f'im{k}.png', H, W) for k, (H, W) in enumerate(sizes)]
    for k, im in enumerate(images):
        torch.save({'J': torch.full((im.camera.height, im.camera.width, 3), float(k))}, (tmp_path / im.name).with_suffix('.pt'))
    reads = []
    real = sucre._read_restored

    def spy(path, image, lazy=False):
        if not lazy:
            reads.append(path.name)
        return real(path, image, lazy)

    monkeypatch.setattr(sucre, '_read_restored', spy)
    return images, sucre._RestoredCache(tmp_path, 'cpu', budget), reads


def held(cache):
    """The names the cache holds, least recently used first, after checking its byte count against what it holds."""
    assert cache.total == sum(J.numel() * J.element_size() for J in cache.entries.values())
    return list(cache.entries)


def test_cache_hit_moves_the_entry_to_the_end_and_reads_nothing(tmp_path, monkeypatch):
    images, cache, reads = cache_with_files(tmp_path, monkeypatch, [(6, 8)] * 3, 3 * 6 * 8 * 12)
    assert cache.nbytes(images[0]) == 6 * 8 * 12
    first = [cache.get(im, set()) for im in images]
    assert reads == ['im0.pt', 'im1.pt', 'im2.pt'] and held(cache) == ['im0.png', 'im1.png', 'im2.png']
    assert all(J.dtype == torch.float32 and tuple(J.shape) == (6, 8, 3) and bool((J == k).all()) for k, J in enumerate(first))
    again = cache.get(images[0], set())
    assert again is first[0] and len(reads) == 3 and held(cache) == ['im1.png', 'im2.png', 'im0.png']
    assert cache.get(images[2], {'im1.png'}) is first[2] and len(reads) == 3 and held(cache) == ['im1.png', 'im0.png', 'im2.png']
    assert cache.total == 3 * 6 * 8 * 12 == cache.budget


def test_cache_evicts_least_recently_used_first_skips_pinned_and_stops_when_the_image_fits(tmp_path, monkeypatch):
    unit = 4 * 4 * 12
    #          im0     im1     im2     im3     im4 (2 units)  im5 (3 units)  im6
    sizes = [(4, 4), (4, 4), (4, 4), (4, 4), (8, 4),        (4, 12),       (4, 4)]
    images, cache, reads = cache_with_files(tmp_path, monkeypatch, sizes, 4 * unit)
    for im in images[:4]:
        cache.get(im, set())
    assert held(cache) == ['im0.png', 'im1.png', 'im2.png', 'im3.png'] and cache.total == 4 * unit
    cache.get(images[0], set())                                  # im0 becomes the most recently used
    assert held(cache) == ['im1.png', 'im2.png', 'im3.png', 'im0.png']
    # two units wanted: the two least recently used go, no more
    J4 = cache.get(images[4], set())
    assert held(cache) == ['im3.png', 'im0.png', 'im4.png'] and cache.total == 4 * unit and bool((J4 == 4).all())
    # one unit wanted, the least recently used pinned: the next one goes, and only that one
    cache.get(images[1], {'im3.png', 'im1.png'})
    assert held(cache) == ['im3.png', 'im4.png', 'im1.png'] and cache.total == 4 * unit
    # three units wanted, im4 (two units) pinned: both others go -- images of different sizes leave, the count follows
    J5 = cache.get(images[5], {'im4.png', 'im5.png'})
    assert held(cache) == ['im4.png', 'im5.png'] and cache.total == 5 * unit and bool((J5 == 5).all())   # (the pinned pair exceeds the budget)
    # one unit wanted, nothing pinned: im4 alone does not make room (3 + 1 = 4 fits after it), so im5 stays
    cache.get(images[6], {'im6.png'})
    assert held(cache) == ['im5.png', 'im6.png'] and cache.total == 4 * unit
    # an evicted image is read again, and is the right one
    n = len(reads)
    J0 = cache.get(images[0], {'im0.png', 'im6.png'})
    assert reads[n:] == ['im0.pt'] and bool((J0 == 0).all()) and held(cache) == ['im6.png', 'im0.png'] and cache.total == 2 * unit
    assert reads == ['im0.pt', 'im1.pt', 'im2.pt', 'im3.pt', 'im4.pt', 'im1.pt', 'im5.pt', 'im6.pt', 'im0.pt']


def test_cache_with_a_pinned_set_that_fills_the_budget_evicts_nothing(tmp_path, monkeypatch):
    unit = 6 * 8 * 12
    images, cache, reads = cache_with_files(tmp_path, monkeypatch, [(6, 8)] * 4, 3 * unit)
    pinned = {im.name for im in images[:3]}
    got = [cache.get(im, pinned) for im in images[:3]]
    assert cache.total == cache.budget and held(cache) == ['im0.png', 'im1.png', 'im2.png']
    # a fourth image while all three are pinned: nothing can go; the cache grows past its budget rather than hand out a wrong J
    J3 = cache.get(images[3], pinned | {'im3.png'})
    assert held(cache) == ['im0.png', 'im1.png', 'im2.png', 'im3.png'] and cache.total == 4 * unit and bool((J3 == 3).all())
    for k, im in enumerate(images[:3]):
        J = cache.get(im, pinned)
        assert J is got[k] and bool((J == k).all()), im.name
    assert reads == ['im0.pt', 'im1.pt', 'im2.pt', 'im3.pt']
    # the next target pins other names: the budget holds again as soon as something may go
    cache.get(images[3], {'im3.png'})
    J0 = cache.get(images[0], {'im3.png', 'im0.png'})
    assert J0 is got[0] and len(reads) == 4   # (a hit evicts nothing)
    assert held(cache) == ['im1.png', 'im2.png', 'im3.png', 'im0.png']


# ---- the overlap cull on the neighbour lists --check-consistency asks about ----------------------------------------------------
def test_overlap_cull_answers_for_the_list_it_is_given_not_for_a_look_alike():
    """check_consistency asks ``overlapping_views`` about another list for every target: the images with a restored image but
    the target.  Two such lists can share their length and their first, middle and last image -- of the strip of eight without
    image 3, the lists of targets 1 and 2 do -- and are still different lists: each must get its own answer (the camera stacks
    kept from the previous question were once taken for the look-alike's, and target 4 got image 1 for a neighbour)."""
    from pathlib import Path
    from sucre_amd import sfm, synth
    survey = synth.make_survey(96, 64, 8, 1, seed=5, spacing=0.5)
    images = [sfm.Image(i + 1, Path(v.name), Path('depth_' + v.name), sfm.Pose(v.R, v.t), sfm.Camera(i + 1, 96, 64, survey.K))
              for i, v in enumerate(survey.views)]
    for im, v in zip(images, survey.views):
        d = v.depth_f32()
        im.__dict__['_depth_range'] = (float(d[d > 0].min()), float(d[d > 0].max()))
    have = [im for im in images if im.name != 'img_0003.png']
    lists = {im.name: [o for o in have if o is not im] for im in have}
    a, b = lists['img_0001.png'], lists['img_0002.png']
    assert len(a) == len(b) and a[0] is b[0] and a[-1] is b[-1] and a[len(a) // 2] is b[len(b) // 2] and a[1] is not b[1]
    whole = {}
    for im in have:   # one question about the whole list, the target taken out afterwards: what each list's answer must be
        whole[im.name] = [have[i].name for i in im.overlapping_views(have, 'cpu') if have[i] is not im]
    assert whole['img_0004.png'] == ['img_0002.png', 'img_0005.png', 'img_0006.png']
    assert [len(whole[im.name]) for im in have] == [2, 2, 3, 3, 3, 3, 2]   # (2, 3, 4, 4, 4, 4, 3, 2 with image 3: each of its four neighbours loses one)
    for im in have:   # in the order of a run, every answer with the previous list's stacks still kept
        others = lists[im.name]
        assert [others[i].name for i in im.overlapping_views(others, 'cpu')] == whole[im.name], im.name
    # the same list asked about again is still served from what was kept
    kept = sfm._STACKED['entry']
    have[-1].overlapping_views(lists[have[-1].name], 'cpu')
    assert sfm._STACKED['entry'] is kept
