"""The seabed mosaic, its blend and its hole filling (engine.mosaic_of, sucre.mosaic, --mosaic, --mosaic-blend, --mosaic-fill) off
their demo scenes: images of five sizes in one request -- smaller than a workgroup, smaller than a wave --, launch and table-set
boundaries between images of different sizes, general camera matrices next to pinhole ones in one launch, plane coordinates of
one sign, caller-given axes, grids one cell thin, depths and colours that are not numbers, and the command line on two cameras,
with a small cache, a fixed stretch, sub-requests, 33 images and ``J`` files written by a fit.

The yardsticks are the three CPU restatements (tests/mosaic_ref.py, mosaic_blend_ref.py, mosaic_fill_ref.py), each evaluated on
exactly the inputs the engine got; the bar is bit equality of the bounds, the grid size and every tensor.  The engine-level cases
and their expected results are built in tests/test_mosaic_variants_host.py, which also asserts -- without a GPU -- that each case
holds the edge it was chosen for; the same assertions run again here before the engine does.
"""
import contextlib
import copy
import io
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_blend_ref as bref
import mosaic_fill_ref as fref
import mosaic_ref as ref
import test_mosaic_variants_host as cases
from sucre_amd import engine, sucre, synth
from test_gpu_mosaic import DEV, host_view, same_bits
from test_mosaic_variants_host import BEST, BLEND, BLEND_FILLED, BLENDED, FILLED, made, measured

pytestmark = pytest.mark.gpu

ALL = BEST + BLENDED + FILLED + BLEND_FILLED


def on_device(c):
    """The case's views as DeviceViews (the very K, K^-1, R and t the restatements read) and its restored images, uploaded once."""
    def make():
        views = [engine.DeviceView(depth=v.depth.to(DEV).contiguous(), rgb=v.rgb.to(DEV).contiguous(), K=v.K, R=v.R, t=v.t, name=v.name, Kinv=v.Kinv)
                 for v in c.views]
        return views, [J.to(DEV).contiguous() for J in c.Js]
    return made(('device', id(c)), make)


def run(c, **how):
    views, Js = on_device(c)
    return engine.mosaic_of(views, Js, c.axes, c.gsd, bounds=c.bounds, blend=c.blend, fill=c.reach, **how)


def check(m, want, what, bounds=True):
    """Bounds, grid, levels and every tensor of the three stages against the restatements, bit for bit."""
    print(f'{what}: {measured(want)}')
    if bounds:
        assert m.bounds() == want['bounds'], (what, m.bounds(), want['bounds'])
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']), what
    assert m.fill_levels == want['L'], what
    got = m.result()
    assert set(got) == set(ALL)
    assert same_bits(m.acc, want['acc']), (what, 'acc', int((m.acc.cpu() != want['acc']).sum()))
    for k in ALL:
        assert same_bits(got[k], want[k]), (what, k, int((got[k].cpu().contiguous().view(torch.uint8) != want[k].contiguous().view(torch.uint8)).sum()))


def same_results(a, b, what):
    assert (a.Hm, a.Wm) == (b.Hm, b.Wm) and a.bounds() == b.bounds(), what
    assert same_bits(a.key, b.key) and same_bits(a.pix, b.pix) and same_bits(a.acc, b.acc), what
    for k in ALL:
        assert same_bits(a.result()[k], b.result()[k]), (what, k)


# ---- the engine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gsd_factor', [1.0, 0.25], ids=['default gsd', 'gsd / 4'])
def test_ten_images_of_five_sizes_in_one_launch(gsd_factor):
    cases.test_every_one_of_the_ten_images_wins_cells(gsd_factor)
    c, want = cases.the_ten(gsd_factor)
    m = run(c)
    check(m, want, f'ten images of five sizes, gsd {float(c.gsd):.4f} m')
    same_results(run(c, batch=3), m, 'in calls of three')          # calls that begin at images of different sizes: ordinals 3, 6, 9
    same_results(run(c, plain_atomic=True), m, 'plain atomics')


def test_thirty_five_images_across_two_launches_and_three_table_sets():
    cases.test_thirty_five_images_every_table_set_wins_and_copies_tie()
    c, want = cases.the_thirty_five()
    m = run(c, batch=35)       # one call per phase: launches of 32 and 3 images, table sets of 16, 16 and 3
    check(m, want, '35 images in one call')
    same_results(run(c, batch=7), m, 'in calls of seven')


@pytest.mark.parametrize('variant', ['all', 'some', 'tiny'])
def test_general_camera_matrices(variant):
    cases.test_a_skewed_camera_moves_a_bound_or_a_winner(variant)
    c, want = cases.the_skewed(variant)
    check(run(c), want, f'skewed K on {variant}')


def test_one_sided_plane_coordinates_and_caller_given_axes():
    cases.test_one_sided_plane_coordinates_and_a_turned_frame()
    for frame in ('default', 'turned'):
        c, want = cases.the_shifted(frame)
        check(run(c), want, f'shifted survey, {frame} frame')


@pytest.mark.parametrize('which', ['row', 'column'])
def test_a_grid_one_cell_thin(which):
    cases.test_a_grid_one_cell_thin(which)
    c, want = cases.the_thin(which)
    m = run(c)
    check(m, want, f'one {which}', bounds=False)
    assert min(m.Hm, m.Wm) == 1 and m.fill_levels == (max(m.Hm, m.Wm) - 1).bit_length()


def test_depths_that_are_not_numbers():
    """NaN, -1 and 0 do not take part; a subnormal depth is an ordinary pixel; a pixel at +inf takes part and its coordinates are
    not numbers: without bounds the request is refused, with bounds such a pixel has no cell -- the result is that of the same
    images with those depths set to 0."""
    cases.test_odd_depths_take_part_only_when_positive()
    c, clean, where, want = cases.the_odd_depths()
    views, Js = on_device(c)
    m = engine.Mosaic(c.axes, c.gsd, DEV)
    m.add_bounds(views, Js)
    with pytest.raises(ValueError, match='not finite'):
        m.begin(blend=c.blend)
    assert m.key is None and m.acc is None and m.grid is None
    check(run(c), want, 'odd depths, caller-given bounds', bounds=False)
    same_results(run(c, plain_atomic=True), run(c), 'plain atomics')


def test_infinities_in_the_restored_images():
    cases.test_infinite_colours_are_copied_clamped_and_left_out_of_the_fill()
    c, want = cases.the_infinite_colours()
    m = run(c)
    check(m, want, 'infinite colours')
    got = m.result()
    inf_cells = (got['source'] >= 0) & torch.isinf(got['J']).any(dim=2)
    assert int(inf_cells.sum()) > 0 and same_bits(got['J_filled'][inf_cells], got['J'][inf_cells])
    assert bool(torch.isfinite(got['J_blend'][got['source'] >= 0]).all())
    assert same_bits(got['fill_level'], want['fill_level']) and not torch.equal(want['fill_level'], want['blend_fill_level'])


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _main(argv):
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        sucre.main([str(a) for a in argv])
    return text.getvalue()


def _as_scene(survey):
    return synth.SynthScene(width=survey.width, height=survey.height, K=survey.K, views=list(survey.views))


def _write_water_and_stretch(root):
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    torch.save({'lo': torch.tensor([0.1, 0.15, 0.2]), 'hi': torch.tensor([0.8, 0.85, 0.9])}, root / 'stretch.pt')


def _base(root):
    return ['--image-dir', root / 'images', '--depth-dir', root / 'depth', '--model-dir', root / 'model']


def _quarter_gsd(model, names):
    views = [model[n].device_view(DEV) for n in names]
    return np.float32(sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views]) * np.float32(0.25))


@pytest.fixture(scope='module')
def cli(tmp_path_factory):
    """``mixed``: the six 96x64 images of the survey and three 47x33 images under a second camera in one model, restored with the
    true water; ``many``: a survey of 33 images of 24x16, restored the same way.  ``flags(root)``: what every mosaic run is given."""
    from sucre_amd import sfm
    from test_gpu_api import write_scene
    from test_gpu_stretch import _merge
    top = tmp_path_factory.mktemp('mosaic_variants')
    root_a, root_b, mixed, many = top / 'a', top / 'b', top / 'mixed', top / 'many'
    write_scene(_as_scene(synth.make_survey(96, 64, 3, 2)), root_a)
    small = synth.make_scene(47, 33, 2, seed=5)
    small.views = [copy.copy(v) for v in small.views]
    for v in small.views:
        v.name = 'b_' + v.name
    write_scene(small, root_b)
    mixed.mkdir()
    _merge(root_a, root_b, mixed)
    write_scene(_as_scene(synth.make_survey(24, 16, 11, 3, seed=2)), many)
    out = {'top': top}
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv('WORLD_SIZE', raising=False)
        for key, root, n in (('mixed', mixed, 9), ('many', many, 33)):
            _write_water_and_stretch(root)
            _main(_base(root) + ['--image-ids', 1, n + 1, '--output-dir', root / 'restored', '--apply-water', root / 'true_water.pt'])
            model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
            names = [model.images[i].name for i in range(1, n + 1)]
            gsd = _quarter_gsd(model, names)
            flags = ['--mosaic', root / 'restored', '--mosaic-gsd', repr(float(gsd)), '--mosaic-blend', BLEND, '--mosaic-fill', repr(cases.FILL_GSDS * float(gsd))]
            printed = _main(_base(root) + ['--image-ids', 1, n + 1, '--output-dir', root / 'all'] + flags)
            out[key] = SimpleNamespace(root=root, model=model, names=names, gsd=gsd, flags=flags, printed=printed, restored=root / 'restored')
    return out


def expected_of_files(model, names, restored, gsd):
    """The three restatements on what the files hold: images, depths and poses as the model loads them, ``J`` as torch.load reads it."""
    views = [host_view(model[n].device_view(DEV)) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'] for n in names]
    c = cases.case(views, Js, axes=sucre.mosaic_axes([model[n] for n in names]), gsd=gsd, reach=cases.FILL_GSDS * float(gsd))
    return c, cases.expected(c)


def check_file(got, want, names, what):
    """mosaic.pt against the restatements, and its bookkeeping against its tensors."""
    print(f'{what}: {measured(want)}')
    assert tuple(got['source'].shape) == (want['Hm'], want['Wm']) and tuple(got['lo'].tolist()) == want['bounds'][:2], what
    assert got['fill_levels'] == want['L'] and got['blend'] == float(np.float32(BLEND))
    for k in ALL:
        assert same_bits(got[k], want[k]), (what, k, int((got[k].contiguous().view(torch.uint8) != want[k].contiguous().view(torch.uint8)).sum()))
    n_filled = int((got['source'] >= 0).sum())
    assert got['images'] == list(names) and got['n_filled'] == n_filled and int(got['per_image'].sum()) == n_filled
    assert torch.equal(got['per_image'], torch.bincount(got['source'][got['source'] >= 0].long(), minlength=len(names)))


def png(path):
    from PIL import Image as PILImage
    return np.asarray(PILImage.open(path))


PICTURES = {'mosaic.png': 'J', 'mosaic_blend.png': 'J_blend', 'mosaic_filled.png': 'J_filled', 'mosaic_blend_filled.png': 'J_blend_filled'}
OTHER_PICTURES = ('mosaic_raw.png', 'mosaic_source.png', 'mosaic_blend_raw.png', 'mosaic_raw_filled.png', 'mosaic_blend_raw_filled.png', 'mosaic_filled_mask.png')


def same_tensors(a, b, what):
    assert set(a) == set(b), what
    for k, v in a.items():
        assert same_bits(v, b[k]) if torch.is_tensor(v) else v == b[k], (what, k)


def test_cli_two_cameras_equal_the_restatements(cli):
    s = cli['mixed']
    got = torch.load(s.root / 'all' / 'mosaic.pt')
    assert sorted(p.name for p in (s.root / 'all').iterdir()) == sorted(list(PICTURES) + list(OTHER_PICTURES) + ['mosaic.pt'])
    assert got['gsd'] == float(s.gsd) and len(s.names) == 9
    c, want = expected_of_files(s.model, s.names, s.restored, s.gsd)
    assert sorted({tuple(v.depth.shape) for v in c.views}) == [(33, 47), (64, 96)]
    assert not torch.equal(c.views[0].K, c.views[8].K)
    check_file(got, want, s.names, 'two cameras, nine images')
    won = set(cases.winners(want))
    assert won & set(range(6)) and won & {6, 7, 8}       # both sizes win cells
    assert cases.holes_close(want) and int((want['samples'] > 1).sum()) > 0
    # the three lines match the tensors
    Hm, Wm = got['source'].shape
    n_filled, per_image = got['n_filled'], got['per_image']
    top = int(per_image.argmax())
    lines = s.printed.splitlines()
    assert (f'mosaic of 9 images: {Wm} x {Hm} cells of {got["gsd"]:.6g} m, {n_filled} filled ({100.0 * n_filled / (Hm * Wm):.1f} %), {Hm * Wm - n_filled} empty; '
            f'largest share {s.names[top]} ({100.0 * int(per_image[top]) / n_filled:.1f} %)') in lines
    samples = got['samples'].long()
    total, most, several = int(samples.sum()), int(samples.max()), int((samples > 1).sum())
    assert (f'mosaic blend of depth {got["blend"]:.6g} m: {total} samples, {total / n_filled:.2f} per filled cell on average, '
            f'{most} at most; {100.0 * several / n_filled:.1f} % of the filled cells blend more than one sample') in lines
    level = got['fill_level']
    assert lines[-1] == (f'mosaic fill of {got["fill"]:.6g} m (3 levels): {int((level > 0).sum())} cells filled, {int((level < 0).sum())} left empty; '
                         f'deepest level {int(level.max())}')


def test_cli_eviction_changes_no_bit(cli, monkeypatch):
    """A cache budget of one and a half of the larger images: every phase, the accumulate phase too, reads the files again."""
    s = cli['mixed']
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('SUCRE_CONSISTENCY_CACHE_GB', str(1.5 * 96 * 64 * 12 / 2 ** 30))
    reads = []
    real = sucre._read_restored
    monkeypatch.setattr(sucre, '_read_restored', lambda path, image, **kw: (reads.append((path.name, kw.get('lazy', False))), real(path, image, **kw))[1])
    _main(_base(s.root) + ['--image-ids', 1, 10, '--output-dir', s.root / 'small_cache'] + s.flags)
    full_reads = [n for n, lazy in reads if not lazy]
    print(f'{len(full_reads)} reads of 9 restored images over the five phases')
    assert len(full_reads) > 4 * len(s.names)      # bounds, splat, resolve, gather and accumulate
    same_tensors(torch.load(s.root / 'all' / 'mosaic.pt'), torch.load(s.root / 'small_cache' / 'mosaic.pt'), 'small cache')
    for name in list(PICTURES) + list(OTHER_PICTURES):
        assert (s.root / 'all' / name).read_bytes() == (s.root / 'small_cache' / name).read_bytes(), name


def test_cli_a_fixed_stretch_reaches_every_picture(cli, monkeypatch):
    s = cli['mixed']
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    _main(_base(s.root) + ['--image-ids', 1, 10, '--output-dir', s.root / 'fixed', '--stretch-from', s.root / 'stretch.pt'] + s.flags)
    was, got = torch.load(s.root / 'all' / 'mosaic.pt'), torch.load(s.root / 'fixed' / 'mosaic.pt')
    same_tensors(was, got, 'fixed stretch')
    lo, hi = sucre.read_stretch_file(s.root / 'stretch.pt')
    for name, k in PICTURES.items():
        assert np.array_equal(png(s.root / 'fixed' / name), sucre.stretch_picture(got[k].numpy(), lo, hi)), name
        assert not np.array_equal(png(s.root / 'fixed' / name), png(s.root / 'all' / name)), name
    for name in OTHER_PICTURES:
        assert (s.root / 'all' / name).read_bytes() == (s.root / 'fixed' / name).read_bytes(), name


def test_cli_a_request_is_its_own_ordinals(cli, monkeypatch):
    s = cli['mixed']
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    # ids 4 .. 8: the last three images of camera 1 and the first two of camera 2
    _main(_base(s.root) + ['--image-ids', 4, 9, '--output-dir', s.root / 'some'] + s.flags)
    names = s.names[3:8]
    got = torch.load(s.root / 'some' / 'mosaic.pt')
    c, want = expected_of_files(s.model, names, s.restored, s.gsd)
    assert sorted({tuple(v.depth.shape) for v in c.views}) == [(33, 47), (64, 96)]
    check_file(got, want, names, 'images 4 .. 8')
    assert set(got['source'].flatten().tolist()) <= set(range(-1, 5)) and cases.winners(want) == [0, 1, 2, 3, 4]
    # one image of the second camera
    one = s.names[7]
    _main(_base(s.root) + ['--image-name', one, '--output-dir', s.root / 'one'] + s.flags)
    got = torch.load(s.root / 'one' / 'mosaic.pt')
    c, want = expected_of_files(s.model, [one], s.restored, s.gsd)
    check_file(got, want, [one], f'{one} alone')
    filled = got['source'] >= 0
    assert set(got['source'].flatten().tolist()) == {-1, 0} and bool((got['samples'][filled] >= 1).all()) and not bool(got['samples'][~filled].any())


def test_cli_thirty_three_images_through_the_batching_of_sucre_mosaic(cli, monkeypatch):
    s = cli['many']
    assert len(s.names) == 33 > sucre.MOSAIC_IMAGES_PER_CALL
    got = torch.load(s.root / 'all' / 'mosaic.pt')
    c, want = expected_of_files(s.model, s.names, s.restored, s.gsd)
    check_file(got, want, s.names, '33 images')
    assert 32 in cases.winners(want) and int(got['per_image'][32]) > 0
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('SUCRE_CONSISTENCY_CACHE_GB', str(5 * 24 * 16 * 12 / 2 ** 30))      # five images: batches of five
    _main(_base(s.root) + ['--image-ids', 1, 34, '--output-dir', s.root / 'small_cache'] + s.flags)
    same_tensors(got, torch.load(s.root / 'small_cache' / 'mosaic.pt'), '33 images, small cache')
    for name in list(PICTURES) + list(OTHER_PICTURES):
        assert (s.root / 'all' / name).read_bytes() == (s.root / 'small_cache' / name).read_bytes(), name


def test_cli_mosaic_of_images_restored_by_a_fit(cli, monkeypatch):
    """``J`` of a per-image fit is NaN where no view observes the pixel: who takes part is not the depth mask alone.  A J-parameter
    fit starts from the image's own colours and an image observes itself, so neither leaves such a pixel; the closed-form J of an
    image that is no neighbour of its own (the first one here, seen by the second and third alone) is 0 / 0 where they do not look."""
    s = cli['mixed']
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    names = s.names[:3]
    fitted = s.root / 'fitted'
    (s.root / 'not_neighbours.txt').write_text('\n'.join(s.names[3:] + s.names[:1]) + '\n')
    _main(_base(s.root) + ['--image-ids', 1, 4, '--output-dir', fitted, '--num-iter', 3, '--use-closed-form',
                           '--filter-images-path', s.root / 'not_neighbours.txt'])
    flags = ['--mosaic', fitted] + s.flags[2:]
    _main(_base(s.root) + ['--image-ids', 1, 4, '--output-dir', s.root / 'of_fitted'] + flags)
    c, want = expected_of_files(s.model, names, fitted, s.gsd)
    unseen = [int(((v.depth > 0) & torch.isnan(J).any(dim=2)).sum()) for v, J in zip(c.views, c.Js)]
    print(f'pixels with a valid depth and no restored colour: {unseen}')
    assert max(unseen) > 0
    check_file(torch.load(s.root / 'of_fitted' / 'mosaic.pt'), want, names, 'three fitted images')
