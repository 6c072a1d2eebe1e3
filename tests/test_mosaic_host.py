"""CPU tier of the seabed mosaic: the default frame and ground sample distance, the --mosaic flag and what is refused before any
file is opened, the new library entries and their argument validation (nothing is launched), and the oracle of the GPU tests
(tests/mosaic_ref.py) against hand-computed mosaics."""
import builtins
import ctypes as C
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_ref as ref
from sucre_amd import _lib, engine, sucre, synth

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


# ---- mosaic_axes ---------------------------------------------------------------------------------------------------------------

def axes64(Rs):
    """The frame in float64, written out independently of sucre.mosaic_axes."""
    Rs = [np.asarray(R, np.float64) for R in Rs]
    m = np.mean([R[:, 2] for R in Rs], axis=0)
    e3 = m / np.sqrt((m * m).sum())
    a = Rs[0][:, 0] - (Rs[0][:, 0] @ e3) * e3
    if np.sqrt((a * a).sum()) < 1e-6:
        a = Rs[0][:, 1] - (Rs[0][:, 1] @ e3) * e3
    e1 = a / np.sqrt((a * a).sum())
    return np.stack([e1, np.cross(e3, e1), e3])


def test_axes_are_orthonormal_and_look_the_way_the_cameras_look():
    survey = synth.make_survey(24, 16, 3, 2)
    axes = sucre.mosaic_axes(survey.views)
    assert axes.dtype == torch.float32 and tuple(axes.shape) == (3, 3)
    A = axes.double().numpy()
    assert np.abs(A @ A.T - np.eye(3)).max() < 1e-6
    mean_axis = np.mean([v.R.double().numpy()[:, 2] for v in survey.views], axis=0)
    assert A[2] @ mean_axis > 0
    assert np.allclose(np.cross(A[2], A[0]), A[1], atol=1e-6)
    # sfm.Image objects (pose.R) give the same frame as anything with R
    as_images = [SimpleNamespace(pose=SimpleNamespace(R=v.R)) for v in survey.views]
    assert torch.equal(sucre.mosaic_axes(as_images), axes)


def test_axes_are_rounded_once_from_float64():
    survey = synth.make_survey(24, 16, 3, 2, seed=4)
    want = axes64([v.R.double().numpy() for v in survey.views])
    got = sucre.mosaic_axes(survey.views).numpy()
    assert np.array_equal(got, want.astype(np.float32))
    # a frame formed in float32 throughout is not that one: the check above can tell the two apart
    f32 = axes64([v.R.numpy().astype(np.float32) for v in survey.views])
    assert np.abs(want - f32).max() < 1e-12   # (float32 rotations widen exactly: the inputs are the same)


def test_axes_fall_back_to_the_second_column():
    """Both cameras look along z; the first one's column 0 is that very direction (the function reads columns only, so the
    matrix need not be a rotation): nothing of it is left once e3 is removed, and column 1 serves."""
    first = torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])
    views = [SimpleNamespace(R=first), SimpleNamespace(R=torch.eye(3))]
    axes = sucre.mosaic_axes(views).numpy()
    assert np.array_equal(axes[2], [0.0, 0.0, 1.0])
    assert np.array_equal(axes[0], [0.0, 1.0, 0.0])
    assert np.array_equal(axes[1], [-1.0, 0.0, 0.0])    # e3 x e1
    # a remainder just above the threshold is still taken from column 0
    tilted = first.clone()
    tilted[0, 0] = 1e-5
    axes = sucre.mosaic_axes([SimpleNamespace(R=tilted), SimpleNamespace(R=torch.eye(3))]).numpy()
    assert axes[0, 0] > 0.999
    with pytest.raises(ValueError, match='no image'):
        sucre.mosaic_axes([])


# ---- the default ground sample distance -----------------------------------------------------------------------------------------

def test_default_gsd_on_a_known_survey():
    survey = synth.make_survey(96, 64, 3, 2)
    fx = float(survey.K[0, 0])
    medians = []
    for v in survey.views:
        d = np.sort(v.depth_f32().double().numpy().ravel())
        d = d[d > 0]
        mid = d.size // 2
        medians.append((d[mid] if d.size % 2 else 0.5 * (d[mid - 1] + d[mid])) / fx)
    medians = np.sort(medians)
    want = np.float32(2.0 * 0.5 * (medians[2] + medians[3]))
    got = sucre.mosaic_default_gsd([v.depth_f32() for v in survey.views], [fx] * 6)
    assert isinstance(got, np.float32) and got == want
    assert 0.05 < float(got) < 0.12    # about 2 x 3 m / (0.78 x 96)
    # an image without a valid depth is left out; none at all is refused
    empty = torch.zeros(4, 4)
    assert sucre.mosaic_default_gsd([v.depth_f32() for v in survey.views] + [empty], [fx] * 7) == want
    with pytest.raises(ValueError, match='valid depth'):
        sucre.mosaic_default_gsd([empty], [fx])
    assert engine.mosaic_cells(0.0, 1.0, 0.25) == 5 and engine.mosaic_cells(1.5, 1.5, 0.1) == 1


# ---- the flag and what it refuses -------------------------------------------------------------------------------------------

def test_flag_lives_in_extras_and_leaves_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'mosaic' not in vars(off) and 'mosaic_gsd' not in vars(off)
    on = p.parse_args(BASE + ['--mosaic', 'results', '--mosaic-gsd', '0.05'])
    assert str(on.mosaic) == 'results' and on.mosaic_gsd == 0.05
    assert vars(off) == {k: v for k, v in vars(on).items() if k not in ('mosaic', 'mosaic_gsd')}
    assert all(a.dest not in ('mosaic', 'mosaic_gsd') for a in p._actions)
    assert '--mosaic DIR' in p.format_help() and '--mosaic-gsd G' in p.format_help()


REFUSED = [(['--shared-water'], '--shared-water'), (['--apply-water', 'w.pt'], '--apply-water'), (['--check-consistency', 'r'], '--check-consistency'),
           (['--trim-outliers', '3'], '--trim-outliers'), (['--trim-rounds', '2'], '--trim-outliers'), (['--view-gains'], '--view-gains'),
           (['--gain-rounds', '2'], '--view-gains'), (['--gain-limit', '3'], '--view-gains'), (['--save-quality'], '--save-quality'),
           (['--save-interval', '5'], '--save-interval'), (['--params-path', 'p.pt'], '--params-path'), (['--keep-matches'], '--keep-matches'),
           (['--common-stretch'], '--common-stretch'), (['--image-scale', '0.5'], '--image-scale'), (['--mosaic-gsd', '0'], '--mosaic-gsd'),
           (['--mosaic-gsd', 'nan'], '--mosaic-gsd')]


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


@pytest.mark.parametrize('extra, named', REFUSED, ids=[' '.join(e) for e, _ in REFUSED])
def test_refusals_name_both_flags_before_any_file_is_opened(extra, named, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    message = run_refused(['--mosaic', str(tmp_path / 'results')] + extra, tmp_path, monkeypatch)
    assert '--mosaic' in message and named in message


def test_a_world_above_one_is_refused_with_the_reason(tmp_path, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    message = run_refused(['--mosaic', str(tmp_path / 'results')], tmp_path, monkeypatch)
    assert '--mosaic' in message and 'world size of 2' in message and 'all-reduce is not built' in message and 'separate entries' in message


def test_mosaic_gsd_needs_mosaic(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert '--mosaic-gsd: only with --mosaic' in run_refused(['--mosaic-gsd', '0.1'], tmp_path, monkeypatch)


def test_stretch_from_combines_with_mosaic(tmp_path, monkeypatch):
    """--stretch-from is not refused: the run gets as far as reading the stretch file, the first thing a run opens."""
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    out = tmp_path / 'out'
    argv = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
            '--output-dir', str(out), '--image-name', 'x.png', '--mosaic', str(tmp_path / 'results'), '--stretch-from', str(tmp_path / 'none.pt')]
    with pytest.raises(SystemExit) as e:
        sucre.main(argv)
    assert str(e.value.code).startswith('--stretch-from: cannot read') and not out.exists()


def test_the_other_modes_refuse_mosaic_in_their_own_wording():
    args = sucre.build_parser().parse_args(BASE + ['--mosaic', 'r'])
    for flag in ('--check-consistency', '--apply-water'):
        with pytest.raises(SystemExit) as e:
            sucre._refuse_mode_flags(args, flag)
        assert str(e.value.code).startswith(f'{flag}: --mosaic does not combine with it (') and str(e.value.code).endswith('; drop one of the two flags')


def test_a_missing_or_misshaped_restored_image_stops_the_run_before_anything_is_decoded(tmp_path, monkeypatch):
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda *a, **k: None)
    decoded = []
    cam = SimpleNamespace(height=4, width=6, K=torch.eye(3))

    def image(name):
        return SimpleNamespace(name=name, camera=cam, pose=SimpleNamespace(R=torch.eye(3)), device_view=lambda dev: decoded.append(name))

    results = tmp_path / 'results'
    results.mkdir()
    torch.save({'J': torch.zeros(4, 6, 3)}, results / 'a.pt')
    with pytest.raises(SystemExit) as e:
        sucre.mosaic([image('a.png'), image('b.png')], None, results, tmp_path / 'out')
    assert '--mosaic' in str(e.value.code) and 'b.pt' in str(e.value.code) and 'missing' in str(e.value.code)
    torch.save({'J': torch.zeros(4, 5, 3)}, results / 'b.pt')
    with pytest.raises(SystemExit) as e:
        sucre.mosaic([image('a.png'), image('b.png')], None, results, tmp_path / 'out')
    assert str(e.value.code).startswith('--mosaic: J of') and '(4, 5, 3)' in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        sucre.mosaic([image('a.png')] * (engine.MAX_VIEWS + 1), None, results, tmp_path / 'out')
    assert 'at most 4096' in str(e.value.code)
    assert not decoded and not (tmp_path / 'out').exists()
    # --check-consistency keeps its own wording for the same file
    with pytest.raises(SystemExit) as e:
        sucre._read_restored(results / 'b.pt', image('b.png'))
    assert str(e.value.code).startswith('--check-consistency: J of')


def test_source_picture_gives_every_ordinal_a_colour_and_leaves_empty_cells_black():
    source = np.array([[-1, 0, 1], [2, 0, 4095]], np.int32)
    pic = sucre.mosaic_source_picture(source)
    assert pic.dtype == np.uint8 and pic.shape == (2, 3, 3)
    assert not pic[0, 0].any() and (pic[source >= 0] >= 64).all()
    assert np.array_equal(pic[0, 1], pic[1, 1])
    colours = {tuple(sucre.mosaic_source_picture(np.array([[i]]))[0, 0]) for i in range(64)}
    assert len(colours) == 64


# ---- the library: the entries exist and check their arguments before any launch -------------------------------------------------

def test_abi_has_the_mosaic_entries_and_keeps_its_version():
    for name in ('sucre_mosaic_table_bytes', 'sucre_mosaic_bounds', 'sucre_mosaic_splat', 'sucre_mosaic_resolve', 'sucre_mosaic_gather'):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.sucre_version() == 2 == _lib.ABI_VERSION
    assert C.sizeof(_lib.MosaicImage) == 128 and C.sizeof(_lib.MosaicGrid) == 56
    assert lib.sucre_mosaic_table_bytes(1) == 256 and lib.sucre_mosaic_table_bytes(33) == 34 * 128 and lib.sucre_mosaic_table_bytes(4096) == 4096 * 128
    assert lib.sucre_mosaic_table_bytes(0) == 0 and lib.sucre_mosaic_table_bytes(4097) == 0 and b'n_images' in lib.sucre_last_error()


def good_image():
    im = _lib.MosaicImage()
    im.depth, im.rgb, im.J, im.H, im.W = 256, 512, 1024, 8, 16
    return im


def good_grid():
    g = _lib.MosaicGrid()
    g.axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = 0.5, 0.0, 0.0, 4, 4
    return g


def test_argument_validation_happens_before_any_launch():
    lib = _lib.load()
    ERR = -1   # SUCRE_ERR_ARG
    p = C.c_void_p(4096)
    axes = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    one = (_lib.MosaicImage * 1)(good_image())
    grid = good_grid()

    def each_phase(table, n, images, first, g):
        return [lib.sucre_mosaic_splat(table, n, images, first, g, p, 0, None), lib.sucre_mosaic_resolve(table, n, images, first, g, p, p, None),
                lib.sucre_mosaic_gather(table, n, images, first, g, p, p, p, p, p, p, p, None)]

    # the table, the count, the ordinals, the images
    assert lib.sucre_mosaic_bounds(None, 1, one, axes, p, None) == ERR and b'table' in lib.sucre_last_error()
    assert lib.sucre_mosaic_bounds(C.c_void_p(4100), 1, one, axes, p, None) == ERR and b'aligned' in lib.sucre_last_error()
    assert lib.sucre_mosaic_bounds(p, 0, one, axes, p, None) == ERR
    assert lib.sucre_mosaic_bounds(p, engine.MAX_VIEWS + 1, one, axes, p, None) == ERR and b'n_images=4097' in lib.sucre_last_error()
    assert lib.sucre_mosaic_bounds(p, 1, None, axes, p, None) == ERR and b'images is NULL' in lib.sucre_last_error()
    assert lib.sucre_mosaic_bounds(p, 1, one, None, p, None) == ERR and b'axes' in lib.sucre_last_error()
    assert lib.sucre_mosaic_bounds(p, 1, one, axes, None, None) == ERR and b'bounds_dev' in lib.sucre_last_error()
    assert lib.sucre_mosaic_bounds(p, 1, one, (C.c_float * 9)(*([float('nan')] * 9)), p, None) == ERR
    assert each_phase(None, 1, one, 0, C.byref(grid)) == [ERR] * 3
    assert each_phase(p, engine.MAX_VIEWS + 1, one, 0, C.byref(grid)) == [ERR] * 3
    assert each_phase(p, 1, one, engine.MAX_VIEWS, C.byref(grid)) == [ERR] * 3 and b'ordinals' in lib.sucre_last_error()
    assert each_phase(p, 1, one, -1, C.byref(grid)) == [ERR] * 3
    for field, value, what in (('depth', None, b'NULL'), ('rgb', None, b'NULL'), ('J', None, b'NULL'), ('H', 0, b'invalid size'),
                               ('W', 40000, b'invalid size'), ('J', 1026, b'aligned')):
        bad = good_image()
        setattr(bad, field, value)
        arr = (_lib.MosaicImage * 1)(bad)
        assert lib.sucre_mosaic_bounds(p, 1, arr, axes, p, None) == ERR and what in lib.sucre_last_error(), field
        assert each_phase(p, 1, arr, 0, C.byref(grid)) == [ERR] * 3, field
    # the grid
    assert each_phase(p, 1, one, 0, None) == [ERR] * 3 and b'grid is NULL' in lib.sucre_last_error()
    for field, value, what in (('gsd', 0.0, b'gsd'), ('gsd', -1.0, b'gsd'), ('gsd', float('nan'), b'gsd'), ('gsd', float('inf'), b'gsd'),
                               ('lo_s', float('inf'), b'lo='), ('Hm', 0, b'cells'), ('Wm', (1 << 24) + 1, b'cells')):
        bad = good_grid()
        setattr(bad, field, value)
        assert each_phase(p, 1, one, 0, C.byref(bad)) == [ERR] * 3 and what in lib.sucre_last_error(), (field, value)
    # the phase's own buffers
    assert lib.sucre_mosaic_splat(p, 1, one, 0, C.byref(grid), None, 0, None) == ERR and b'key_dev' in lib.sucre_last_error()
    assert lib.sucre_mosaic_splat(p, 1, one, 0, C.byref(grid), C.c_void_p(4100), 0, None) == ERR
    assert lib.sucre_mosaic_splat(p, 1, one, 0, C.byref(grid), p, 2, None) == ERR and b'flags' in lib.sucre_last_error()
    assert lib.sucre_mosaic_resolve(p, 1, one, 0, C.byref(grid), p, None, None) == ERR and b'pix_dev' in lib.sucre_last_error()
    assert lib.sucre_mosaic_gather(p, 1, one, 0, C.byref(grid), p, p, p, None, p, p, p, None) == ERR and b'raw_out' in lib.sucre_last_error()


def test_cell_limit_and_bad_arguments_of_the_python_class(monkeypatch):
    monkeypatch.delenv('SUCRE_MOSAIC_MAX_CELLS', raising=False)
    assert engine.mosaic_max_cells() == 1 << 27
    monkeypatch.setenv('SUCRE_MOSAIC_MAX_CELLS', '1000')
    assert engine.mosaic_max_cells() == 1000
    with pytest.raises(_lib.SucreError, match='no CPU fallback'):
        engine.Mosaic(torch.eye(3), 0.1, 'cpu')


# ---- the oracle on mosaics computed by hand ----------------------------------------------------------------------------------

def hand_view(depth, rgb=None, K=None, t=(0.0, 0.0, 0.0)):
    depth = torch.tensor(depth, dtype=torch.float32)
    H, W = depth.shape
    if rgb is None:
        rgb = (torch.arange(H * W * 3) % 251).to(torch.uint8).reshape(H, W, 3)
    K = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 1.0]] if K is None else K, dtype=torch.float32)
    return SimpleNamespace(depth=depth, rgb=rgb, K=K, R=torch.eye(3), t=torch.tensor(t, dtype=torch.float32).view(3, 1))


def test_oracle_on_a_two_by_two_mosaic_computed_by_hand():
    """Two 2x2 cameras looking down the z axis, K = [[1,0,1],[0,1,1],[0,0,1]]: pixel (u, v) at depth d is the camera point
    d (u - .5, v - .5, 1).  View 0 at depth 2 puts its pixels on x, y = -1 or +1 with range sqrt 6; its pixel 1 has no depth and its
    pixel 2 a NaN in J, so pixels 0 and 3 take part and the bounds are [-1, 1]^2.  gsd 1.5 gives 2 x 2 cells: q = (a + 1) / 1.5.
    View 1 at depth 1, shifted by .25 in x, puts its pixels on x = -.25 or .75 (q_s = .5, 1.1667: columns 0, 1) and y = -.5 or .5
    (q_t = .3333, 1.0: rows 0, 1) with range sqrt 1.5: it is nearer and wins all four cells, pixel p in cell p."""
    axes = torch.eye(3)
    v0 = hand_view([[2.0, 0.0], [2.0, 2.0]])
    v1 = hand_view([[1.0, 1.0], [1.0, 1.0]], t=(0.25, 0.0, 0.0))
    J0 = torch.arange(12, dtype=torch.float32).reshape(2, 2, 3)
    J0[1, 0, 1] = float('nan')
    J1 = 100 + torch.arange(12, dtype=torch.float32).reshape(2, 2, 3)
    p, z, a_s, a_t = ref.pixels(v0, J0, axes)
    assert p.tolist() == [0, 3] and a_s.tolist() == [-1.0, 1.0] and a_t.tolist() == [-1.0, 1.0]
    assert z.tolist() == [float(np.sqrt(np.float32(6.0)))] * 2    # (numpy's root is IEEE; torch's vectorised one is not)
    out = ref.mosaic([v0, v1], [J0, J1], axes, 1.5, bounds=(-1.0, -1.0, 1.0, 1.0))
    assert (out['Hm'], out['Wm']) == (2, 2)
    assert out['source'].tolist() == [[1, 1], [1, 1]]
    assert out['pixel'].tolist() == [[0, 1], [2, 3]]
    assert out['range'].tolist() == [[float(np.sqrt(np.float32(1.5)))] * 2] * 2
    assert torch.equal(out['J'], J1) and torch.equal(out['raw'], v1.rgb)
    # without view 1: view 0's two participating pixels, the rest empty
    out = ref.mosaic([v0], [J0], axes, 1.5)
    assert out['bounds'] == (-1.0, -1.0, 1.0, 1.0) and (out['Hm'], out['Wm']) == (2, 2)
    assert out['source'].tolist() == [[0, -1], [-1, 0]] and out['pixel'].tolist() == [[0, -1], [-1, 3]]
    assert torch.isnan(out['range'][0, 1]) and torch.isnan(out['J'][1, 0]).all() and out['raw'][0, 1].tolist() == [0, 0, 0]
    assert torch.equal(out['J'][1, 1], J0[1, 1]) and torch.equal(out['raw'][1, 1], v0.rgb[1, 1])
    # caller-given bounds that leave pixel 3 outside drop it
    out = ref.mosaic([v0], [J0], axes, 1.5, bounds=(-1.0, -1.0, 0.0, 0.0))
    assert (out['Hm'], out['Wm']) == (1, 1) and out['pixel'].tolist() == [[0]]
    # the same view twice: the earlier ordinal holds every cell
    out = ref.mosaic([v1, v1], [J1, J1], axes, 0.75)
    assert set(out['source'].flatten().tolist()) <= {0, -1} and int((out['source'] == 0).sum()) == 4


TIE_K = [[16.0, 0.0, 8.0], [0.0, 16.0, 4.0], [0.0, 0.0, 1.0]]


def tie_view():
    return hand_view(torch.ones(8, 16).tolist(), K=TIE_K)


def test_oracle_sees_the_four_way_tie_of_the_centre_pixels():
    """16x8 image, K = [[16,0,8],[0,16,4],[0,0,1]], depth 1: pixel (u, v) is the camera point ((u - 7.5) / 16, (v - 3.5) / 16, 1) --
    dyadic, so x^2 + y^2 + 1 is exact in float32 and the four centre pixels (7|8, 3|4) have ONE range, to the bit."""
    v = tie_view()
    J = torch.rand((8, 16, 3), generator=torch.Generator().manual_seed(1))
    p, z, a_s, a_t = ref.pixels(v, J, torch.eye(3))
    assert p.tolist() == list(range(128))
    zb = z.view(torch.int32)
    centre = [55, 56, 71, 72]
    assert len({int(zb[i]) for i in centre}) == 1 and float(z[55]) == float(np.sqrt(np.float32(1.0 + 2.0 / 1024.0)))
    assert all(int(zb[i]) > int(zb[55]) for i in range(128) if i not in centre)
    out = ref.mosaic([v], [J], torch.eye(3), 4.0)    # one cell for the whole image
    assert (out['Hm'], out['Wm']) == (1, 1) and int(out['ties'][0, 0]) == 4
    assert out['pixel'].tolist() == [[55]] and out['source'].tolist() == [[0]]
    assert torch.equal(out['J'][0, 0], J[3, 7])
