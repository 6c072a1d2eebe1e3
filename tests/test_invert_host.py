"""CPU tier of the single-view inversion: host-side validation of sucre_invert_bytes / sucre_invert_images (nothing is
launched), the --apply-water flag, the combinations refused before any file is opened, and the water file's keys and shapes."""
import builtins
import ctypes as C
import io

import pytest
import torch

from sucre_amd import _lib, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def image(depth=256, rgb=512, J=1024, H=48, W=64):
    im = _lib.InvertImage()
    im.depth, im.rgb, im.J, im.H, im.W = depth, rgb, J, H, W
    im.Kinv = (C.c_float * 9)(0.01, 0, -0.3, 0, 0.01, -0.2, 0, 0, 1)
    return im


def test_struct_and_table_size():
    assert C.sizeof(_lib.InvertImage) == 72 and _lib.InvertImage.Kinv.offset == 32 and _lib.InvertImage.reserved.offset == 68
    lib = _lib.load()
    one, many = lib.sucre_invert_bytes(1), lib.sucre_invert_bytes(_lib.INVERT_MAX_IMAGES)
    assert one >= 72 and one % 256 == 0 and many >= 72 * _lib.INVERT_MAX_IMAGES and many % 256 == 0
    assert lib.sucre_invert_bytes(32) >= lib.sucre_invert_bytes(31) >= one
    assert lib.sucre_invert_bytes(0) == 0 and b'n_images' in lib.sucre_last_error()
    assert lib.sucre_invert_bytes(-3) == 0
    assert lib.sucre_invert_bytes(_lib.INVERT_MAX_IMAGES + 1) == 0 and b'4096' in lib.sucre_last_error()


def test_invert_validates_before_any_launch():
    """No device is needed: every call below returns before a kernel would be launched (the pointers are not memory)."""
    lib = _lib.load()
    table = C.c_void_p(4096)
    p9, p19 = (C.c_float * 9)(*[0.1] * 9), (C.c_float * 19)(*[0.1] * 19)
    one = (_lib.InvertImage * 1)(image())
    call = lib.sucre_invert_images
    # the table
    assert call(None, 1, one, p9, 0, None) == -1 and b'table' in lib.sucre_last_error()
    assert call(C.c_void_p(4096 + 128), 1, one, p9, 0, None) == -1 and b'256-byte aligned' in lib.sucre_last_error()
    # the count
    assert call(table, 0, one, p9, 0, None) == -2 and b'n_images' in lib.sucre_last_error()
    assert call(table, -1, one, p9, 0, None) == -2
    assert call(table, _lib.INVERT_MAX_IMAGES + 1, one, p9, 0, None) == -2 and b'4096' in lib.sucre_last_error()
    # images / params
    assert call(table, 1, None, p9, 0, None) == -1 and b'NULL' in lib.sucre_last_error()
    assert call(table, 1, one, None, 0, None) == -1 and b'NULL' in lib.sucre_last_error()
    # flags
    for flags in (4, 8, 64, 1 | 4):
        assert call(table, 1, one, p19, flags, None) == -1 and b'unknown invert flags' in lib.sucre_last_error(), flags
    # sizes
    for H, W in ((0, 64), (48, 0), (-1, 64), (32768, 64), (48, 32768)):
        bad = (_lib.InvertImage * 2)(image(), image(H=H, W=W))
        assert call(table, 2, bad, p9, 0, None) == -1 and b'image 1: invalid size' in lib.sucre_last_error(), (H, W)
    # pointers: NULL, then misaligned
    for field in ('depth', 'rgb', 'J'):
        bad = (_lib.InvertImage * 2)(image(), image(**{field: 0}))
        assert call(table, 2, bad, p9, 0, None) == -1 and b'image 1' in lib.sucre_last_error() and b'NULL' in lib.sucre_last_error(), field
    for flags, field, ptr in ((0, 'depth', 260), (0, 'J', 1032), (0, 'rgb', 514), (_lib.INVERT_FLOAT_COLOUR, 'rgb', 516),
                              (_lib.INVERT_LIGHT | _lib.INVERT_FLOAT_COLOUR, 'rgb', 520)):
        bad = (_lib.InvertImage * 1)(image(**{field: ptr}))
        assert call(table, 1, bad, p19, flags, None) == -1 and b'aligned' in lib.sucre_last_error(), (flags, field)
    # (uint8 colours need 4 bytes only: 516 passes the checks of a call that then fails on the next image)
    ok_then_bad = (_lib.InvertImage * 2)(image(rgb=516), image(H=0))
    assert call(table, 2, ok_then_bad, p9, 0, None) == -1 and b'image 1: invalid size' in lib.sucre_last_error()


def test_flag_parses_and_leaves_the_reference_table_alone():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'apply_water' not in vars(off)
    on = p.parse_args(BASE + ['--apply-water', 'w.pt'])
    assert str(on.apply_water) == 'w.pt' and vars(off) == {k: v for k, v in vars(on).items() if k != 'apply_water'}
    assert '--apply-water PATH' in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ['--apply-water'])
    # the reference's actions and defaults, as tests/test_shared_water_cli.py pins them
    defaults = {a.dest: a.default for a in p._actions if a.dest not in ('help', 'shared_water')}
    assert defaults == {'image_dir': None, 'depth_dir': None, 'model_dir': None, 'output_dir': None, 'image_name': None,
                        'image_list': None, 'image_ids': None, 'light_model': False, 'use_closed_form': False,
                        'min_cover': 0.000001, 'image_scale': 1.0, 'filter_images_path': None, 'learning_rate': 0.05,
                        'num_iter': 200, 'batch_size': 5, 'save_interval': None, 'params_path': None,
                        'force_compute_matches': False, 'keep_matches': False, 'num_workers': 0, 'device': 'cuda'}
    assert all(a.dest != 'apply_water' for a in p._actions)


@pytest.mark.parametrize('extra, named', [(['--shared-water'], '--shared-water'), (['--trim-outliers', '3'], '--trim-outliers'),
                                          (['--trim-rounds', '2'], '--trim-outliers'), (['--save-quality'], '--save-quality'),
                                          (['--save-interval', '5'], '--save-interval'), (['--params-path', 'p.pt'], '--params-path'),
                                          (['--keep-matches'], '--keep-matches')])
def test_refusals_exit_before_any_file_is_opened(extra, named, tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    opened = []
    real_open = builtins.open
    spy = lambda *a, **k: (opened.append(a[0]), real_open(*a, **k))[1]   # noqa: E731
    monkeypatch.setattr(builtins, 'open', spy)
    monkeypatch.setattr(io, 'open', spy)   # (pathlib's read_text / open)
    monkeypatch.setattr(torch, 'load', lambda *a, **k: opened.append(a[0]))
    out = tmp_path / 'out'
    argv = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
            '--output-dir', str(out), '--image-name', 'x.png', '--apply-water', str(tmp_path / 'w.pt')] + extra
    with pytest.raises(SystemExit) as e:
        sucre.main(argv)
    assert e.value.code != 0 and '--apply-water' in str(e.value.code) and named in str(e.value.code)
    assert not opened and not out.exists()


def water(light=False):
    w = {'B': torch.full((3, 1), 0.09), 'beta': torch.full((3, 1), 0.3), 'gamma': torch.full((3, 1), 0.14)}
    if light:
        w.update(cam2light=torch.zeros(6), sigma=torch.eye(2))
    return w


def test_water_file_keys_and_shapes(tmp_path):
    # what qualifies: a shared_water.pt (extra keys trace, images) and a per-image <name>.pt (extra key J)
    torch.save({**water(), 'trace': torch.zeros(4, 10, dtype=torch.float64), 'images': ['a.png']}, tmp_path / 'shared_water.pt')
    got = sucre.read_water_file(tmp_path / 'shared_water.pt')
    assert list(got) == ['B', 'beta', 'gamma'] and all(t.dtype == torch.float32 and t.shape == (3, 1) for t in got.values())
    torch.save({**water(True), 'J': torch.zeros(2, 2, 3)}, tmp_path / 'a.pt')
    assert list(sucre.read_water_file(tmp_path / 'a.pt', True)) == ['B', 'beta', 'gamma', 'cam2light', 'sigma']
    assert list(sucre.read_water_file(tmp_path / 'a.pt', False)) == ['B', 'beta', 'gamma']
    torch.save({k: v.double() for k, v in water().items()}, tmp_path / 'f64.pt')
    assert sucre.read_water_file(tmp_path / 'f64.pt')['beta'].dtype == torch.float32
    # missing keys
    for light, key in ((False, 'B'), (False, 'beta'), (False, 'gamma'), (True, 'cam2light'), (True, 'sigma')):
        w = water(light)
        del w[key]
        torch.save(w, tmp_path / 'bad.pt')
        with pytest.raises(SystemExit) as e:
            sucre.read_water_file(tmp_path / 'bad.pt', light)
        assert '--apply-water' in str(e.value.code) and f"'{key}'" in str(e.value.code) and 'bad.pt' in str(e.value.code)
    # a 9-parameter file with --light-model
    torch.save(water(), tmp_path / 'nine.pt')
    with pytest.raises(SystemExit) as e:
        sucre.read_water_file(tmp_path / 'nine.pt', True)
    assert "'cam2light'" in str(e.value.code)
    # mis-shaped keys
    for light, key, value in ((False, 'B', torch.zeros(3)), (False, 'beta', torch.zeros(1, 3)), (False, 'gamma', [0.1, 0.1, 0.1]),
                              (True, 'cam2light', torch.zeros(6, 1)), (True, 'sigma', torch.zeros(4))):
        torch.save({**water(light), key: value}, tmp_path / 'bad.pt')
        with pytest.raises(SystemExit) as e:
            sucre.read_water_file(tmp_path / 'bad.pt', light)
        assert f"'{key}'" in str(e.value.code) and 'shape' in str(e.value.code)
    # not a parameter file at all, and no file
    torch.save(torch.zeros(3), tmp_path / 'tensor.pt')
    with pytest.raises(SystemExit) as e:
        sucre.read_water_file(tmp_path / 'tensor.pt')
    assert '--apply-water' in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        sucre.read_water_file(tmp_path / 'absent.pt')
    assert 'absent.pt' in str(e.value.code)


def test_a_bad_water_file_stops_the_command_line_before_the_model_is_looked_for(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    w = water()
    del w['gamma']
    torch.save(w, tmp_path / 'w.pt')
    out = tmp_path / 'out'
    argv = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
            '--output-dir', str(out), '--image-name', 'x.png', '--apply-water', str(tmp_path / 'w.pt')]
    with pytest.raises(SystemExit) as e:
        sucre.main(argv)
    assert "'gamma'" in str(e.value.code) and not out.exists()


def test_check_water_and_the_engine_entry_point_refuse_on_the_host():
    from sucre_amd import engine
    with pytest.raises(ValueError, match="'beta'"):
        sucre.check_water({'B': torch.zeros(3, 1), 'gamma': torch.zeros(3, 1)})
    with pytest.raises(ValueError, match='no view'):
        engine.invert_images([], [0.1] * 9)
    cpu = engine.DeviceView(depth=torch.ones(2, 2), rgb=torch.zeros(2, 2, 3, dtype=torch.uint8), K=torch.eye(3), R=torch.eye(3), t=torch.zeros(3, 1))
    f32 = engine.DeviceView(depth=torch.ones(2, 2), rgb=torch.zeros(2, 2, 3), K=torch.eye(3), R=torch.eye(3), t=torch.zeros(3, 1))
    with pytest.raises(ValueError, match='all uint8 or all float32'):
        engine.invert_images([cpu, f32], [0.1] * 9)
    with pytest.raises(ValueError, match='9 parameters'):
        engine.invert_images([cpu], [0.1] * 19)
    with pytest.raises(ValueError, match='19 parameters'):
        engine.invert_images([cpu], [0.1] * 9, light=True)
    with pytest.raises(_lib.SucreError, match='no CPU fallback'):
        engine.invert_images([cpu], [0.1] * 9)
