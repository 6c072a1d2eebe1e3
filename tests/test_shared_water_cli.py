"""CPU tier: the --shared-water flag of the command line (sucre_amd/sucre.py) and the light group's C ABI validation."""
import ctypes as C

from sucre_amd import _lib, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def test_parser_accepts_shared_water_and_leaves_other_defaults():
    p = sucre.build_parser()
    off, on = p.parse_args(BASE), p.parse_args(BASE + ['--shared-water'])
    # off unless given: the namespace of a run without the flag is the reference's, key for key
    assert getattr(off, 'shared_water', False) is False and 'shared_water' not in vars(off) and on.shared_water is True
    assert vars(off) == {k: v for k, v in vars(on).items() if k != 'shared_water'}
    assert '--shared-water' in p.format_help()
    defaults = {a.dest: a.default for a in p._actions if a.dest not in ('help', 'shared_water')}
    assert defaults == {'image_dir': None, 'depth_dir': None, 'model_dir': None, 'output_dir': None, 'image_name': None,
                        'image_list': None, 'image_ids': None, 'light_model': False, 'use_closed_form': False,
                        'min_cover': 0.000001, 'image_scale': 1.0, 'filter_images_path': None, 'learning_rate': 0.05,
                        'num_iter': 200, 'batch_size': 5, 'save_interval': None, 'params_path': None,
                        'force_compute_matches': False, 'keep_matches': False, 'num_workers': 0, 'device': 'cuda'}


def test_shared_water_refuses_flags_before_any_work(tmp_path, capsys):
    import pytest
    for extra, word in ((['--image-scale', '0.5'], '--image-scale'), (['--save-interval', '5'], '--save-interval')):
        out = tmp_path / 'out'
        argv = ['--image-dir', str(tmp_path / 'nowhere'), '--depth-dir', str(tmp_path), '--model-dir', str(tmp_path / 'nomodel'),
                '--output-dir', str(out), '--image-name', 'x.png', '--shared-water'] + extra
        with pytest.raises(SystemExit) as e:
            sucre.main(argv)
        assert e.value.code != 0 and word in str(e.value.code) and '--shared-water' in str(e.value.code)
        assert not out.exists()


def test_light_group_abi_validates_on_the_host():
    lib = _lib.load()
    assert lib.sucre_light_group_bytes(0) == 0
    assert lib.sucre_light_group_bytes(3) > lib.sucre_light_group_bytes(1) > 0
    off = lib.sucre_light_group_sums_offset()
    assert off >= 0 and off % 8 == 0
    p0 = (C.c_float * 19)()
    img = (_lib.LightGroupImage * 1)(_lib.LightGroupImage(256, 512, 48, 64, 3, 0))
    g = C.c_void_p(1 << 20)
    assert lib.sucre_light_group_init(None, 1, img, p0, None) == -1
    assert lib.sucre_light_group_init(C.c_void_p(4), 1, img, p0, None) == -1 and b'aligned' in lib.sucre_last_error()
    assert lib.sucre_light_group_init(g, 0, img, p0, None) == -1
    assert lib.sucre_light_group_init(g, 1, img, None, None) == -1
    bad = (_lib.LightGroupImage * 1)(_lib.LightGroupImage(256, None, 48, 64, 3, 0))
    assert lib.sucre_light_group_init(g, 1, bad, p0, None) == -1 and b'light workspace' in lib.sucre_last_error()
    # a buffer no init has set up, and the flags a light group refuses, are refused before anything is launched
    h = C.c_void_p(1 << 21)
    assert lib.sucre_light_group_iter(h, 1, 1, 0.05, 0.9, 0.999, 1e-8, 0, 10, None, None) == -1
    assert b'sucre_light_group_init' in lib.sucre_last_error()
    for flags, word in ((_lib.FIT_EXT_COLOUR, b'uint8 colours'), (_lib.FIT_EXT_BOTH, b'uint8 colours'),
                        (_lib.FIT_OBS_U16MM, b'f32 store'), (64, b'unknown')):
        assert lib.sucre_light_group_iter(h, 1, 1, 0.05, 0.9, 0.999, 1e-8, flags, 10, None, None) == -1
        assert word in lib.sucre_last_error()
        assert lib.sucre_light_group_finish(h, 1, 0, 0.05, 0.9, 0.999, 1e-8, flags, 10, None, None) == -1
    assert lib.sucre_light_group_iter(h, 1, 0, 0.05, 0.9, 0.999, 1e-8, 0, 10, None, None) == -2
    assert lib.sucre_light_group_iter(h, 1, 1, 0.05, 0.9, 0.999, 1e-8, 0, 0, None, None) == -2
