"""CPU tier of the residual pass: host-side validation of sucre_fit_residuals* (nothing is launched), the scratch size, the two
picture mappings of --save-quality and the flag itself."""
import ctypes as C

import numpy as np

from sucre_amd import _lib, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def test_scratch_size_grows_with_the_views():
    lib = _lib.load()
    a, b = lib.sucre_residual_scratch_bytes(52, 75, 7), lib.sucre_residual_scratch_bytes(52, 75, 8)
    assert 0 < a < b
    assert b - a == 5 * 4 * 16                                  # one {n, sum r^2 R, G, B} per tile and view
    assert lib.sucre_residual_scratch_bytes(1080, 1920, 65) >= 8160 * 65 * 16
    assert lib.sucre_residual_scratch_bytes(0, 75, 7) == 0 and b'invalid geometry' in lib.sucre_last_error()
    assert lib.sucre_residual_scratch_bytes(52, 75, 0) == 0
    assert lib.sucre_residual_scratch_bytes(52, 75, 4097) == 0


def test_residual_entry_points_validate_before_any_launch():
    lib = _lib.load()
    ws, lws, out = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    plain = lambda *a: lib.sucre_fit_residuals(*a)           # noqa: E731
    ext = lambda *a: lib.sucre_fit_residuals_ext(*a)         # noqa: E731
    # workspace and geometry
    assert plain(None, 48, 64, 3, _lib.OBS_F32, out, out, out, out, None) == -1 and b'NULL' in lib.sucre_last_error()
    assert plain(C.c_void_p(4), 48, 64, 3, _lib.OBS_F32, out, out, out, out, None) == -1 and b'aligned' in lib.sucre_last_error()
    assert plain(ws, 0, 64, 3, _lib.OBS_F32, out, out, out, out, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
    # format
    assert plain(ws, 48, 64, 3, 7, out, out, out, out, None) == -1 and b'unknown observation format' in lib.sucre_last_error()
    assert plain(ws, 48, 64, 3, -1, out, out, out, out, None) == -1
    # outputs: NULL, then misaligned
    for i in range(4):
        args = [out] * 4
        args[i] = None
        assert plain(ws, 48, 64, 3, _lib.OBS_U16MM, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
        assert ext(ws, lws, 48, 64, 3, 0, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
    for i, bad in enumerate((1026, 1026, 1028, 1032)):          # int32, float32, float64, 16-byte scratch
        args = [out] * 4
        args[i] = C.c_void_p(bad)
        assert plain(ws, 48, 64, 3, _lib.OBS_F32, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
        assert ext(ws, lws, 48, 64, 3, 0, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
    # the extension workspace and the flags
    assert ext(ws, None, 48, 64, 3, 0, out, out, out, out, None) == -1 and b'light workspace' in lib.sucre_last_error()
    assert ext(ws, C.c_void_p(516), 48, 64, 3, 0, out, out, out, out, None) == -1 and b'aligned' in lib.sucre_last_error()
    assert ext(None, lws, 48, 64, 3, 0, out, out, out, out, None) == -1
    for flags in (_lib.FIT_CLOSED_FORM, _lib.FIT_OBS_U16MM, _lib.FIT_KEEP_J, 64):
        assert ext(ws, lws, 48, 64, 3, flags, out, out, out, out, None) == -1 and b'unknown flags' in lib.sucre_last_error(), flags
    assert ext(ws, lws, 48, 64, 3, _lib.FIT_EXT_COLOUR | _lib.FIT_EXT_BOTH, out, out, out, out, None) == -1
    assert b'exclude each other' in lib.sucre_last_error()


def test_picture_mappings_on_a_fixed_array():
    count = np.array([[0, 1, 2, 3], [4, 5, 6, 6]], np.int32)
    cov = sucre.coverage_image(count, 6)
    assert cov.dtype == np.uint8 and cov.tolist() == [[0, 42, 85, 127], [170, 212, 255, 255]]     # 255 * count // 6
    assert sucre.coverage_image(np.zeros((1, 2), np.int32), 0).tolist() == [[0, 0]]
    assert sucre.QUALITY_RMS_FULL_SCALE == 0.25
    ssr = np.zeros((2, 4, 3), np.float32)
    ssr[0, 0] = 5.0                        # no observation: black whatever the sums hold
    ssr[0, 1] = [0.03, 0.03, 0.03]         # rms = sqrt(0.09 / 3) = 0.1732 -> 255 * 0.6928 = 176.7
    ssr[0, 2] = [0.0, 0.0, 0.12]           # rms = sqrt(0.12 / 6) = 0.1414 -> 255 * 0.5657 = 144.2
    ssr[0, 3] = [1.0, 1.0, 1.0]            # rms = sqrt(3 / 9) = 0.577: clipped to white
    ssr[1, 0] = [0.75, 0.0, 0.0]           # rms = sqrt(0.75 / 12) = 0.25: exactly full scale
    res = sucre.residual_image(count, ssr)
    assert res.dtype == np.uint8 and res.shape == (2, 4)
    assert res[0].tolist() == [0, 176, 144, 255] and res[1].tolist() == [255, 0, 0, 0]


def test_parser_namespace_is_unchanged_without_the_flag():
    p = sucre.build_parser()
    off, on = p.parse_args(BASE), p.parse_args(BASE + ['--save-quality'])
    assert 'save_quality' not in vars(off) and on.save_quality is True
    assert vars(off) == {k: v for k, v in vars(on).items() if k != 'save_quality'}
    both = p.parse_args(['--save-quality'] + BASE + ['--shared-water'])
    assert both.save_quality is True and both.shared_water is True
    assert '--save-quality' in p.format_help()
    # the reference's table of flags and defaults is what it was (sucre.py:265-305)
    assert set(vars(off)) == {'image_dir', 'depth_dir', 'model_dir', 'output_dir', 'image_name', 'image_list', 'image_ids',
                              'light_model', 'use_closed_form', 'min_cover', 'image_scale', 'filter_images_path', 'learning_rate',
                              'num_iter', 'batch_size', 'save_interval', 'params_path', 'force_compute_matches', 'keep_matches',
                              'num_workers', 'device'}
