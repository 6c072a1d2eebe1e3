"""CPU tier of the outlier trim: the two flags, the combinations refused before any work, host-side validation of
sucre_trim_outliers* (nothing is launched), the scratch size and the arithmetic of <stem>_trimmed.png."""
import ctypes as C

import numpy as np
import pytest

from sucre_amd import _lib, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def test_flags_parse_and_leave_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert 'trim_outliers' not in vars(off) and 'trim_rounds' not in vars(off)
    on = p.parse_args(BASE + ['--trim-outliers', '3'])
    assert on.trim_outliers == 3.0 and isinstance(on.trim_outliers, float) and 'trim_rounds' not in vars(on)
    assert vars(off) == {k: v for k, v in vars(on).items() if k != 'trim_outliers'}
    two = p.parse_args(['--trim-rounds', '2'] + BASE + ['--trim-outliers', '2.5', '--save-quality'])
    assert two.trim_outliers == 2.5 and two.trim_rounds == 2 and two.save_quality is True
    assert '--trim-outliers K' in p.format_help() and '--trim-rounds N' in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ['--trim-outliers', 'three'])


@pytest.mark.parametrize('extra, named', [(['--shared-water'], '--shared-water'), (['--save-interval', '5'], '--save-interval')])
def test_refused_combinations_name_the_flag(extra, named, monkeypatch):
    """Refused at run time, before the model is even looked for (the directories of BASE do not exist)."""
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = sucre.build_parser().parse_args(BASE + ['--trim-outliers', '3'] + extra)
    with pytest.raises(SystemExit) as e:
        sucre.parse_args(args)
    assert '--trim-outliers' in str(e.value) and named in str(e.value)


@pytest.mark.parametrize('extra, word', [(['--trim-outliers', '0'], '--trim-outliers'), (['--trim-outliers', '-2'], '--trim-outliers'),
                                         (['--trim-outliers', 'nan'], '--trim-outliers'), (['--trim-outliers', 'inf'], '--trim-outliers'),
                                         (['--trim-outliers', '3', '--trim-rounds', '0'], '--trim-rounds'),
                                         (['--trim-rounds', '2'], '--trim-rounds')])
def test_refused_values(extra, word, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(SystemExit) as e:
        sucre.parse_args(sucre.build_parser().parse_args(BASE + extra))
    assert word in str(e.value)


def test_keywords_of_the_host_entry_points():
    import dataclasses
    import inspect
    par = inspect.signature(sucre.adam).parameters
    assert par['trim_outliers'].default is None and par['trim_rounds'].default == 1
    field = {f.name: f.default for f in dataclasses.fields(sucre._Extras)}     # what _restore_one and _restore_submit take
    assert field['trim_outliers'] is None and field['trim_rounds'] == 1
    sucre.restore_images([], None, None, fit_batch=1, trim_outliers=None, trim_rounds=1)     # accepted: no image, nothing to do
    with pytest.raises(ValueError, match='trim_outliers'):
        sucre.restore_images([], None, None, trim_outliers=-1.0)
    with pytest.raises(ValueError, match='trim_rounds'):
        sucre.restore_images([], None, None, trim_outliers=3.0, trim_rounds=0)
    with pytest.raises(ValueError, match='save_interval'):
        sucre.adam(None, None, save_dir='x', save_interval=5, trim_outliers=3.0)


def test_scratch_size():
    lib = _lib.load()
    a, b = lib.sucre_trim_scratch_bytes(52, 75, 7), lib.sucre_trim_scratch_bytes(52, 75, 64)
    assert 0 < a < b
    assert lib.sucre_trim_scratch_bytes(1080, 1920, 65) >= 8160 * 65 * 4      # one drop count per tile and view
    assert lib.sucre_trim_scratch_bytes(0, 75, 7) == 0 and b'invalid geometry' in lib.sucre_last_error()
    assert lib.sucre_trim_scratch_bytes(52, 75, 0) == 0
    assert lib.sucre_trim_scratch_bytes(52, 75, 4097) == 0


def test_trim_entry_points_validate_before_any_launch():
    """No device is needed: every call below returns before a kernel would be launched (the pointers are not memory)."""
    lib = _lib.load()
    ws, lws, out = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    plain = lambda *a: lib.sucre_trim_outliers(*a)           # noqa: E731
    ext = lambda *a: lib.sucre_trim_outliers_ext(*a)         # noqa: E731
    five = [out] * 5
    # workspace and geometry
    assert plain(None, 48, 64, 3, _lib.OBS_F32, 3.0, *five, None) == -1 and b'NULL' in lib.sucre_last_error()
    assert plain(C.c_void_p(4), 48, 64, 3, _lib.OBS_F32, 3.0, *five, None) == -1 and b'aligned' in lib.sucre_last_error()
    assert plain(ws, 0, 64, 3, _lib.OBS_F32, 3.0, *five, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
    assert plain(ws, 48, 64, 4097, _lib.OBS_F32, 3.0, *five, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
    # format
    assert plain(ws, 48, 64, 3, 7, 3.0, *five, None) == -1 and b'unknown observation format' in lib.sucre_last_error()
    # the multiple
    for k in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
        assert plain(ws, 48, 64, 3, _lib.OBS_F32, k, *five, None) == -1 and b'k_sigma' in lib.sucre_last_error(), k
        assert ext(ws, lws, 48, 64, 3, 0, k, *five, None) == -1 and b'k_sigma' in lib.sucre_last_error(), k
    # view_stats, dropped, view_dropped, thresholds, scratch: NULL, then misaligned
    for i in range(5):
        args = [out] * 5
        args[i] = None
        assert plain(ws, 48, 64, 3, _lib.OBS_U16MM, 3.0, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
        assert ext(ws, lws, 48, 64, 3, 0, 3.0, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
    for i, bad in enumerate((1028, 1026, 1028, 1026, 1032)):    # float64, int32, int64, float32, 16-byte scratch
        args = [out] * 5
        args[i] = C.c_void_p(bad)
        assert plain(ws, 48, 64, 3, _lib.OBS_F32, 3.0, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
        assert ext(ws, lws, 48, 64, 3, 0, 3.0, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
    # the extension workspace and the flags
    assert ext(ws, None, 48, 64, 3, 0, 3.0, *five, None) == -1 and b'light workspace' in lib.sucre_last_error()
    assert ext(ws, C.c_void_p(516), 48, 64, 3, 0, 3.0, *five, None) == -1 and b'aligned' in lib.sucre_last_error()
    for flags in (_lib.FIT_CLOSED_FORM, _lib.FIT_OBS_U16MM, _lib.FIT_KEEP_J, 64):
        assert ext(ws, lws, 48, 64, 3, flags, 3.0, *five, None) == -1 and b'unknown flags' in lib.sucre_last_error(), flags
    assert ext(ws, lws, 48, 64, 3, _lib.FIT_EXT_COLOUR | _lib.FIT_EXT_BOTH, 3.0, *five, None) == -1
    assert b'exclude each other' in lib.sucre_last_error()


def test_trimmed_picture_arithmetic():
    """<stem>_trimmed.png = coverage_image(dropped summed over the rounds, kept views) = 255 * sum // n_kept."""
    r1 = np.array([[0, 1, 2, 0], [3, 0, 0, 5]], np.int32)
    r2 = np.array([[0, 0, 1, 0], [0, 1, 0, 0]], np.int32)
    one = sucre.trimmed_image(r1[None], 5)
    assert one.dtype == np.uint8 and one.shape == (2, 4) and one.tolist() == [[0, 51, 102, 0], [153, 0, 0, 255]]
    two = sucre.trimmed_image(np.stack([r1, r2]), 6)
    assert two.tolist() == [[0, 42, 127, 0], [127, 42, 0, 212]]          # 255 * (r1 + r2) // 6
    assert np.array_equal(two, sucre.coverage_image(r1 + r2, 6))
    assert sucre.trimmed_image(np.zeros((1, 1, 2), np.int32), 0).tolist() == [[0, 0]]
