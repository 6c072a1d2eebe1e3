"""CPU tier of the per-view gain compensation: numpy restatements of the estimate (float64) and of the apply rule (float32) that
the GPU tests import, the three flags, the combinations refused before any work, host-side validation of sucre_view_gains* and
sucre_apply_view_gains* (nothing is launched) and the scratch size."""
import ctypes as C

import numpy as np
import pytest

from sucre_amd import _lib, sucre

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


# ---- the restatements -------------------------------------------------------------------------------------------------------
def gains_from_sums(sums, kept, limit=2.0):
    """(gains (n,3) float64, inv (n,3) float32) from the (n,7) table {n, sum I Ihat [3], sum Ihat^2 [3]}: g = S_IIhat / S_IhatIhat
    clamped to [1 / limit, limit]; g = 1 exactly for a view that is not kept, has no observation, or whose S_IhatIhat or quotient
    is not finite and positive."""
    sums = np.asarray(sums, np.float64)
    gains = np.ones((len(sums), 3), np.float64)
    for k in range(len(sums)):
        if not kept[k] or not sums[k, 0] > 0:
            continue
        for c in range(3):
            sih, shh = sums[k, 1 + c], sums[k, 4 + c]
            if not (np.isfinite(shh) and shh > 0):
                continue
            with np.errstate(all='ignore'):
                q = sih / shh
            if np.isfinite(q) and q > 0:
                gains[k, c] = min(max(q, 1.0 / limit), limit)
    return gains, (1.0 / gains).astype(np.float32)


def gain_sums(I, Ihat):
    """One view's row of the table from its observations' I and Ihat, (n,3) each, in float64; a term whose Ihat is not finite
    contributes to neither sum."""
    I, Ihat = np.asarray(I, np.float64), np.asarray(Ihat, np.float64)
    ok = np.isfinite(Ihat)
    h, i = np.where(ok, Ihat, 0.0), np.where(ok, I, 0.0)
    return np.array([len(I), *(i * h).sum(axis=0), *(h * h).sum(axis=0)], np.float64)


def apply_u8(rgb_u8, inv):
    """uint8 colours (n,3) of one view times inv (3,) float32: min(255, rint(float32(k) * inv_c)), one float32 multiply, round
    half to even.  Returns (corrected uint8, how many values met the clamp)."""
    x = np.rint(np.asarray(rgb_u8).astype(np.float32) * np.asarray(inv, np.float32)[None, :])
    assert x.dtype == np.float32
    return np.minimum(x, np.float32(255.0)).astype(np.uint8), int((x > 255.0).sum())


def apply_f32(I, inv):
    """float32 colours (n,3) of one view times inv (3,) float32: one float32 multiply, no clamp."""
    out = np.asarray(I, np.float32) * np.asarray(inv, np.float32)[None, :]
    assert out.dtype == np.float32
    return out


def test_restatement_rules():
    sums = np.array([[10, 8.0, 9.0, 10.0, 10.0, 10.0, 10.0],      # 0.8, 0.9, 1.0
                     [10, 30.0, 1.0, 10.0, 10.0, 10.0, 10.0],     # clamped to 2 and 0.5
                     [0, 0, 0, 0, 0, 0, 0],                       # nothing observed
                     [10, 8.0, 8.0, 8.0, 10.0, 10.0, 10.0],       # not kept
                     [10, 5.0, -5.0, 5.0, 0.0, 10.0, np.inf]], np.float64)
    g, inv = gains_from_sums(sums, [True, True, True, False, True])
    assert g[0].tolist() == [0.8, 0.9, 1.0] and g[1].tolist() == [2.0, 0.5, 1.0]
    assert g[2].tolist() == g[3].tolist() == g[4].tolist() == [1.0, 1.0, 1.0]
    assert inv.dtype == np.float32 and inv[1].tolist() == [0.5, 2.0, 1.0] and inv[0, 0] == np.float32(1 / 0.8)
    assert gains_from_sums(sums, [True] * 5, limit=1.1)[0][0].tolist() == [1 / 1.1, 1 / 1.1, 1.0]
    row = gain_sums([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0]], [[0.25, np.nan, 0.5], [0.5, 0.5, np.inf]])
    assert row.tolist() == [2, 0.625, 0.5, 0.25, 0.3125, 0.25, 0.25]
    # ties go to even, the clamp counts what it cuts, 1.0 is the identity
    out, clipped = apply_u8([[1, 3, 5], [200, 255, 128]], [0.5, 0.5, 2.0])
    assert out.tolist() == [[0, 2, 10], [100, 128, 255]] and clipped == 1
    out, clipped = apply_u8(np.arange(256, dtype=np.uint8).repeat(3).reshape(256, 3), [1.0, 1.0, 1.0])
    assert np.array_equal(out[:, 0], np.arange(256)) and clipped == 0
    assert apply_f32([[0.5, 2.0, 0.1]], [1.5, 1.5, 1.0]).tolist() == [[0.75, 3.0, float(np.float32(0.1))]]


# ---- flags ------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_leave_no_trace_when_absent():
    p = sucre.build_parser()
    off = p.parse_args(BASE)
    assert not {'view_gains', 'gain_rounds', 'gain_limit'} & set(vars(off))
    on = p.parse_args(BASE + ['--view-gains'])
    assert on.view_gains is True and 'gain_rounds' not in vars(on) and 'gain_limit' not in vars(on)
    assert vars(off) == {k: v for k, v in vars(on).items() if k != 'view_gains'}
    two = p.parse_args(['--gain-rounds', '2'] + BASE + ['--view-gains', '--gain-limit', '1.5', '--save-quality'])
    assert two.gain_rounds == 2 and two.gain_limit == 1.5 and two.save_quality is True
    text = p.format_help()
    assert '--view-gains' in text and '--gain-rounds N' in text and '--gain-limit L' in text


@pytest.mark.parametrize('extra, named', [(['--shared-water'], '--shared-water'), (['--save-interval', '5'], '--save-interval'),
                                          (['--trim-outliers', '3'], '--trim-outliers'),
                                          (['--apply-water', 'nowhere/water.pt'], '--apply-water')])
def test_refused_combinations_name_the_flag(extra, named, monkeypatch):
    """Refused at run time, before any file is opened (neither the directories of BASE nor the water file exist)."""
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = sucre.build_parser().parse_args(BASE + ['--view-gains'] + extra)
    with pytest.raises(SystemExit) as e:
        sucre.parse_args(args)
    assert '--view-gains' in str(e.value) and named in str(e.value)


@pytest.mark.parametrize('extra, word', [(['--view-gains', '--gain-rounds', '0'], '--gain-rounds'),
                                         (['--view-gains', '--gain-rounds', '-1'], '--gain-rounds'),
                                         (['--view-gains', '--gain-limit', '0.9'], '--gain-limit'),
                                         (['--view-gains', '--gain-limit', 'nan'], '--gain-limit'),
                                         (['--view-gains', '--gain-limit', 'inf'], '--gain-limit'),
                                         (['--gain-rounds', '2'], '--gain-rounds'), (['--gain-limit', '2'], '--gain-limit')])
def test_refused_values(extra, word, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(SystemExit) as e:
        sucre.parse_args(sucre.build_parser().parse_args(BASE + extra))
    assert word in str(e.value)


def test_keywords_of_the_host_entry_points():
    import dataclasses
    import inspect
    par = inspect.signature(sucre.adam).parameters
    assert par['view_gains'].default is False and par['gain_rounds'].default == 1 and par['gain_limit'].default == 2.0
    field = {f.name: f.default for f in dataclasses.fields(sucre._Extras)}     # what _restore_one and _restore_submit take
    assert field['view_gains'] is False and field['gain_rounds'] == 1 and field['gain_limit'] == 2.0
    sucre.restore_images([], None, None, fit_batch=1, view_gains=False, gain_rounds=1, gain_limit=2.0)     # accepted: no image
    assert 'view_gains' not in inspect.signature(sucre.restore_image).parameters      # the reference's signature stays
    with pytest.raises(ValueError, match='gain_rounds'):
        sucre.restore_images([], None, None, view_gains=True, gain_rounds=0)
    for limit in (0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='gain_limit'):
            sucre.restore_images([], None, None, view_gains=True, gain_limit=limit)
    with pytest.raises(ValueError, match='trim_outliers'):
        sucre.restore_images([], None, None, view_gains=True, trim_outliers=3.0)
    with pytest.raises(ValueError, match='save_interval'):
        sucre.adam(None, None, save_dir='x', save_interval=5, view_gains=True)
    with pytest.raises(ValueError, match='trim_outliers'):
        sucre.adam(None, None, view_gains=True, trim_outliers=3.0)
    sucre._Extras(view_gains=False, gain_rounds=0, gain_limit=0.5).checked()      # without view_gains the other two are not looked at


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(52, 75), (32, 48), (1, 1), (250, 272), (1080, 1920)])
def test_scratch_size_is_positive_and_never_shrinks_with_the_view_count(H, W):
    lib = _lib.load()
    sizes = [lib.sucre_gain_scratch_bytes(H, W, n) for n in range(1, 330)]
    assert sizes[0] > 0
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    assert sizes[64] >= tiles * 65 * 7 * 4        # seven float32 per tile and view


def test_scratch_size_of_a_bad_geometry():
    lib = _lib.load()
    assert lib.sucre_gain_scratch_bytes(0, 75, 7) == 0 and b'invalid geometry' in lib.sucre_last_error()
    assert lib.sucre_gain_scratch_bytes(52, 75, 0) == 0
    assert lib.sucre_gain_scratch_bytes(52, 75, 4097) == 0


def test_gain_entry_points_validate_before_any_launch():
    """No device is needed: every call below returns before a kernel would be launched (the pointers are not memory)."""
    lib = _lib.load()
    ws, lws, out = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    est = lambda *a: lib.sucre_view_gains(*a)                 # noqa: E731
    est_x = lambda *a: lib.sucre_view_gains_ext(*a)           # noqa: E731
    app = lambda *a: lib.sucre_apply_view_gains(*a)           # noqa: E731
    app_x = lambda *a: lib.sucre_apply_view_gains_ext(*a)     # noqa: E731
    four, three = [out] * 4, [out] * 3
    # workspace and geometry
    assert est(None, 48, 64, 3, _lib.OBS_F32, 2.0, *four, None) == -1 and b'NULL' in lib.sucre_last_error()
    assert app(None, 48, 64, 3, *three, None) == -1 and b'NULL' in lib.sucre_last_error()
    assert est(C.c_void_p(4), 48, 64, 3, _lib.OBS_F32, 2.0, *four, None) == -1 and b'aligned' in lib.sucre_last_error()
    assert app(C.c_void_p(4), 48, 64, 3, *three, None) == -1 and b'aligned' in lib.sucre_last_error()
    for H, n in ((0, 3), (48, 4097), (48, 0)):
        assert est(ws, H, 64, n, _lib.OBS_F32, 2.0, *four, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
        assert est_x(ws, lws, H, 64, n, 0, 2.0, *four, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
        assert app(ws, H, 64, n, *three, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
        assert app_x(ws, lws, H, 64, n, 0, *three, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
    # format
    assert est(ws, 48, 64, 3, 7, 2.0, *four, None) == -1 and b'unknown observation format' in lib.sucre_last_error()
    # the limit
    for limit in (0.0, 0.999, -2.0, float('nan'), float('inf'), -float('inf')):
        assert est(ws, 48, 64, 3, _lib.OBS_F32, limit, *four, None) == -1 and b'limit' in lib.sucre_last_error(), limit
        assert est_x(ws, lws, 48, 64, 3, 0, limit, *four, None) == -1 and b'limit' in lib.sucre_last_error(), limit
    # gains, inv, sums, scratch: NULL, then misaligned
    for i in range(4):
        args = [out] * 4
        args[i] = None
        assert est(ws, 48, 64, 3, _lib.OBS_U16MM, 2.0, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
        assert est_x(ws, lws, 48, 64, 3, 0, 2.0, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
    for i, bad in enumerate((1028, 1026, 1028, 1032)):          # float64, float32, float64, 16-byte scratch
        args = [out] * 4
        args[i] = C.c_void_p(bad)
        assert est(ws, 48, 64, 3, _lib.OBS_F32, 1.0, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
        assert est_x(ws, lws, 48, 64, 3, 0, 1.0, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
    # inv, view_clipped, scratch: NULL, then misaligned
    for i in range(3):
        args = [out] * 3
        args[i] = None
        assert app(ws, 48, 64, 3, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
        assert app_x(ws, lws, 48, 64, 3, 0, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
    for i, bad in enumerate((1026, 1028, 1032)):                # float32, int64, 16-byte scratch
        args = [out] * 3
        args[i] = C.c_void_p(bad)
        assert app(ws, 48, 64, 3, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
        assert app_x(ws, lws, 48, 64, 3, 0, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
    # the extension workspace and the flags
    assert est_x(ws, None, 48, 64, 3, 0, 2.0, *four, None) == -1 and b'light workspace' in lib.sucre_last_error()
    assert app_x(ws, None, 48, 64, 3, 0, *three, None) == -1 and b'light workspace' in lib.sucre_last_error()
    assert est_x(ws, C.c_void_p(516), 48, 64, 3, 0, 2.0, *four, None) == -1 and b'aligned' in lib.sucre_last_error()
    for flags in (_lib.FIT_CLOSED_FORM, _lib.FIT_OBS_U16MM, _lib.FIT_KEEP_J, 64):
        assert est_x(ws, lws, 48, 64, 3, flags, 2.0, *four, None) == -1 and b'unknown flags' in lib.sucre_last_error(), flags
        assert app_x(ws, lws, 48, 64, 3, flags, *three, None) == -1 and b'unknown flags' in lib.sucre_last_error(), flags
    both = _lib.FIT_EXT_COLOUR | _lib.FIT_EXT_BOTH
    assert est_x(ws, lws, 48, 64, 3, both, 2.0, *four, None) == -1 and b'exclude each other' in lib.sucre_last_error()
    assert app_x(ws, lws, 48, 64, 3, both, *three, None) == -1 and b'exclude each other' in lib.sucre_last_error()
