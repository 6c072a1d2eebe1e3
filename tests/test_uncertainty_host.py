"""CPU tier of the uncertainty pass: the float64 restatement (tests/uncertainty_ref.py) against the dense Jacobian, the host
functions engine.water_uncertainty and sucre.pooled_uncertainty, the flag, its refusals and the keywords, and host-side validation
of sucre_fit_uncertainty* (nothing is launched).

Bars.  se and sigma_J of the restatement against s^2 (J^T J)^-1 of the full Jacobian: 1e-6 relative -- a cap on a formula error,
which would miss it by orders of magnitude (measured 1.8e-9 on the one-altitude scene, 1.9e-12 on the deep one).
engine.water_uncertainty on the restatement's own sums against the restatement's cov: 1e-9 relative to se_i se_j (two inversions of
one 3x3 matrix of scaled condition number <= 3e4 in float64: about 1e-16 x 3e4)."""
import ctypes as C
import inspect
import os
import socket

import numpy as np
import pytest
import torch

import helpers
import uncertainty_ref as uref
from oracle import oracle
from sucre_amd import _lib, engine, sucre, synth

BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']


def _fitted(scene):
    _, samples = helpers.oracle_scene_samples(scene)
    tgt = scene.views[scene.target]
    J0 = oracle.init_J(tgt.rgb_u8.numpy(), tgt.depth_f32().numpy())
    J, params, _ = oracle.fit(scene.height, scene.width, samples, J0, num_iter=60)
    return uref.flatten(samples, scene.width), J, params


@pytest.fixture(scope='module', params=['one-altitude', 'deep'])
def fitted_scene(request):
    make = synth.make_scene if request.param == 'one-altitude' else synth.make_deep_scene
    scene = make(36, 20, 4, seed=3)
    (px, z, I), J, params = _fitted(scene)
    ref = uref.restatement(px, z, I, J, params, scene.height, scene.width)
    return request.param, scene, (px, z, I), J, params, ref


def test_restatement_equals_the_dense_jacobian(fitted_scene):
    label, scene, (px, z, I), J, params, ref = fitted_scene
    se, J_se = uref.dense(px, z, I, J, params, scene.height, scene.width)
    seen = ref['count'] > 0
    d_se = float(np.abs(ref['se'] / se - 1).max())
    d_J = float(np.abs(ref['J_se'][seen] / J_se[seen] - 1).max())
    print(f'{label}: restatement vs dense: se {d_se:.2e}, sigma_J {d_J:.2e} (N {ref["N"]}, P {ref["P"]}); se(B, beta, gamma) red {ref["se"][0]}')
    assert np.array_equal(np.isnan(ref['J_se']).any(axis=-1), ~seen) and np.array_equal(np.isnan(J_se).any(axis=-1), ~seen)
    assert d_se <= 1e-6 and d_J <= 1e-6


def test_one_pass_float64_holds_the_device_bar_and_float32_does_not(fitted_scene):
    """The sums the device forms, on the CPU: in float64 they meet the GPU tests' bar of 1e-9 with margin, in float32 they miss it
    by orders of magnitude -- the reason the pass is float64."""
    label, scene, (px, z, I), J, params, ref = fitted_scene
    d64 = uref.scaled_distance(uref.one_pass(px, z, I, J, params, scene.height, scene.width)['H'], ref['H'])
    d32 = uref.scaled_distance(uref.one_pass(px, z, I, J, params, scene.height, scene.width, np.float32)['H'], ref['H'])
    print(f'{label}: one-pass H against the restatement: float64 {d64:.2e}, float32 {d32:.2e}')
    assert d64 <= 1e-10
    assert d32 >= 1e-6


def test_water_uncertainty_reproduces_the_restatement(fitted_scene):
    label, scene, _, _, _, ref = fitted_scene
    res = engine.water_uncertainty(ref['sums'])
    assert res['well_posed'].all() and res['n_obs'] == ref['N'] and res['n_pixels'] == ref['P'] and res['dof'] == ref['N'] - ref['P'] - 3
    scale = np.einsum('ci,cj->cij', ref['se'], ref['se'])
    d = float(np.abs((res['cov'] - ref['cov']) / scale).max())
    print(f'{label}: water_uncertainty vs restatement cov {d:.2e}; cond {res["cond"]}; corr(B, gamma) {res["corr"][:, 0, 2]}')
    assert d <= 1e-9
    assert np.allclose(res['se'], ref['se'], rtol=1e-9, atol=0) and np.allclose(res['s2'], ref['s2'], rtol=1e-12, atol=0)
    assert np.array_equal(res['normal'], ref['H'])
    assert np.allclose(np.einsum('cii->ci', res['corr']), 1.0, atol=1e-12) and (np.abs(res['corr']) <= 1 + 1e-12).all()
    assert res['cov'].shape == (3, 3, 3) and res['se'].shape == (3, 3) and res['cond'].shape == (3,) and res['well_posed'].shape == (3,)
    assert (res['cond'] >= 1).all()
    # torch tensors are taken as well
    again = engine.water_uncertainty(torch.from_numpy(ref['sums']))
    assert np.array_equal(again['cov'], res['cov'])
    # sigma_J from the host function, on the CPU here
    J_se = engine.j_standard_error(torch.from_numpy(ref['jterms'].astype(np.float32)), torch.from_numpy(ref['count'].astype(np.int32)), res)
    assert J_se.dtype == torch.float32 and J_se.shape == (scene.height, scene.width, 3)
    seen = ref['count'] > 0
    assert np.array_equal(np.isnan(J_se.numpy()).any(axis=-1), ~seen)
    assert float(np.abs(J_se.numpy()[seen] / ref['J_se'][seen] - 1).max()) <= 1e-6


def test_not_well_posed_gives_nan_and_no_exception(fitted_scene):
    _, _, _, _, _, ref = fitted_scene
    good = ref['sums']
    # dof <= 0: as many pixels as observations
    w = good.copy(); w[1] = w[0]
    res = engine.water_uncertainty(w)
    assert res['dof'] == -3 and not res['well_posed'].any() and np.isnan(res['cov']).all() and np.isnan(res['se']).all() and np.isnan(res['s2']).all()
    w = good.copy(); w[1] = w[0] - 3
    assert engine.water_uncertainty(w)['dof'] == 0 and not engine.water_uncertainty(w)['well_posed'].any()
    # a singular H in one channel only: gamma's row and column are B's
    w = good.copy(); w[3 + 2], w[3 + 4], w[3 + 5] = w[3 + 0], w[3 + 1], w[3 + 0]
    res = engine.water_uncertainty(w)
    assert res['well_posed'].tolist() == [False, True, True] and np.isnan(res['cov'][0]).all() and np.isfinite(res['cov'][1:]).all()
    # not finite, negative diagonal, all zeros, pixels without an A
    for mutate in (lambda w: w.__setitem__(10 + 3, np.nan), lambda w: w.__setitem__(10 + 0, -1.0), lambda w: w.__setitem__(10 + 6, np.inf)):
        w = good.copy(); mutate(w)
        assert engine.water_uncertainty(w)['well_posed'].tolist() == [True, False, True]
    assert not engine.water_uncertainty(np.zeros(24))['well_posed'].any()
    w = good.copy(); w[2] = 1
    assert not engine.water_uncertainty(w)['well_posed'].any()
    w = good.copy(); w[0] = np.nan
    assert not engine.water_uncertainty(w)['well_posed'].any()
    # sigma_J of a channel that is not well posed is NaN everywhere
    w = good.copy(); w[10] = -1.0
    J_se = engine.j_standard_error(torch.from_numpy(ref['jterms'].astype(np.float32)), torch.from_numpy(ref['count'].astype(np.int32)),
                                   engine.water_uncertainty(w)).numpy()
    assert np.isnan(J_se[..., 1]).all() and np.isfinite(J_se[..., 0][ref['count'] > 0]).all()


def _pool_worker(rank, port, out):
    from sucre_amd import dist as sdist
    os.environ.update(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    sdist.COLLECTIVE_AT_WORLD_1 = True     # the all-reduce really runs
    sdist.init_process_group(backend='gloo')
    rng = np.random.default_rng(5)
    parts = [torch.from_numpy(rng.random(24)) for _ in range(3)]
    total = sucre.pooled_uncertainty(parts, group=None)
    torch.save({'parts': parts, 'total': total}, out)
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(120)
def test_pooled_uncertainty_over_a_one_rank_gloo_group(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_pool_worker, args=(port, str(tmp_path / 'pool.pt')), nprocs=1, join=True)
    got = torch.load(tmp_path / 'pool.pt')
    plain = (got['parts'][0] + got['parts'][1]) + got['parts'][2]
    assert got['total'].dtype == torch.float64 and torch.equal(got['total'], plain)
    # and without a process group
    assert torch.equal(sucre.pooled_uncertainty(got['parts']), plain)


def test_flag_parses_and_leaves_the_namespace_alone():
    p = sucre.build_parser()
    off, on = p.parse_args(BASE), p.parse_args(BASE + ['--save-uncertainty'])
    assert 'save_uncertainty' not in vars(off) and on.save_uncertainty is True
    assert vars(off) == {k: v for k, v in vars(on).items() if k != 'save_uncertainty'}
    assert '--save-uncertainty' in p.format_help()
    assert sucre._extras_of(on).save_uncertainty is True and sucre._extras_of(off).save_uncertainty is False


@pytest.mark.parametrize('other', [['--light-model'], ['--apply-water', 'w.pt'], ['--check-consistency', 'd'], ['--mosaic', 'd']],
                         ids=['light-model', 'apply-water', 'check-consistency', 'mosaic'])
def test_refusals_name_both_flags(other, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)            # nothing is opened: the directories of BASE do not exist
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        monkeypatch.delenv(k, raising=False)
    if other[0] == '--apply-water':        # (that mode reads its water file before anything else of the request)
        torch.save({'B': torch.full((3, 1), 0.1), 'beta': torch.full((3, 1), 0.1), 'gamma': torch.full((3, 1), 0.1)}, tmp_path / 'w.pt')
    args = sucre.build_parser().parse_args(BASE + ['--save-uncertainty'] + other)
    with pytest.raises(SystemExit) as e:
        sucre.parse_args(args)
    text = str(e.value)
    assert '--save-uncertainty' in text and other[0] in text, text


def test_extras_field_and_keywords():
    import dataclasses
    field = {f.name: f.default for f in dataclasses.fields(sucre._Extras)}
    assert field['save_uncertainty'] is False
    assert inspect.signature(sucre.adam).parameters['save_uncertainty'].default is False
    assert 'save_uncertainty' not in inspect.signature(sucre.restore_image).parameters      # the reference's signature stays
    kw = {'save_uncertainty': True, 'lr': 0.05}
    extras = sucre._Extras(**{f.name: kw.pop(f.name) for f in dataclasses.fields(sucre._Extras) if f.name in kw}).checked()   # restore_images' line
    assert extras.save_uncertainty is True and kw == {'lr': 0.05}


def test_uncertainty_image_mapping():
    J_se = np.full((1, 4, 3), np.nan, np.float32)
    J_se[0, 1] = 0.1                      # 255 * 0.4 = 102
    J_se[0, 2] = [0.0, 0.0, 0.3]          # sqrt(0.09 / 3) = 0.1732 -> 176.7
    J_se[0, 3] = 1.0                      # clipped
    assert sucre.uncertainty_image(J_se).tolist() == [[0, 102, 176, 255]]


def test_scratch_size_grows_with_the_tiles():
    lib = _lib.load()
    a, b = lib.sucre_uncertainty_scratch_bytes(52, 75, 7), lib.sucre_uncertainty_scratch_bytes(52, 81, 7)
    assert 0 < a < b and a == 5 * 4 * 24 * 8 and b == 6 * 4 * 24 * 8          # 24 float64 words per tile
    assert lib.sucre_uncertainty_scratch_bytes(0, 75, 7) == 0 and b'invalid geometry' in lib.sucre_last_error()
    assert lib.sucre_uncertainty_scratch_bytes(52, 75, 0) == 0
    assert lib.sucre_uncertainty_scratch_bytes(52, 75, 4097) == 0
    assert _lib.UNCERTAINTY_WORDS == 24


def test_entry_points_validate_before_any_launch():
    lib = _lib.load()
    ws, lws, out = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    plain = lambda *a: lib.sucre_fit_uncertainty(*a)           # noqa: E731
    ext = lambda *a: lib.sucre_fit_uncertainty_ext(*a)         # noqa: E731
    colour = _lib.FIT_EXT_COLOUR
    assert plain(None, 48, 64, 3, _lib.OBS_F32, out, out, out, out, None) == -1 and b'NULL' in lib.sucre_last_error()
    assert plain(C.c_void_p(4), 48, 64, 3, _lib.OBS_F32, out, out, out, out, None) == -1 and b'aligned' in lib.sucre_last_error()
    assert plain(ws, 0, 64, 3, _lib.OBS_F32, out, out, out, out, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
    assert plain(ws, 48, 64, 0, _lib.OBS_F32, out, out, out, out, None) == -1 and b'invalid geometry' in lib.sucre_last_error()
    assert plain(ws, 48, 64, 3, 7, out, out, out, out, None) == -1 and b'unknown observation format' in lib.sucre_last_error()
    for i in range(4):
        args = [out] * 4
        args[i] = None
        assert plain(ws, 48, 64, 3, _lib.OBS_U16MM, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
        assert ext(ws, lws, 48, 64, 3, colour, *args, None) == -1 and b'NULL' in lib.sucre_last_error(), i
    for i, bad in enumerate((1026, 1032, 1028, 1032)):          # int32, float4, float64, 16-byte scratch
        args = [out] * 4
        args[i] = C.c_void_p(bad)
        assert plain(ws, 48, 64, 3, _lib.OBS_F32, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
        assert ext(ws, lws, 48, 64, 3, colour, *args, None) == -1 and b'aligned' in lib.sucre_last_error(), i
    assert ext(ws, None, 48, 64, 3, colour, out, out, out, out, None) == -1 and b'light workspace' in lib.sucre_last_error()
    assert ext(None, lws, 48, 64, 3, colour, out, out, out, out, None) == -1
    # the light model is named as not built
    for flags in (0, _lib.FIT_EXT_BOTH):
        assert ext(ws, lws, 48, 64, 3, flags, out, out, out, out, None) == -1 and b'light model' in lib.sucre_last_error(), flags
    for flags in (_lib.FIT_CLOSED_FORM, _lib.FIT_KEEP_J, 64):
        assert ext(ws, lws, 48, 64, 3, flags, out, out, out, out, None) == -1 and b'unknown flags' in lib.sucre_last_error(), flags
    assert ext(ws, lws, 48, 64, 3, colour | _lib.FIT_EXT_BOTH, out, out, out, out, None) == -1
