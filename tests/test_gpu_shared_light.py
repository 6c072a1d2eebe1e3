"""Shared water AND light (engine.HipWaterGroup over light-model restorations, sucre_light_group_*; the CLI's
--shared-water): one B, beta, gamma, cam2light, sigma for several images, a J per image, one n_obs."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import helpers
from oracle import oracle
from sucre_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RMS_BAR = 1e-4


def _light(scene, target=None, device='cuda'):
    from sucre_amd import engine
    views = engine.device_views_from_scene(scene, device)
    tgt = scene.target if target is None else int(target)
    r = engine.Restoration(scene.height, scene.width, len(views), device=device, light=True)
    r.match(views[tgt], views)
    r.fit_init(views[tgt])
    return r


def _group_fit(rs, T, closed, params0=None):
    from sucre_amd import dist as sdist
    from sucre_amd import engine
    trace = torch.zeros((T, 20), dtype=torch.float64, device='cuda')
    sdist.fit_shared_water(engine.HipWaterGroup(rs, use_closed_form=closed, trace=trace, params0=params0), T)
    torch.cuda.synchronize()
    return trace.cpu().numpy()


@pytest.mark.parametrize('closed', [False, True])
def test_light_group_of_one_equals_the_single_fit(golden, closed):
    """A group of one light image is sucre_fit_run_light: same gradient kernel, light_reduce / light_step on image 0's sums
    as they are -- bit for bit (trace, J with its NaNs, parameters)."""
    sc = golden.scene
    T = 12
    r = _light(sc)
    t1 = r.fit(T, use_closed_form=closed).cpu().numpy()
    J1, p1 = r.J().cpu().numpy(), r.params().cpu().numpy()
    from sucre_amd import engine
    views = engine.device_views_from_scene(sc, 'cuda')
    r.fit_init(views[sc.target])
    tg = _group_fit([r], T, closed)
    assert np.array_equal(tg, t1)
    assert np.array_equal(r.J().cpu().numpy(), J1, equal_nan=True) and np.array_equal(r.params().cpu().numpy(), p1)


def _composite(parts, closed):
    """Two images side by side as ONE oracle problem -- J per pixel, every parameter shared, one n_obs (sucre.py:145): the
    tied objective.  parts: (scene, target); rows below a shorter image have no observation."""
    Hc = max(sc.height for sc, _ in parts)
    Wc = sum(sc.width for sc, _ in parts)
    samples, J0s, off = [], [], 0
    for sc, tgt in parts:
        s2 = sc if tgt == sc.target else _retarget(sc, tgt)
        _, smp = helpers.oracle_scene_samples(s2)
        samples += [((np.asarray(u, np.int64) + off).astype(np.int16), v, cP, I) for u, v, cP, I in smp]
        tv = s2.views[s2.target]
        J0 = oracle.init_J(tv.rgb_u8.numpy(), tv.depth_f32().numpy())
        J0s.append(np.concatenate([J0, np.full((Hc - sc.height, sc.width, 3), np.nan, np.float32)], axis=0))
        off += sc.width
    return Hc, Wc, samples, (None if closed else np.concatenate(J0s, axis=1))


def _retarget(scene, tgt):
    import copy
    s = copy.copy(scene)
    s.target = int(tgt)
    return s


def _halves(Jo, parts):
    out, off = [], 0
    for sc, _ in parts:
        out.append(Jo[:sc.height, off:off + sc.width])
        off += sc.width
    return out


@pytest.mark.parametrize('closed', [False, True])
@pytest.mark.parametrize('sizes', ['same', 'different'])
def test_light_group_of_two_vs_the_composite_oracle_problem(golden, closed, sizes):
    """Two different images against the oracle on their side-by-side composite (the tied objective exactly), 10 iterations,
    held to the bars of test_light_model_vs_oracle_short / test_light_model_closed_form_vs_oracle."""
    sc = golden.scene
    other = synth.make_scene(80, 48, 3, seed=5)
    t0, t1 = (int(t) for t in golden['shared_targets'])
    parts = [(sc, t0), (sc, t1) if sizes == 'same' else (other, other.target)]
    T = 10
    rs = [_light(s, t) for s, t in parts]
    tr = _group_fit(rs, T, closed)
    Hc, Wc, samples, J0 = _composite(parts, closed)
    assert sum(r.n_obs() for r in rs) == sum(len(s[0]) for s in samples)
    Jo, po, to = oracle.fit_light(Hc, Wc, samples, J0, num_iter=T, use_closed_form=closed)
    assert abs(tr[0, 0] / to[0, 0] - 1) < (1e-5 if closed else 1e-6)
    assert np.abs(tr[:, 1:10] - to[:, 1:10]).max() < (5e-5 if closed else 2e-5)
    assert np.abs(tr[:, 10:] - to[:, 10:]).max() < 1e-3
    p = [r.params().cpu().numpy() for r in rs]
    assert np.array_equal(p[0], p[1]) and np.array_equal(p[0], tr[-1, 1:].astype(np.float32))
    for r, Jh in zip(rs, _halves(Jo, parts)):
        J = r.J().cpu().numpy()
        assert np.array_equal(np.isnan(J), np.isnan(Jh))
        assert helpers.rms_per_channel(J, Jh).max() < (RMS_BAR if closed else 2e-5)


@pytest.mark.parametrize('mode', ['param', 'closed'])
def test_light_group_vs_tied_reference_modules(mode):
    """Against two reference SUCRe(light_model=True) modules with B, beta, gamma, cam2light, sigma tied
    (tests/golden/shared_light_96x64.npz; 40 iterations with J as a parameter, 5 in the chaotic closed-form mode), held to
    the bars of test_light_model_vs_reference_golden."""
    fx = helpers.load_fixture('relief_96x64_n6')
    g = np.load(helpers.GOLDEN_DIR / 'shared_light_96x64.npz')
    rt = g[f'{mode}_trace']
    rs = [_light(fx.scene, t) for t in g['targets']]
    assert sum(r.n_obs() for r in rs) == int(g['n_total'])
    tr = _group_fit(rs, rt.shape[0], mode == 'closed')
    assert np.abs(tr[:, 1:10] - rt[:, 1:10]).max() < 3e-4
    assert np.abs(tr[:, 10:] - rt[:, 10:]).max() < 3e-3
    assert np.abs(tr[:, 0] / rt[:, 0] - 1).max() < 5e-3
    for r, key in zip(rs, (f'{mode}_J0', f'{mode}_J1')):
        J = r.J().cpu().numpy()
        assert np.array_equal(np.isnan(J), np.isnan(g[key]))
        assert helpers.rms_per_channel(J, g[key]).max() < RMS_BAR


def test_copies_of_one_image_are_the_one_image_problem(golden):
    """Eight copies of one image in closed-form mode: every sum is eight times the one image's and so is n_obs, so the
    trajectory is the one-image group's (to rounding) and the eight J are the same bits."""
    sc = golden.scene
    T = 10
    one = _group_fit([_light(sc)], T, True)
    rs = [_light(sc) for _ in range(8)]
    eight = _group_fit(rs, T, True)
    assert np.abs(eight[:, 1:] - one[:, 1:]).max() < 1e-6
    assert np.abs(eight[:, 0] / (8 * one[:, 0]) - 1).max() < 1e-6
    Js = [r.J().cpu().numpy() for r in rs]
    for J in Js[1:]:
        assert np.array_equal(J, Js[0], equal_nan=True)


def test_light_group_refusals(golden):
    from sucre_amd import _lib, engine
    sc = golden.scene
    views = engine.device_views_from_scene(sc, 'cuda')
    plain = engine.Restoration(sc.height, sc.width, len(views))
    plain.match(views[sc.target], views)
    plain.fit_init(views[sc.target])
    lit = _light(sc)
    with pytest.raises(NotImplementedError, match='not a mix'):
        engine.HipWaterGroup([lit, plain])
    fc = engine.Restoration(sc.height, sc.width, len(views), light=True, float_colour=True)
    with pytest.raises(NotImplementedError, match='uint8 colours'):
        engine.HipWaterGroup([fc])
    g = engine.HipWaterGroup([lit])
    g.set_n_obs_total(lit.n_obs())
    g.grad(1)
    with pytest.raises(_lib.SucreError, match='iterations run in order'):
        g.grad(1)
    # the library itself keeps the order too
    lib = lit.lib
    rc = lib.sucre_light_group_iter(ctypes.c_void_p(g.buf.data_ptr()), 1, 1, 0.05, 0.9, 0.999, 1e-8, 0, lit.n_obs(), None, None)
    assert rc == -2 and b'iterations run in order' in lib.sucre_last_error()
    torch.cuda.synchronize()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize('closed', [False, True])
def test_two_processes_equal_one_process(tmp_path, closed):
    """Two gloo ranks with one light image each (both on the box's one GPU) against one process holding both: with two
    terms the all-reduce is the in-process sum, so trace, J and parameters are the same bits."""
    T = 12
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), SUCRE_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, str(ROOT / 'tests' / 'shared_light_worker.py'), str(tmp_path),
                                       '1' if closed else '0', str(T)], env=env))
    assert [p.wait(timeout=500) for p in procs] == [0, 0]
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    assert str(r0['backend']) == 'gloo' and int(r0['world']) == 2
    fx = helpers.load_fixture('relief_96x64_n6')
    rs = [_light(fx.scene, t) for t in fx['shared_targets']]
    tr = _group_fit(rs, T, closed)
    for rk, r in zip((r0, r1), rs):
        assert np.array_equal(rk['trace'], tr)
        assert np.array_equal(rk['params'], r.params().cpu().numpy())
        assert np.array_equal(rk['J'], r.J().cpu().numpy(), equal_nan=True)


# ---- the command line -------------------------------------------------------------------------------------------------------

def _cli(args, env, out):
    cmd = [sys.executable, '-m', 'sucre_amd.sucre'] + args + ['--output-dir', str(out)]
    return subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)


def _engine_group(scene_dir, names, light, closed, T):
    """The same images through engine.HipWaterGroup directly (views culled as Image.match_images does)."""
    from sucre_amd import engine, sfm
    model = sfm.COLMAPModel(scene_dir / 'model', scene_dir / 'images', scene_dir / 'depth')
    image_list = list(model.images.values())
    rs = []
    for name in names:
        im = model[name]
        idx = im.overlapping_views(image_list, 'cuda')
        views = [image_list[i].device_view('cuda') for i in idx]
        tgt = im.device_view('cuda')
        r = engine.Restoration(im.camera.height, im.camera.width, len(views), light=light)
        r.match(tgt, views)
        r.fit_init(tgt)
        rs.append(r)
    trace = torch.zeros((T, 20 if light else 10), dtype=torch.float64, device='cuda')
    from sucre_amd import dist as sdist
    sdist.fit_shared_water(engine.HipWaterGroup(rs, use_closed_form=closed, trace=trace), T)
    return [r.J().cpu().numpy() for r in rs], trace.cpu().numpy()


@pytest.mark.timeout(900)
@pytest.mark.parametrize('light', [False, True], ids=['plain', 'light'])
@pytest.mark.parametrize('closed', [False, True], ids=['param', 'closed'])
def test_cli_shared_water(tmp_path, light, closed):
    scene_dir = tmp_path / 'scene'
    survey = synth.make_survey(160, 120, 3, 2, seed=4)
    synth.write_to_disk(survey, scene_dir)
    names = sorted(v.name for v in survey.views)
    T = 12
    base = ['--image-dir', str(scene_dir / 'images'), '--depth-dir', str(scene_dir / 'depth'), '--model-dir', str(scene_dir / 'model'),
            '--num-iter', str(T)] + (['--light-model'] if light else []) + (['--use-closed-form'] if closed else [])
    clean = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    clean['PYTHONPATH'] = str(ROOT) + os.pathsep + clean.get('PYTHONPATH', '')
    # every image of the request in one shared fit, next to today's per-image run of the same request
    p = _cli(base + ['--image-ids', '1', '7', '--shared-water'], clean, tmp_path / 'shared')
    so, se = p.communicate(timeout=600)
    assert p.returncode == 0, se[-2000:]
    q = _cli(base + ['--image-ids', '1', '7'], clean, tmp_path / 'plain')
    qo, qe = q.communicate(timeout=600)
    assert q.returncode == 0, qe[-2000:]
    files = sorted(f.name for f in (tmp_path / 'shared').iterdir())
    assert files == sorted([f.name for f in (tmp_path / 'plain').iterdir()] + ['shared_water.pt'])
    sw = torch.load(tmp_path / 'shared' / 'shared_water.pt')
    keys = {'B', 'beta', 'gamma'} | ({'cam2light', 'sigma'} if light else set())
    assert set(sw) == keys | {'trace', 'images'} and sw['images'] == names
    assert sw['trace'].dtype == torch.float64 and tuple(sw['trace'].shape) == (T, 20 if light else 10)
    assert sum(ln.startswith('iter: ') for ln in so.splitlines()) == T
    Js, trace = _engine_group(scene_dir, names, light, closed, T)
    assert np.array_equal(sw['trace'].numpy(), trace)
    for name, J in zip(names, Js):
        pt = torch.load((tmp_path / 'shared' / name).with_suffix('.pt'))
        assert set(pt) - {'J'} == keys
        for k in keys:
            assert torch.equal(pt[k], sw[k]), (name, k)
        assert np.array_equal(pt['J'].numpy(), J, equal_nan=True), name
    # refused before any work: no output directory content
    for extra in (['--image-scale', '0.5'], ['--save-interval', '5']):
        r = _cli(base + ['--image-ids', '1', '7', '--shared-water'] + extra, clean, tmp_path / 'refused')
        ro, re_ = r.communicate(timeout=300)
        assert r.returncode != 0 and extra[0] in re_ and '--shared-water' in re_
        assert not (tmp_path / 'refused').exists() or not any((tmp_path / 'refused').iterdir())


@pytest.mark.timeout(900)
@pytest.mark.parametrize('light', [False, True], ids=['plain', 'light'])
@pytest.mark.parametrize('closed', [False, True], ids=['param', 'closed'])
def test_cli_shared_water_two_ranks_equal_one_process(tmp_path, light, closed):
    """Two images under WORLD_SIZE=2 (one each; gloo on the box's one GPU) against the one-process run.  With the light model
    bit for bit: the light group reduces every image to float64 sums and adds the images in float64, so with two terms the
    all-reduce is the in-process sum.  The plain-water group (fit.hip, group_iter_kernel) adds the images of a rank inside its
    single launch, in float32 per workgroup, before the float64 reduction: one process with two images groups the additions
    differently from two ranks with one each, so the plain runs are held to 1e-6 in the parameters instead."""
    scene_dir = tmp_path / 'scene'
    survey = synth.make_survey(160, 120, 3, 2, seed=4)
    synth.write_to_disk(survey, scene_dir)
    base = ['--image-dir', str(scene_dir / 'images'), '--depth-dir', str(scene_dir / 'depth'), '--model-dir', str(scene_dir / 'model'),
            '--num-iter', '12', '--image-ids', '2', '4', '--shared-water'] + (['--light-model'] if light else []) + \
        (['--use-closed-form'] if closed else [])
    clean = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    clean['PYTHONPATH'] = str(ROOT) + os.pathsep + clean.get('PYTHONPATH', '')
    one = _cli(base, clean, tmp_path / 'one')
    oo, oe = one.communicate(timeout=600)
    assert one.returncode == 0, oe[-2000:]
    port = _free_port()
    procs = [_cli(base, dict(clean, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                             MASTER_PORT=str(port), SUCRE_DIST_BACKEND='gloo'), tmp_path / 'two') for k in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    files_one = sorted(f.name for f in (tmp_path / 'one').iterdir())
    assert files_one == sorted(f.name for f in (tmp_path / 'two').iterdir()) and 'shared_water.pt' in files_one
    for name in files_one:
        if not name.endswith('.pt'):
            continue
        sa, sb = torch.load(tmp_path / 'one' / name), torch.load(tmp_path / 'two' / name)
        assert set(sa) == set(sb)
        for k in sa:
            if k == 'images':
                assert sa[k] == sb[k]
                continue
            assert torch.equal(torch.isnan(sa[k]), torch.isnan(sb[k])), (name, k)
            if light:
                assert torch.equal(torch.nan_to_num(sa[k]), torch.nan_to_num(sb[k])), (name, k)
            else:
                d = _rel_trace(sa[k], sb[k]) if k == 'trace' else \
                    (torch.nan_to_num(sa[k]).double() - torch.nan_to_num(sb[k]).double()).abs().max().item()
                assert d < (1e-5 if k == 'J' else 1e-6), (name, k, d)


def _rel_trace(a, b):
    """Largest difference of two logs: relative in the cost column, absolute in the parameters."""
    a, b = a.double(), b.double()
    return max(float((a[:, 0] / b[:, 0] - 1).abs().max()), float((a[:, 1:] - b[:, 1:]).abs().max()))
