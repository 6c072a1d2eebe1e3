"""Host-side checks of the B-scaled fit arithmetic (csrc/fit_math.h scaled_b_ok, csrc/experiment.h SUCRE_SCALED_B): the
predicate's edges, the committed goldens' trajectories inside its window, and the knob's other build."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers

ROOT = Path(helpers.ROOT)
CSRC = ROOT / 'sucre_amd' / 'csrc'


def _hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if Path('/opt/rocm/bin/hipcc').exists() else None)


@pytest.fixture(scope='module')
def check_exes(tmp_path_factory):
    """tests/native/scaled_b_check.cpp, host code only (no device pass, no GPU call), for the product and for SUCRE_SCALED_B=0."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('no hipcc on this machine')
    out = {}
    d = tmp_path_factory.mktemp('scaled_b')
    for name, flags in (('product', []), ('unscaled', ['-DSUCRE_SCALED_B=0'])):
        exe = d / f'scaled_b_{name}'
        build = subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', f'-I{CSRC}', *flags,
                                str(ROOT / 'tests' / 'native' / 'scaled_b_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        out[name] = exe
    return out


@pytest.mark.parametrize('name', ['product', 'unscaled'])
def test_predicate_edges(check_exes, name):
    run = subprocess.run([str(check_exes[name])], capture_output=True, text=True)
    assert run.returncode == 0 and ' 0 violations' in run.stdout, (name, run.stdout, run.stderr)


def test_every_golden_trajectory_stays_inside_the_window(check_exes, tmp_path):
    """Every B the reference's stored traces visit (and fit_init's 0.1, from which they start) satisfies the predicate: the
    fixtures, like the benchmark, run the scaled form in every launch."""
    triples = [np.full((1, 3), 0.1, np.float32)]
    n_traces = 0
    for f in sorted((ROOT / 'tests' / 'golden').rglob('*.npz')):
        with np.load(f) as d:
            for k in d.files:
                if 'trace' in k and d[k].ndim == 2 and d[k].shape[1] >= 10:
                    triples.append(np.ascontiguousarray(d[k][:, 1:4], np.float32))
                    n_traces += 1
                elif ('params' in k) and d[k].shape in ((9,), (19,)):      # stored fit parameters: B first
                    triples.append(np.ascontiguousarray(np.asarray(d[k]).reshape(-1)[:3][None], np.float32))
    assert n_traces >= 40
    allB = np.concatenate(triples)
    assert np.isfinite(allB).all()
    path = tmp_path / 'B.f32'
    allB.tofile(path)
    run = subprocess.run([str(check_exes['product']), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and f'{len(allB)} triples, 0 outside' in run.stdout, (run.stdout, run.stderr, np.abs(allB).min(), np.abs(allB).max())


def test_unscaled_build_compiles():
    """SUCRE_SCALED_B=0 (tools/exp/ab_vs.sh, ab_bench.sh unscaledb) through the product Makefile's own rule, so that the no-scratch
    check applies to it; the object goes to a scratch suffix and is removed."""
    if _hipcc() is None:
        pytest.skip('no hipcc on this machine')
    name = 'tunscaledb'
    try:
        out = subprocess.run(['make', '-C', str(CSRC), f'VARIANT={name}', 'EXTRA=-DSUCRE_SCALED_B=0', f'fit_{name}.o'], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
        assert (CSRC / f'fit_{name}.o').exists()
    finally:
        for f in CSRC.glob(f'*_{name}.*'):
            f.unlink()
