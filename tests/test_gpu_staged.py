"""The yields in the chunk arithmetic of the J-parameter kernels (csrc/fit.hip, grad_terms' kYield; csrc/experiment.h
SUCRE_STAGED_TERMS): three s_nop per observation-channel of a full chunk, which move no value.  Every value keeps its operations and
every accumulator the sequence of its products, so the bar is BIT EQUALITY of everything a fit leaves behind -- J and the moments
of every strip, the nine parameters and theirs, ``J()`` and the trace -- between the product library and the ``unstaged`` variant
(SUCRE_STAGED_TERMS=0: the kernels until round 12), built once per session into a temporary directory.  Each library runs
tests/staged_worker.py in a fresh child process, selected with ``SUCRE_HIP_LIB``."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

import helpers
import staged_worker

pytestmark = pytest.mark.gpu

ROOT = Path(helpers.ROOT)
DRIVERS = ('paired', 'unpaired', 'group', 'batch0', 'batch1')


def _fits(lib=None):
    env = dict(os.environ)
    env.pop('SUCRE_HIP_LIB', None)
    if lib is not None:
        env['SUCRE_HIP_LIB'] = str(lib)
    run = subprocess.run([sys.executable, str(ROOT / 'tests' / 'staged_worker.py')], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    used = [ln.split(' ', 1)[1] for ln in lines if ln.startswith('LIB ')]
    assert used == [str(lib if lib is not None else ROOT / 'sucre_amd' / 'libsucre_hip.so')], used
    return {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith('FIT ')}


@pytest.fixture(scope='session')
def both(tmp_path_factory):
    """({key: digests} of the product library, the same of the unstaged variant)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert Path(hipcc).exists(), 'the variant needs hipcc'
    tmp = tmp_path_factory.mktemp('unstaged')
    shutil.copytree(ROOT / 'sucre_amd' / 'csrc', tmp / 'sucre_amd' / 'csrc',
                    ignore=shutil.ignore_patterns('*.o', '*.s', '*.rpt', '*.so'))
    shutil.copytree(ROOT / 'include', tmp / 'include')
    out = subprocess.run(['make', '-C', str(tmp / 'sucre_amd' / 'csrc'), '-j16', f'HIPCC={hipcc}', 'VARIANT=unstaged', 'EXTRA=-DSUCRE_STAGED_TERMS=0'],
                         capture_output=True, text=True)
    lib = tmp / 'sucre_amd' / 'libsucre_hip_unstaged.so'
    assert out.returncode == 0 and lib.exists(), (out.stdout[-1500:], out.stderr[-1500:])
    return _fits(), _fits(lib)


def test_every_fit_ran_in_both_builds(both):
    new, old = both
    want = {f'{c}/{f}/{p}/{d}' for c in staged_worker.CASES for f in staged_worker.FORMATS for p, _ in staged_worker.PARAMS for d in DRIVERS}
    assert set(new) == want and set(old) == want
    assert all(len(v) == 4 for v in new.values())


@pytest.mark.parametrize('fmt', staged_worker.FORMATS)
@pytest.mark.parametrize('cid', staged_worker.CASES)
def test_the_product_keeps_every_bit_of_the_unstaged_build(both, cid, fmt):
    """Scaled-B form and fallback; in pairs, one launch per iteration, a group of one, and a batch launch of two images."""
    new, old = both
    for pname, _ in staged_worker.PARAMS:
        for d in DRIVERS:
            key = f'{cid}/{fmt}/{pname}/{d}'
            for what, a, b in zip(('state', 'parameters', 'J', 'trace'), new[key], old[key]):
                assert a == b, (key, what, 'differs between the product and the unstaged build')


def test_the_fits_depend_on_what_they_should(both):
    """The digests tell fits apart (a worker that hashed nothing would pass the comparison): forms, stores and cases differ,
    while the paired and the unpaired fit of one build agree (tests/test_gpu_paired.py)."""
    new, _ = both
    assert new['stair/f32/scaled/paired'] == new['stair/f32/scaled/unpaired']
    assert new['stair/f32/scaled/paired'][2] != new['stair/f32/fallback/paired'][2]
    assert new['stair/f32/scaled/paired'][2] != new['stair/u16mm/scaled/paired'][2]
    assert new['eq4/f32/scaled/paired'][2] != new['eq5/f32/scaled/paired'][2]
