"""The straight run of unmasked full chunks in the J-parameter kernels of the headline (csrc/fit.hip: stream_strips' straight_run,
read_chunk_z24, accumulate_chunk_z24; csrc/experiment.h SUCRE_STRAIGHT_CHUNKS): the consumer side of one loop, unrolled by the ring
for the 24-bit range-code store.  No value changes its operations or their order, so the bar is BIT EQUALITY of everything a fit
leaves behind -- J and the moments of every strip, the nine parameters and theirs, ``J()`` and the trace -- between the product
library and the ``generic`` variant (SUCRE_STRAIGHT_CHUNKS=0: the kernels until round 13), built once per session into a temporary
directory.  Each library runs tests/straight_worker.py in a fresh child process, selected with ``SUCRE_HIP_LIB``: three tiny
synthetic scenes, five and six iterations (the odd one ends with the one-launch kernel), in pairs of launches and one by one, and
two restorations in flight on two streams.

The unrolled loop has three entries and three ways out.  The worker reads every wave's strips back from the workspace's plan, and
the scenes count only if every kernel -- L, F, the one-launch kernel -- takes runs that start at every ring slot with every
remainder, and meets a strip without a run at all."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

import helpers
import straight_worker

pytestmark = pytest.mark.gpu

ROOT = Path(helpers.ROOT)
STORE_Z24 = 2   # sucre_amd/_lib.py STORE_Z24


def _run(where, lib=None):
    env = dict(os.environ)
    env.pop('SUCRE_HIP_LIB', None)
    if lib is not None:
        env['SUCRE_HIP_LIB'] = str(lib)
    run = subprocess.run([sys.executable, str(ROOT / 'tests' / 'straight_worker.py'), str(where)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    lines = [ln.split() for ln in run.stdout.splitlines()]
    used = [ln[1] for ln in lines if ln[0] == 'LIB']
    assert used == [str(lib if lib is not None else ROOT / 'sucre_amd' / 'libsucre_hip.so')], used
    return {
        'fits': {ln[1]: ln[2:] for ln in lines if ln[0] == 'FIT'},
        'store': {int(ln[1]): int(ln[2]) for ln in lines if ln[0] == 'STORE'},
        'runs': {(int(ln[1]), ln[2]): {tuple(int(x) for x in p.split(',')) for p in ln[3:]} for ln in lines if ln[0] == 'RUNS'},
        'nu': {int(ln[1]): (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == 'NU'},
    }


@pytest.fixture(scope='session')
def both(tmp_path_factory):
    """(what the worker printed with the product library, the same with the generic variant)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert Path(hipcc).exists(), 'the variant needs hipcc'
    assert shutil.which('g++') is not None, 'the plan helper needs g++'
    tmp = tmp_path_factory.mktemp('generic')
    shutil.copytree(ROOT / 'sucre_amd' / 'csrc', tmp / 'sucre_amd' / 'csrc',
                    ignore=shutil.ignore_patterns('*.o', '*.s', '*.rpt', '*.so'))
    shutil.copytree(ROOT / 'include', tmp / 'include')
    where = tmp / 'plan_where'
    out = subprocess.run(['g++', '-std=c++17', '-O1', f'-I{ROOT / "sucre_amd" / "csrc"}', f'-I{ROOT / "include"}',
                          str(ROOT / 'tests' / 'native' / 'plan_where.cpp'), '-o', str(where)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run(['make', '-C', str(tmp / 'sucre_amd' / 'csrc'), '-j16', f'HIPCC={hipcc}', 'VARIANT=generic', 'EXTRA=-DSUCRE_STRAIGHT_CHUNKS=0'],
                         capture_output=True, text=True)
    lib = tmp / 'sucre_amd' / 'libsucre_hip_generic.so'
    assert out.returncode == 0 and lib.exists(), (out.stdout[-1500:], out.stderr[-1500:])
    return _run(where), _run(where, lib)


def _keys():
    keys = [f'{n}/T{T}/{p}' for n in straight_worker.NEIGHBOURS for T in straight_worker.ITERATIONS for p in ('paired', 'unpaired')]
    return keys + ['inflight0', 'inflight1']


def test_the_scenes_reach_every_entry_and_exit_of_the_unrolled_loop(both):
    new, old = both
    assert new['runs'] == old['runs'] and new['nu'] == old['nu'] and new['store'] == old['store']
    assert new['store'] == {n: STORE_Z24 for n in straight_worker.NEIGHBOURS}, new['store']   # the store the straight run is written for
    nine = {(p, m) for p in range(3) for m in range(3)}
    for kernel in straight_worker.KERNELS:
        seen = set().union(*(new['runs'][(n, kernel)] for n in straight_worker.NEIGHBOURS))
        print(kernel, 'runs (ring slot, chunks mod 3):', sorted(seen))
        assert seen == nine, (kernel, sorted(nine - seen))
    assert all(strips > 0 for strips, _ in new['nu'].values())
    assert any(without > 0 for _, without in new['nu'].values()), new['nu']


def test_every_fit_ran_in_both_builds(both):
    new, old = both
    assert set(new['fits']) == set(_keys()) and set(old['fits']) == set(_keys())
    assert all(len(v) == 4 for v in new['fits'].values())


@pytest.mark.parametrize('key', _keys())
def test_the_product_keeps_every_bit_of_the_generic_build(both, key):
    new, old = both
    for what, a, b in zip(('state', 'parameters', 'J', 'trace'), new['fits'][key], old['fits'][key]):
        assert a == b, (key, what, 'differs between the product and the generic build')


def test_the_fits_depend_on_what_they_should(both):
    """The digests tell fits apart (a worker that hashed nothing would pass the comparison): scenes and iteration counts differ,
    the paired and the unpaired fit of one build agree (tests/test_gpu_paired.py), and a restoration keeps its bits with a
    neighbour in flight."""
    new = both[0]['fits']
    n0, n1, n2 = straight_worker.NEIGHBOURS
    assert new[f'{n1}/T6/paired'] == new[f'{n1}/T6/unpaired'] and new[f'{n1}/T5/paired'] == new[f'{n1}/T5/unpaired']
    assert new[f'{n1}/T6/paired'][2] != new[f'{n1}/T5/paired'][2]
    assert new[f'{n0}/T6/paired'][2] != new[f'{n2}/T6/paired'][2]
    assert new['inflight0'] == new[f'{n1}/T6/paired'] and new['inflight1'] == new[f'{n2}/T6/paired']
