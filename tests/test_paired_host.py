"""Host-side checks of the paired J-parameter iterations (csrc/layout.h: plan_thread, kStreamL / kStreamF; csrc/experiment.h
SUCRE_PAIRED_J): the item streams the plan kernel writes for them, on hand-built strip tables, and the knob's other build."""
import shutil
import subprocess
from pathlib import Path

import pytest

import helpers

ROOT = Path(helpers.ROOT)
CSRC = ROOT / 'sucre_amd' / 'csrc'
CHECK = ROOT / 'tests' / 'native' / 'paired_plan_check.cpp'


@pytest.mark.parametrize('name,flags', [('product', []), ('equal_shares', ['-DSUCRE_DEAL_FIT=64,64,64,64,64']), ('ring4', ['-DSUCRE_RING=4', '-DSUCRE_MIN_STRIPS=1'])])
def test_paired_streams_name_plan_zeros_strips_inside_their_regions(tmp_path, name, flags):
    """tests/native/paired_plan_check.cpp (g++, the plan kernel's own per-thread code compiled for the host): L's and F's streams
    walk plan 0's strips in plan 0's order with plan 0's chunk items, F's J plane, G plane and moments come before its chunks,
    every source range lies inside its region and every wave's items fit the stride reserved for them."""
    if shutil.which('g++') is None:
        pytest.skip('no g++ on this machine')
    exe = tmp_path / f'paired_plan_{name}'
    out = subprocess.run(['g++', '-std=c++17', '-O1', f'-I{CSRC}', f'-I{ROOT / "include"}', *flags, str(CHECK), '-o', str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and ' 0 violations' in run.stdout, (name, run.stdout[-2000:], run.stderr[-2000:])


def test_unpaired_build_compiles():
    """SUCRE_PAIRED_J=0 through the product Makefile's own rule (the no-scratch check applies); the object goes to a scratch suffix
    and is removed.  That build holds no paired kernel: its fit_grad_kernel instantiations are the two J modes' only."""
    if shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists():
        pytest.skip('no hipcc on this machine')
    name = 'tunpaired'
    try:
        out = subprocess.run(['make', '-C', str(CSRC), f'VARIANT={name}', 'EXTRA=-DSUCRE_PAIRED_J=0', f'fit_{name}.o'], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
        rpt = (CSRC / f'fit_{name}.rpt').read_text()
        assert 'fit_grad_kernelILb1ELi0ELi0E' in rpt and 'fit_grad_kernelILb1ELi0ELi1E' not in rpt and 'fit_grad_kernelILb1ELi0ELi2E' not in rpt
    finally:
        for f in CSRC.glob(f'*_{name}.*'):
            f.unlink()


def test_the_switch_reaches_the_library(monkeypatch):
    """``engine.Restoration.fit(paired=...)`` and the engine knob SUCRE_PAIRED_FIT set SUCRE_FIT_UNPAIRED, and only where
    sucre_fit_run pairs: the plain model's J-parameter mode."""
    import inspect

    from sucre_amd import _lib, engine
    header = (ROOT / 'include' / 'sucre_hip.h').read_text()
    assert f'#define SUCRE_FIT_UNPAIRED {_lib.FIT_UNPAIRED}u' in header
    assert _lib.FIT_UNPAIRED & (_lib.FIT_CLOSED_FORM | _lib.FIT_OBS_U16MM | _lib.FIT_EXT_COLOUR | _lib.FIT_KEEP_J | _lib.FIT_EXT_BOTH) == 0
    assert inspect.signature(engine.Restoration.fit).parameters['paired'].default is None
    assert isinstance(engine.PAIRED_FIT, bool)
