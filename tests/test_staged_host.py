"""Host-side checks of the yields in the fit kernels' chunk arithmetic (csrc/fit.hip, grad_terms' kYield; csrc/experiment.h
SUCRE_STAGED_TERMS): fit.hip compiled for gfx950 with the knob at 1 (the product) and at 0 through the product Makefile's own
rules -- no kernel with scratch, every fit kernel inside the registers of its wave count, and the 0 form instruction for
instruction what fit.hip was before the knob (opcode hashes of tools/isa_digest.py, kept as data in
tests/golden/fit_isa_unstaged.txt)."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

import helpers

ROOT = Path(helpers.ROOT)
CSRC = ROOT / 'sucre_amd' / 'csrc'
GOLDEN = ROOT / 'tests' / 'golden' / 'fit_isa_unstaged.txt'
# waves per SIMD a kernel is launched for (layout.h kFitWaves / kClosedWaves, fit.hip kGroupFitWaves): 5 -> 96 VGPRs, 4 -> 128
WAVES = (('fit_grad_kernel', 5), ('fit_closed_kernel', 4), ('group_iter_kernelILi0E', 5), ('group_iter_kernelILi1E', 4),
         ('batch_iter_kernelILi0E', 5), ('batch_iter_kernelILi1E', 4))
VGPR_LIMIT = {5: 96, 4: 128}


def _resources(rpt):
    """{mangled kernel name: (VGPRs, scratch bytes per lane, occupancy)} from the compiler's kernel-resource-usage remarks."""
    out = {}
    for block in rpt.split('remark: Function Name: ')[1:]:
        name = block.split()[0]
        vgprs, scratch, occ = (int(re.search(pat, block).group(1)) for pat in
                               (r'remark:\s+VGPRs: (\d+)', r'ScratchSize \[bytes/lane\]: (\d+)', r'Occupancy \[waves/SIMD\]: (\d+)'))
        out[name] = (vgprs, scratch, occ)
    return out


@pytest.fixture(scope='module')
def builds():
    """{knob: (resource remarks of fit.hip, path of its assembly or None)}; the files carry scratch suffixes and are removed."""
    if shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists():
        pytest.skip('no hipcc on this machine')
    names = {1: 'tstaged1', 0: 'tstaged0'}
    try:
        got = {}
        for knob, name in names.items():
            targets = [f'fit_{name}.o'] + ([f'fit_{name}.s'] if knob == 0 else [])
            out = subprocess.run(['make', '-C', str(CSRC), '-j2', f'VARIANT={name}', f'EXTRA=-DSUCRE_STAGED_TERMS={knob}', *targets],
                                 capture_output=True, text=True)
            assert out.returncode == 0, (knob, out.stdout[-1500:], out.stderr[-1500:])
            got[knob] = ((CSRC / f'fit_{name}.rpt').read_text(), (CSRC / f'fit_{name}.s').read_text() if knob == 0 else None)
        yield got
    finally:
        for name in names.values():
            for f in CSRC.glob(f'*_{name}.*'):
                f.unlink()


@pytest.mark.parametrize('knob', (1, 0))
def test_no_scratch_and_the_registers_of_the_wave_count(builds, knob):
    res = _resources(builds[knob][0])
    assert len(res) >= 30 and all(scratch == 0 for _, scratch, _ in res.values()), [n for n, r in res.items() if r[1]]
    seen = 0
    for needle, waves in WAVES:
        for name, (vgprs, _, occ) in res.items():
            if needle in name:
                seen += 1
                assert vgprs <= VGPR_LIMIT[waves] and occ >= waves, (knob, name, vgprs, occ)
    assert seen == 22, seen
    # the paired kernels of the headline: L <.., 1>, F <.., 2>, and the one-launch kernel <.., 0>
    for pair in (0, 1, 2):
        for fmt in (0, 1):
            assert res[next(n for n in res if f'fit_grad_kernelILb1ELi{fmt}ELi{pair}E' in n)][0] <= 96


def test_the_knob_changes_the_kernels_it_should(builds):
    """At 1 every J-parameter kernel but the batch launch's holds the yields (four more registers hold what they pin); the batch
    and the closed-form kernels are the same either way."""
    new, old = _resources(builds[1][0]), _resources(builds[0][0])
    assert set(new) == set(old)
    for name in new:
        moved = new[name][0] != old[name][0]
        assert moved == ('fit_grad_kernel' in name or 'group_iter_kernelILi0E' in name), (name, new[name], old[name])


def test_the_knob_at_zero_is_the_parents_code(builds, tmp_path):
    sys.path.insert(0, str(ROOT / 'tools'))
    try:
        import isa_digest
    finally:
        sys.path.pop(0)
    s = tmp_path / 'fit.s'
    s.write_text(builds[0][1])
    got = {name: (n, h_ops) for name, n, _, h_ops, _ in isa_digest.kernels(str(s))}
    want = {}
    for ln in GOLDEN.read_text().splitlines():
        if ln and not ln.startswith('#'):
            name, n, h_ops = (x.strip() for x in ln.split('|'))
            want[name] = (int(n), h_ops)
    assert len(want) == 34 and set(got) == set(want)
    assert got == want, sorted(n for n in want if got[n] != want[n])
