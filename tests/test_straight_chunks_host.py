"""Host-side checks of the straight run of unmasked full chunks in the J-parameter kernels (csrc/fit.hip: stream_strips' straight_run,
read_chunk_z24, accumulate_chunk_z24; csrc/experiment.h SUCRE_STRAIGHT_CHUNKS): fit.hip compiled for gfx950 with the knob at 1 (the
product) and at 0 through the product Makefile's own rules -- the 0 form instruction for instruction what fit.hip was before the
knob (opcode hashes of tools/isa_digest.py, kept as data in tests/golden/fit_isa_generic.txt), the 1 form without scratch and
inside the registers of five waves, its unrolled loop free of format tests, address additions and the gathering of the red bytes,
and every kernel the knob is not meant for left as it was."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

import helpers

ROOT = Path(helpers.ROOT)
CSRC = ROOT / 'sucre_amd' / 'csrc'
GOLDEN = ROOT / 'tests' / 'golden' / 'fit_isa_generic.txt'
HEADLINE = tuple(f'fit_grad_kernelILb{fused}ELi0ELi{pair}E' for fused, pair in ((1, 0), (1, 1), (1, 2), (0, 0)))   # one launch, L, F, the split form
RING = 3


def _digests(text, tmp_path, name):
    sys.path.insert(0, str(ROOT / 'tools'))
    try:
        import isa_digest
    finally:
        sys.path.pop(0)
    s = tmp_path / name
    s.write_text(text)
    return {kernel: (n, h_ops) for kernel, n, _, h_ops, _ in isa_digest.kernels(str(s))}


def _golden():
    want = {}
    for ln in GOLDEN.read_text().splitlines():
        if ln and not ln.startswith('#'):
            name, n, h_ops = (x.strip() for x in ln.split('|'))
            want[name] = (int(n), h_ops)
    assert len(want) == 34
    return want


@pytest.fixture(scope='module')
def builds():
    """{knob: (resource remarks of fit.hip, its assembly)}; the files carry scratch suffixes and are removed."""
    if shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists():
        pytest.skip('no hipcc on this machine')
    names = {1: 'tstraight1', 0: 'tstraight0'}
    try:
        got = {}
        for knob, name in names.items():
            out = subprocess.run(['make', '-C', str(CSRC), '-j2', f'VARIANT={name}', f'EXTRA=-DSUCRE_STRAIGHT_CHUNKS={knob}', f'fit_{name}.o', f'fit_{name}.s'],
                                 capture_output=True, text=True)
            assert out.returncode == 0, (knob, out.stdout[-1500:], out.stderr[-1500:])
            got[knob] = ((CSRC / f'fit_{name}.rpt').read_text(), (CSRC / f'fit_{name}.s').read_text())
        yield got
    finally:
        for name in names.values():
            for f in CSRC.glob(f'*_{name}.*'):
                f.unlink()


def test_the_knob_at_zero_is_the_parents_code(builds, tmp_path):
    got, want = _digests(builds[0][1], tmp_path, 'fit0.s'), _golden()
    assert set(got) == set(want)
    assert got == want, sorted(n for n in want if got[n] != want[n])


def test_the_headline_kernels_keep_their_resources(builds):
    """No scratch anywhere (the Makefile's rule has already refused it), and L, F, the one-launch kernel and the split form inside
    the 96 registers of five waves per SIMD."""
    seen = 0
    for block in builds[1][0].split('remark: Function Name: ')[1:]:
        name = block.split()[0]
        vgprs, scratch, occ = (int(re.search(pat, block).group(1)) for pat in
                               (r'remark:\s+VGPRs: (\d+)', r'ScratchSize \[bytes/lane\]: (\d+)', r'Occupancy \[waves/SIMD\]: (\d+)'))
        assert scratch == 0, name
        if any(k in name for k in HEADLINE):
            seen += 1
            assert vgprs <= 96 and occ >= 5, (name, vgprs, occ)
    assert seen == len(HEADLINE)


def test_the_knob_changes_the_kernels_it_should(builds, tmp_path):
    """Only the fit_grad_kernel instantiations for float32 ranges hold a straight run.  Everything else keeps its opcode sequence --
    but group_iter_kernel<0, 0>, whose short-last-chunk loop comes out with three address registers renamed and their three
    instructions in another order when the module holds the new instantiations (the same instructions, count for count)."""
    got, want = _digests(builds[1][1], tmp_path, 'fit1.s'), _golden()
    assert set(got) == set(want)
    for name in want:
        if 'fit_grad_kernelILb' in name and 'ELi0ELi' in name:
            assert got[name][0] > want[name][0], name
        elif 'group_iter_kernelILi0ELi0E' in name:
            assert got[name][0] == want[name][0], name
        else:
            assert got[name] == want[name], name


def _loops(asm, needle):
    """Instruction lists of the innermost loops of the kernel whose name holds `needle` (the walk of tools/exp/isa_loops.py)."""
    lines = asm.split('\n')
    start = next(i for i, ln in enumerate(lines) if ln.startswith('_Z') and needle in ln and ':' in ln)
    end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
    body = lines[start:end]
    labels = {m.group(1): i for i, ln in enumerate(body) if (m := re.match(r'^(\.LBB\d+_\d+):', ln))}
    loops = []
    for i, ln in enumerate(body):
        m = re.match(r'\s+s_c?branch\w*\s+(\.LBB\d+_\d+)', ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    inner = [(a, b) for a, b in loops if not any((c > a and d < b) for c, d in loops if (c, d) != (a, b))]
    return [[ln.split(';')[0].split() for ln in body[a:b + 1] if re.match(r'\s+[a-z]', ln)] for a, b in inner]


@pytest.mark.parametrize('needle', HEADLINE)
def test_the_unrolled_loop_holds_what_it_should(builds, needle):
    """The loop of whole turns of the ring -- three chunks, 72 exponentials -- in both forms of the backscatter term: per chunk no more
    than 189 vector instructions, the lane's record read by three ds_read_b64 behind ONE address register with the slot in their
    offsets, no other LDS instruction, no v_perm_b32 (the red bytes stay where they lie), no scratch access."""
    turns = [ops for ops in _loops(builds[1][1], needle) if sum(o[0].startswith('v_exp_f32') for o in ops) == RING * 24]
    assert len(turns) >= 2, len(turns)   # scaled B and the fallback (block placement can show a turn's chunks as more than one loop)
    for ops in turns:
        names = [o[0] for o in ops]
        assert sum(n.startswith('v_') for n in names) <= RING * 189, sum(n.startswith('v_') for n in names)
        reads = [o for o in ops if o[0].startswith('ds_')]
        assert [o[0] for o in reads] == ['ds_read_b64'] * (3 * RING), [o[0] for o in reads]
        assert len({o[2].rstrip(',') for o in reads}) == 1, reads
        assert sorted(int(o[3].split(':')[1], 0) for o in reads) == [q * 2048 + b for q in range(RING) for b in (0, 8, 16)], reads
        assert not any(n.startswith(('v_perm_b32', 'scratch_', 'v_add_u32', 'v_add_co')) for n in names), [n for n in names if n.startswith(('v_perm', 'scratch_', 'v_add'))]
        assert sum(n == 's_waitcnt' for n in names) >= 3 * RING
