#!/usr/bin/env python3
"""One line per kernel of the compiler's gfx950 assembly: what a refactor must leave as it was.

  make -C sucre_amd/csrc fit.s match.s compact.s light.s plot.s
  python tools/isa_digest.py sucre_amd/csrc/*.s > after.txt        # the same on the parent commit, then diff the two

Columns: kernel (demangled where c++filt is at hand), instructions, hash of the instruction text (comments dropped, labels
renamed in order of appearance), hash of the opcode mnemonics alone, then the code object's own metadata: vgpr_count,
sgpr_count, vgpr / sgpr spill counts, LDS bytes, scratch bytes."""
import hashlib
import re
import shutil
import subprocess
import sys

META = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'group_segment_fixed_size', 'private_segment_fixed_size')


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()[:12]


def kernels(path):
    src = open(path).read()
    meta = {}
    for block in src.split('  - .agpr_count:')[1:]:   # amdhsa.kernels: one YAML entry per kernel
        name = re.search(r'^\s+\.name:\s+(\S+)', block, re.M).group(1)
        meta[name] = [int(re.search(rf'^\s+\.{key}:\s+(\d+)', block, re.M).group(1)) for key in META]
    lines = src.split('\n')
    for name in sorted(meta):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        labels, text, ops = {}, [], []
        for ln in lines[start + 1:end]:
            ln = ln.split(';')[0].rstrip()
            if not re.match(r'\s+[a-z]', ln):   # labels, directives, blank lines
                continue
            ln = re.sub(r'\.LBB\d+_\d+', lambda m: labels.setdefault(m.group(0), f'L{len(labels)}'), ' '.join(ln.split()))
            text.append(ln)
            ops.append(ln.split()[0])
        yield name, len(ops), digest('\n'.join(text)), digest('\n'.join(ops)), meta[name]


def main():
    rows = [row for path in sys.argv[1:] for row in kernels(path)]
    names = [r[0] for r in rows]
    if shutil.which('c++filt'):
        names = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
        names = [re.sub(r'^void |\((?!anonymous).*$', '', n) for n in names]   # template arguments tell the instantiations apart
    print('# kernel | instructions | text hash | opcode hash | ' + ' '.join(META))
    for shown, (name, n, h_text, h_ops, m) in sorted(zip(names, rows)):
        print(f'{shown} | {n} | {h_text} | {h_ops} | ' + ' '.join(map(str, m)))


if __name__ == '__main__':
    main()
