#!/usr/bin/env python3
"""Compare the gfx950 device code of libcc_mi355x.so's two units at two revisions, per function.

    tools/isa_diff.py <rev_a> <rev_b>      (a revision, or a directory holding a tree: `.`)

Each unit is compiled with build.py's flags plus `--cuda-device-only -S`.  Per function the
normalised body (comments and block-label numbers stripped) and the resource block (the
`.amdhsa_` lines of a kernel, the `.set <name>.*` lines of any function) are compared; functions
that differ are listed with line count, VGPRs, SGPRs, LDS and scratch.  Needs no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cluster_tools_amd'))
import build  # noqa: E402  (compiler, architecture, units)


def compile_unit(tree, unit, out):
    src = os.path.join(tree, 'cluster_tools_amd', 'csrc', unit + '.hip')
    subprocess.run([build.HIPCC, '--offload-arch=%s' % build.ARCH, '-O3', '-std=c++17', '-fPIC', '-Wall',
                    '-Wno-unused-function', '-Wno-unused-command-line-argument', '-DCC_SRC_HASH="isa_diff"',
                    '--cuda-device-only', '-S', src, '-o', out], check=True)
    return out


def functions(path):
    """name -> (body lines, resource lines) of one assembly file"""
    text = re.sub(r'[ \t]*;[^\n]*', '', open(path).read())
    text = re.sub(r'\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+', r'.\1', text)
    lines = [ln for ln in text.split('\n') if ln.strip()]
    at = {ln: i for i, ln in enumerate(lines)}
    out = {}
    for ln in lines:
        m = re.match(r'\s*\.type\s+(\S+),@function', ln)
        if m:
            name = m.group(1)
            beg = at[name + ':']
            end = next(i for i in range(beg, len(lines)) if lines[i].startswith('\t.size\t' + name + ','))
            out[name] = (lines[beg:end], [])
        m = re.match(r'\s*\.set (?:\.L)?(\w+)\.\w+, ', ln)
        if m and m.group(1) in out:
            out[m.group(1)][1].append(ln.strip())
        m = re.match(r'\s*\.amdhsa_kernel (\S+)', ln)
        if m:
            k = at[ln]
            out[m.group(1)][1].extend(s.strip() for s in lines[k:lines.index('\t.end_amdhsa_kernel', k)])
    return out


def figures(name, fn):
    body, res = fn

    def get(key):
        return next((ln.split()[-1] for ln in res if key in ln), '-')
    return '%s: %d lines, vgpr %s, sgpr %s, lds %s, scratch %s' % (
        name, len(body), get('.num_vgpr,'), get('.numbered_sgpr,'), get('group_segment_fixed_size'), get('.private_seg_size,'))


def main(rev_a, rev_b):
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        trees = []
        try:
            for i, rev in enumerate((rev_a, rev_b)):
                if os.path.isdir(rev):
                    trees.append(os.path.abspath(rev))
                    continue
                trees.append(os.path.join(tmp, 'tree%d' % i))
                subprocess.run(['git', 'worktree', 'add', '--detach', '-q', trees[-1], rev], check=True)
            asm = []
            for i, tree in enumerate(trees):
                with ThreadPoolExecutor(2) as pool:       # one job per unit
                    asm.append(list(pool.map(
                        lambda u: functions(compile_unit(tree, u, os.path.join(tmp, '%s_%d.s' % (u, i)))), build.UNITS)))
            for unit, a, b in zip(build.UNITS, *asm):
                both = sorted(set(a) & set(b))
                bad = [n for n in both if a[n] != b[n]]
                differ += len(bad)
                print('%s: %d functions at %s, %d at %s, %d in both, %d differ'
                      % (unit, len(a), rev_a, len(b), rev_b, len(both), len(bad)))
                for rev, only in ((rev_a, set(a) - set(b)), (rev_b, set(b) - set(a))):
                    for n in sorted(only):
                        print('  only at %s: %s' % (rev, n))
                for n in bad:
                    what = ' and '.join(w for w, i in (('body', 0), ('resources', 1)) if a[n][i] != b[n][i])
                    print('  %s differ\n    %s\n    %s' % (what, figures(n, a[n]), figures(n, b[n])))
        finally:
            for t in trees:
                if t.startswith(tmp):
                    subprocess.run(['git', 'worktree', 'remove', '--force', t], check=False)
    return 1 if differ else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
