#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, kernel by kernel.

    python tools/isa_diff.py A B [--tools] [-j N]

A and B are two checkouts of this repository (for instance `git worktree add ../parent HEAD~1` and the working tree).  Every translation unit of
build.py::SOURCES (--tools: TOOLS_SOURCES with -DVP_TOOLS) is compiled in both with build.py::FLAGS (+ its SOURCE_FLAGS entry, where a tree has one) + `--cuda-device-only -S`, each tree with its own
build.py, into a temporary directory.  Comment lines and the `__hip_cuid_*` lines (a hash of the compilation) are dropped, kernels are paired by order
of appearance and their mangled symbols replaced by the ordinal, so a renamed template argument is no difference but any instruction, register count
or kernel descriptor field is.  One line per translation unit: `identical`, or the kernels that differ with their register counts, spills, scratch
and code size on both sides, each followed by the opcodes whose COUNT differs (`same opcode counts`: registers and order moved, no instruction was
added or dropped).  Exit status 1 if anything differs.  No GPU is needed.

A refactor of a kernel source is behaviour- and speed-neutral exactly when this reports `identical` for the product build.  --tools is informative
only where the change adds or retires rows of the tile table: those kernels (dis)appear in the measurement build by design.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

STATS = ['.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.private_segment_fixed_size']


def load_build(tree: str):
    path = os.path.join(tree, 'easy_vitpose_amd', 'build.py')
    spec = importlib.util.spec_from_file_location('_isa_diff_build_%x' % (hash(path) & 0xffffffff), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def describe(tree: str) -> str:
    def git(*a):
        r = subprocess.run(['git', '-C', tree, *a], capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 else None
    head = git('rev-parse', 'HEAD')
    if not head:
        return 'no git'
    return head + (' + uncommitted changes' if git('status', '--porcelain', '--untracked-files=no') else '')


def compile_asm(build, src: str, out: str, tools: bool):
    # run inside csrc with a relative source name: no path of the tree reaches the assembly
    cmd = [build._hipcc(), *build.FLAGS, *getattr(build, 'SOURCE_FLAGS', {}).get(src, []), *(['-DVP_TOOLS'] if tools else []), '--cuda-device-only', '-S', src, '-o', out]
    r = subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed in {build.CSRC}: {" ".join(cmd)}\n{r.stdout}\n{r.stderr}')


class Asm:
    """One translation unit: kernels[i] = (symbol, text, stats); rest = everything outside the kernels."""

    def __init__(self, path: str):
        with open(path) as f:
            lines = f.read().split('\n')
        syms = [m.group(1) for ln in lines if (m := re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln))]
        code_len, cur, symset = {}, None, set(syms)
        for ln in lines:   # `; codeLenInByte = N` is a comment behind the kernel's code: read it before the comments go
            if (m := re.match(r'(\S+):', ln)) and m.group(1) in symset:   # the kernel's label (a comment may follow it)
                cur = m.group(1)
            elif cur and (m := re.match(r';\s*codeLenInByte\s*=\s*(\d+)', ln)):
                code_len[cur] = int(m.group(1))
                cur = None
        lines = [ln for ln in lines if not ln.lstrip().startswith(';') and '__hip_cuid_' not in ln]
        text = '\n'.join(lines)
        if syms:
            ordinal = {s: '@K%d@' % i for i, s in enumerate(syms)}
            alt = re.compile('|'.join(re.escape(s) for s in sorted(syms, key=len, reverse=True)))
            text = alt.sub(lambda m: ordinal[m.group(0)], text)
        # code: a kernel's part runs from the first line that names it to the first line that names the next one
        body, _, meta = text.partition('\t.amdgpu_metadata\n')
        parts, cur = [[] for _ in range(len(syms) + 1)], -1
        tag = re.compile(r'@K(\d+)@')
        closing = False   # behind the last kernel: the register maximums and the constant tables of ALL kernels, which close the unit
        for ln in body.split('\n'):
            closing = closing or '.AMDGPU.gpr_maximums' in ln
            m = None if closing else tag.search(ln)
            if m and int(m.group(1)) > cur:
                cur = int(m.group(1))
            parts[0 if closing else cur + 1].append(ln)
        # ... and neither do the lines behind a kernel's last own line (section switches, padding): without this the unit's tail counts as part of its last
        # kernel, and a kernel added behind it would show as a difference of that one
        tail = []
        for k in range(1, len(parts)):
            last = max((i for i, ln in enumerate(parts[k]) if tag.search(ln)), default=-1)
            tail += parts[k][last + 1:]
            del parts[k][last + 1:]
        parts[0] += tail
        # metadata: one YAML list item per kernel
        meta, sep, closing_meta = meta.partition('\namdhsa.target:')   # what follows the last kernel's item is no part of it
        items = re.split(r'\n(?=  - )', meta) + ([sep + closing_meta] if sep else [])
        stats = [dict() for _ in syms]
        rest = ['\n'.join(parts[0])]
        for it in items:
            m = re.search(r'\.symbol:\s+@K(\d+)@\.kd', it)
            if not m:
                rest.append(it)
                continue
            k = int(m.group(1))
            parts[k + 1].append(it)
            for key in STATS:
                mm = re.search(r'^\s*(?:- )?' + re.escape(key) + r':\s*(\d+)', it, re.M)
                stats[k][key] = int(mm.group(1)) if mm else None
        self.kernels = []
        for i, s in enumerate(syms):
            stats[i]['codeLenInByte'] = code_len.get(s)
            self.kernels.append((s, '\n'.join(parts[i + 1]), stats[i]))
        self.rest = '\n'.join(rest)


def opcode_counts(text: str) -> "dict[str, int]":
    """Instructions of a kernel by opcode (assembler lines start with a tab; directives with a dot, labels and metadata do not match)."""
    return dict(Counter(m.group(1) for m in re.finditer(r'^\t([a-z][a-z0-9_]*)\b', text, re.M)))


def compare(name: str, a: Asm, b: Asm) -> "tuple[bool, list[str]]":
    out, n = [], min(len(a.kernels), len(b.kernels))
    differ = [i for i in range(n) if a.kernels[i][1:] != b.kernels[i][1:]]
    same = not differ and len(a.kernels) == len(b.kernels) and a.rest == b.rest
    if same:
        return True, [f'{name}: identical ({n} kernels)']
    head = f'{name}: {len(differ)} of {n} paired kernels differ'
    if len(a.kernels) != len(b.kernels):
        head += f'; {len(a.kernels)} kernels in A, {len(b.kernels)} in B'
    if not differ and a.rest != b.rest:
        head += '; text outside the kernels differs'
    out.append(head)
    for i in differ:
        sa, sb = a.kernels[i][2], b.kernels[i][2]
        out.append(f'  #{i} {b.kernels[i][0]}: ' + ', '.join(f'{k} {sa[k]} -> {sb[k]}' for k in STATS + ['codeLenInByte']))
        ca, cb = opcode_counts(a.kernels[i][1]), opcode_counts(b.kernels[i][1])
        moved = [f'{op} {ca.get(op, 0)} -> {cb.get(op, 0)}' for op in sorted(set(ca) | set(cb)) if ca.get(op, 0) != cb.get(op, 0)]
        out.append('      ' + (', '.join(moved) if moved else 'same opcode counts'))
    return False, out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('A')
    ap.add_argument('B')
    ap.add_argument('--tools', action='store_true', help='the measurement build: -DVP_TOOLS, TOOLS_SOURCES')
    ap.add_argument('-j', type=int, default=min(16, os.cpu_count() or 1), help='parallel compilations (at most 16)')
    args = ap.parse_args()
    trees = [os.path.abspath(args.A), os.path.abspath(args.B)]
    builds = [load_build(t) for t in trees]
    srcs = [list(b.TOOLS_SOURCES if args.tools else b.SOURCES) for b in builds]
    names = srcs[0] + [s for s in srcs[1] if s not in srcs[0]]
    print(f'# isa_diff ({"measurement build, -DVP_TOOLS" if args.tools else "product build"}): A = {describe(trees[0])}; B = {describe(trees[1])}', flush=True)
    ok = True
    with tempfile.TemporaryDirectory(prefix='isa_diff_') as tmp:
        jobs = [(side, s, os.path.join(tmp, f'{"ab"[side]}_{s}.s')) for s in names for side in (0, 1) if s in srcs[side]]
        with ThreadPoolExecutor(max_workers=max(1, min(args.j, 16))) as ex:
            list(ex.map(lambda j: compile_asm(builds[j[0]], j[1], j[2], args.tools), jobs))
        for s in names:
            if s not in srcs[0] or s not in srcs[1]:
                print(f'{s}: only in {"A" if s in srcs[0] else "B"}')
                ok = False
                continue
            same, lines = compare(s, Asm(os.path.join(tmp, f'a_{s}.s')), Asm(os.path.join(tmp, f'b_{s}.s')))
            ok &= same
            print('\n'.join(lines), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
