#!/usr/bin/env python
"""CPU: compare the gfx950 device code of the project's kernels between two source trees, kernel by kernel.

    python tools/kernel_isa_diff.py PARENT_TREE BRANCH_TREE motion_segment.hip voxel_grid.hip ... [--out FILE]

Each source (a name under hplflownet_amd/csrc of both trees) is compiled to device assembly with the flags of the branch
tree's build.py plus `--cuda-device-only -S`.  A kernel's instruction stream is the text between its label and the end of the
function without comments and directives, local labels renumbered by first appearance.  Per kernel: same or DIFFERS, the
instruction counts, and the four resource figures of the code object's metadata (.vgpr_count, .sgpr_count,
.private_segment_fixed_size = scratch bytes a lane, .group_segment_fixed_size = LDS bytes a workgroup).  Library
instantiations (rocPRIM's kernels: a type's name is part of their symbol) are left out.  The tool only compares; it needs no
GPU.  Exit status 0 whatever differs."""
import argparse
import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIGURES = ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')
LOCAL = re.compile(r'\.L[A-Za-z_$]*\d+(?:_\d+)*')


def assembly(tree, src, flags, hipcc):
    path = os.path.join(tree, 'hplflownet_amd', 'csrc', src)
    return subprocess.check_output([hipcc] + flags + ['-Wno-unused-command-line-argument', '--cuda-device-only', '-S', path,
                                    '-o', '-']).decode()


def kernels_of(text):
    """{kernel symbol: (instruction stream as a list of lines, {figure: value})}"""
    lines = text.splitlines()
    names = [ln.split()[1] for ln in lines if ln.strip().startswith('.amdhsa_kernel ')]
    streams = {}
    for name in names:
        at = lines.index(name + ':') if name + ':' in lines else next(
            i for i, ln in enumerate(lines) if ln.split(';')[0].strip() == name + ':')
        body, seen = [], {}
        for ln in lines[at + 1:]:
            code = ln.split(';')[0].strip()
            if code.startswith('.Lfunc_end'):
                break
            if not code or (code.startswith('.') and not code.endswith(':')):
                continue                         # a comment, or a directive (a local label ends with a colon)
            body.append(LOCAL.sub(lambda m: seen.setdefault(m.group(0), '.L%d' % len(seen)), ' '.join(code.split())))
        streams[name] = body
    figures, cur = {}, None
    for ln in lines:
        m = re.match(r'^(  - | {4})\.(\w+):\s*(.*)$', ln)
        if not m:
            continue
        if m.group(1) == '  - ':
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip()
            if 'name' in cur and cur['name'] in streams:
                figures[cur['name']] = cur
    return {n: (streams[n], {f: int(figures.get(n, {}).get(f, -1)) for f in FIGURES}) for n in names}


def demangled(names):
    for tool in ('/opt/rocm/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt', 'c++filt'):
        try:
            out = subprocess.check_output([tool] + list(names)).decode().splitlines()
            if len(out) == len(names):
                return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(name):
    name = name.replace('(anonymous namespace)::', '').replace('void ', '')
    return re.sub(r'\(.*\)$', '', name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('branch')
    ap.add_argument('sources', nargs='+')
    ap.add_argument('--out', default=None)
    ap.add_argument('--show', default=None, help='also print the unified diff of the kernels whose name contains this')
    a = ap.parse_args()
    from hplflownet_amd.build import FLAGS
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    rows = ['%-16s %-22s %-8s %13s   %s' % ('source', 'kernel', '', 'instructions', 'parent -> branch: VGPRs, SGPRs, scratch, LDS')]
    same = differs = 0
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:    # (the threads only wait for compilers)
        texts = list(pool.map(lambda job: assembly(job[0], job[1], FLAGS, hipcc),
                              [(t, src) for src in a.sources for t in (a.parent, a.branch)]))
    for k, src in enumerate(a.sources):
        old, new = kernels_of(texts[2 * k]), kernels_of(texts[2 * k + 1])
        names = [n for n in new if 'rocprim' not in n] + [n for n in old if n not in new and 'rocprim' not in n]
        pretty = demangled(names)
        for n in sorted(names, key=lambda n: short(pretty[n])):
            if n not in old or n not in new:
                rows.append('%-16s %-22s only in the %s' % (src[:-4], short(pretty[n]), 'branch' if n in new else 'parent'))
                differs += 1
                continue
            (so, fo), (sn, fn) = old[n], new[n]
            equal = so == sn
            same, differs = same + equal, differs + (not equal)
            fig = ', '.join('%d' % fo[f] if fo[f] == fn[f] else '%d -> %d' % (fo[f], fn[f]) for f in FIGURES)
            count = sum(not ln.endswith(':') for ln in so), sum(not ln.endswith(':') for ln in sn)
            rows.append('%-16s %-22s %-8s %13s   %s' % (src[:-4], short(pretty[n]), 'same' if equal else 'DIFFERS',
                                                       '%d' % count[0] if count[0] == count[1] else '%d -> %d' % count, fig))
            if a.show and a.show in pretty[n] and not equal:
                rows.extend(difflib.unified_diff(so, sn, 'parent', 'branch', lineterm='', n=2))
    rows.append('')
    rows.append('%d kernels with the same instruction stream, %d that differ' % (same, differs))
    print('\n'.join(rows))
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
