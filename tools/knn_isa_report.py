#!/usr/bin/env python3
"""Registers, scratch and vector-instruction counts of one KNN scan kernel, read from the device assembly.  No GPU needed.

Compiles tiler_amd/csrc/tm_knn3_k<HT>.hip to gfx950 assembly with the flags build.sh uses (read from build.sh itself) and reports, for the
named instantiations of k_knn_seed / k_knn_consume (nearest-neighbour mode):
  next_free_vgpr, private_segment_fixed_size   from the kernel descriptor
  first_look   vector instructions (matrix instructions not counted) from the chain's last matrix instruction to the branch that
               ends a block for the lanes the first look turns away
  exact        vector instructions of what that branch guards: the minimum's value, its row, the atomics
  nops         s_nop instructions inside `exact` (issue slots that do no work)
  chunk_look   (consume) vector instructions of the first-chunk look, from its last matrix instruction to the branch that ends the block

  python tools/knn_isa_report.py --ht 5 --hq 4 --td 0 [--kernel consume --kernel seed] [--json] [--asm FILE] [--keep FILE]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tiler_amd', 'csrc')


def find_hipcc():
    cand = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    return cand if os.path.isfile(cand) and os.access(cand, os.X_OK) else None


def build_flags():
    """The FLAGS= line of build.sh, without the environment's extras."""
    text = open(os.path.join(CSRC, 'build.sh')).read()
    m = re.search(r'^FLAGS="([^"]*)"', text, re.M)
    if not m:
        raise SystemExit('build.sh: no FLAGS= line')
    return [f for f in m.group(1).split() if not f.startswith('$')]


def compile_asm(ht, out):
    hipcc = find_hipcc()
    if hipcc is None:
        raise SystemExit('hipcc not found')
    cmd = [hipcc] + build_flags() + ['--cuda-device-only', '-S', os.path.join(CSRC, 'tm_knn3_k%d.hip' % ht), '-o', out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def mangled(kernel, ht, hq, td):
    name = {'seed': 'k_knn_seed', 'consume': 'k_knn_consume'}[kernel]
    return '_ZN3tmx%d%sILi%dELi%dELb%dELb0EEEvNS_8Knn3ArgsE' % (len(name), name, ht, hq, 1 if td else 0)


def is_valu(ins):
    return ins.startswith('v_') and not ins.startswith('v_mfma')


def report(lines, sym):
    try:
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ':'))
    except StopIteration:
        raise SystemExit('no kernel %s in the assembly' % sym)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    body = [l.split(';')[0].strip() for l in lines[start:end]]
    desc = next(i for i, l in enumerate(lines) if l.strip() == '.amdhsa_kernel ' + sym)
    out = {}
    for l in lines[desc:desc + 80]:
        m = re.match(r'\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|accum_offset)\s+(\d+)', l)
        if m:
            out[m.group(1)] = int(m.group(2))
        if l.strip() == '.end_amdhsa_kernel':
            break
    # The looks: each is a tree of three-way minima behind a matrix instruction.  The chain's first look ends in a branch on the LANES'
    # verdict (s_and_saveexec); the first-chunk look of the consume kernel (k3_chunk_look) comes before it in the code and ends in a
    # branch on a ballot (s_cbranch): it is reported beside the other two as `chunk_look`.
    # (An assumption about the code as it is scheduled today: no other scalar branch stands between a tree of minima and the branch on its
    # verdict.  One that did would be taken for a ballot's and mislabel the look; tests/test_knn_isa.py would then miss `first_look`.)
    first_min = None
    i = 0
    while first_min is None:
        i = next(j for j in range(i, len(body)) if body[j].startswith('v_min3_i32'))
        mfma = max(j for j in range(i) if body[j].startswith('v_mfma'))
        br = next(j for j in range(i, len(body)) if body[j].startswith('s_and_saveexec_b64') or body[j].startswith('s_cbranch'))
        if body[br].startswith('s_and_saveexec_b64'):
            first_min = i
        else:
            out['chunk_look'] = sum(is_valu(l) for l in body[mfma + 1:br])
            i = br
    last_mfma = max(i for i in range(first_min) if body[i].startswith('v_mfma'))
    save = next(i for i in range(first_min, len(body)) if body[i].startswith('s_and_saveexec_b64'))
    saved = body[save].split()[1].rstrip(',')
    restore = next(i for i in range(save, len(body)) if re.match(r's_or_b64 exec, exec, ' + re.escape(saved) + r'$', body[i]))
    out['first_look'] = sum(is_valu(l) for l in body[last_mfma + 1:save])
    out['exact'] = sum(is_valu(l) for l in body[save + 1:restore])
    out['nops'] = sum(l.startswith('s_nop') for l in body[save + 1:restore])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--ht', type=int, default=5)
    ap.add_argument('--hq', type=int, default=4)
    ap.add_argument('--td', type=int, default=0)
    ap.add_argument('--kernel', action='append', choices=['seed', 'consume'])
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--asm', help='read this assembly file instead of compiling')
    ap.add_argument('--keep', help='keep the assembly here')
    a = ap.parse_args()
    kernels = a.kernel or ['consume', 'seed']
    if a.asm:
        lines = open(a.asm).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'k.s')
            compile_asm(a.ht, path)
            if a.keep:
                shutil.copy(path, a.keep)
            lines = open(path).read().splitlines()
    res = {k: dict(report(lines, mangled(k, a.ht, a.hq, a.td)), instantiation='k_knn_%s<%d, %d, %s, false>' % (k, a.ht, a.hq, 'true' if a.td else 'false'))
           for k in kernels}
    if a.json:
        print(json.dumps(res))
    else:
        for k, r in res.items():
            print('%s: next_free_vgpr %d, private_segment_fixed_size %d, vector instructions: first look %d, exact path %d (+ %d s_nop)%s' %
                  (r['instantiation'], r['next_free_vgpr'], r['private_segment_fixed_size'], r['first_look'], r['exact'], r['nops'],
                   ', first-chunk look %d' % r['chunk_look'] if 'chunk_look' in r else ''))
    return 0


if __name__ == '__main__':
    sys.exit(main())
