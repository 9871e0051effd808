#!/usr/bin/env python3
"""Are two builds of a HIP source the same machine code?  Compares, per kernel and per out-of-line device function, the instruction
text of two gfx950 assembly files (comments, debug and layout directives stripped, labels renumbered by first use) and the kernel
descriptors and metadata (SGPR / VGPR counts, LDS and scratch bytes, kernarg layout).  The order of the functions does not count.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S cholesky_dataflow.hip -o new.s     (same for the other commit)
    python tools/asm_diff.py old.s new.s          exit status 1 if anything differs
"""
import re, sys
def parse(path):
    funcs, desc, cur, name = {}, {}, None, None
    in_kd = None
    for ln in open(path):
        ln = ln.split(';')[0].rstrip() if not ln.lstrip().startswith('.amdhsa') else ln.strip()
        t = ln.strip()
        if not t: continue
        m = re.match(r'^([A-Za-z_$][\w$.]*):$', t)
        if m and not t.startswith('.L'):
            name = m.group(1); cur = funcs.setdefault(name, []); continue
        if t.startswith('.amdhsa_kernel '): in_kd = t.split()[1]; desc[in_kd] = []; continue
        if t == '.end_amdhsa_kernel': in_kd = None; continue
        if in_kd is not None:
            if re.match(r'\.amdhsa_(next_free_[sv]gpr|group_segment_fixed_size|private_segment_fixed_size|accum_offset|kernarg_size|uses_dynamic_stack)', t): desc[in_kd].append(t)
            continue
        if t.startswith('.Lfunc_end'): cur = None; continue
        if cur is None: continue
        if re.match(r'^\.(loc|file|cfi_|p2align|type|size|globl|weak|protected|hidden|section|text|set|amdgpu_|ident|addrsig)', t): continue
        cur.append(t)
    # label numbering is not a difference: rename .LBBx_y by order of first appearance inside each function
    out = {}
    for f, body in funcs.items():
        names = {}
        def sub(m): return names.setdefault(m.group(0), '.L%d' % len(names))
        out[f] = [re.sub(r'\.L[A-Za-z_]*\d+(_\d+)?', sub, l) for l in body]
    return out, desc
def split_meta(funcs, desc):
    # the amdhsa.kernels metadata block is not code: compare it per kernel (as descriptors), whatever the order of the kernels
    body = funcs.pop('amdhsa.kernels', [])
    chunks, cur = [], None
    for l in body:
        if l.startswith('- .agpr_count'):
            cur = [l.lstrip('- ')]; chunks.append(cur)
        elif cur is not None: cur.append(l)
    for c in chunks:
        sym = [x for x in c if x.startswith('.name:')][-1].split()[1]
        desc.setdefault(sym, []).extend(['meta ' + x for x in c])
a, da = parse(sys.argv[1]); b, db = parse(sys.argv[2])
split_meta(a, da); split_meta(b, db)
bad = 0
for f in sorted(set(a) | set(b)):
    if f.startswith('__hip_cuid_'): continue   # hash of the source text
    if f not in a or f not in b: print('ONLY IN', 'A' if f in a else 'B', f); bad += 1
    elif a[f] != b[f]:
        bad += 1; print('DIFFERS', f, len(a[f]), len(b[f]))
        for x, y in zip(a[f], b[f]):
            if x != y: print('   A:', x, '\n   B:', y); break
for k in sorted(set(da) | set(db)):
    if da.get(k) != db.get(k): bad += 1; print('DESCRIPTOR DIFFERS', k, da.get(k), db.get(k))
print(sum(len(v) for v in a.values()), 'instruction lines in A,', sum(len(v) for v in b.values()), 'in B')
print('%d functions, %d kernel descriptors compared, %d differences' % (len(set(a) | set(b)), len(set(da) | set(db)), bad))
print('LDS max', max(int(l.split()[1]) for d in db.values() for l in d if l.startswith('.amdhsa_group_segment')), 'scratch', sorted({int(l.split()[1]) for d in db.values() for l in d if l.startswith('.amdhsa_private_segment')}))
sys.exit(1 if bad else 0)
