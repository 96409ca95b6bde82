#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of iyokan_hip.hip (hipcc ... --cuda-device-only -S):  python tools/codeobj_diff.py OLD.s NEW.s
For a change that must leave the device code alone: same kernel names, and each kernel's text from its label to the end of its descriptor
(code, VGPRs, LDS, scratch) identical.  Exit status 1 when a kernel differs.  (profiles/dispatch_refactor_codeobj.txt is its output.)"""
import hashlib, re, sys
def kernels(path):
    text = open(path).read().splitlines()
    names = [l.split()[1] for l in text if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for n in names:
        lo = next(i for i, l in enumerate(text) if l.startswith(n + ":"))
        start = next(i for i, l in enumerate(text) if l.strip() == ".amdhsa_kernel " + n)
        hi = next(i for i in range(start, len(text)) if text[i].strip() == ".end_amdhsa_kernel")
        # local labels carry the function's ordinal in the file (.LBB33_2, .Lfunc_end33): the ordinal follows the ORDER of the kernels
        body = re.sub(r"\b(\.?L?BB|\.Lfunc_(?:begin|end)|\.LJTI|\.LCPI)\d+", r"\1#", "\n".join(re.sub(r"\s*;.*$", "", l) for l in text[lo:hi + 1]))
        out[n] = (hashlib.sha256(body.encode()).hexdigest()[:16], hi + 1 - lo)
    return names, out
pn, pk = kernels(sys.argv[1]); bn, bk = kernels(sys.argv[2])
print("device code of iyokan_hip.hip, old (parent) vs new (branch): hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --cuda-device-only -S -DIYK_BUILD_ID='\"x\"'")
print("per kernel: sha256[:16] of the text from the kernel's label to .end_amdhsa_kernel (code and descriptor: VGPRs, LDS, scratch), lines;")
print("the function ordinal inside local labels (.LBB<k>_, .Lfunc_end<k>) is masked, since it numbers the kernels in file order,\nand the compiler's comments (from ';' on, padded to a column that depends on the label's width) are dropped")
print(f"kernels: parent {len(pn)}, branch {len(bn)}; same names: {sorted(pn) == sorted(bn)}; same order: {pn == bn}")
bad = 0
for n in sorted(set(pn) | set(bn)):
    a, b = pk.get(n), bk.get(n)
    same = a == b
    bad += not same
    print(f"{'same' if same else 'DIFF'}  parent {a[0] if a else '-':16s} {a[1] if a else 0:6d}  branch {b[0] if b else '-':16s} {b[1] if b else 0:6d}  {n}")
print(f"differing kernels: {bad}")
for title, names in (("old", pn), ("new", bn)):
    print(f"\nkernel names in file order, {title}:")
    for n in names:
        print("  " + n)
sys.exit(1 if bad else 0)
