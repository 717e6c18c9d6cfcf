"""Compare the gfx950 assembly of two `build.py --keep-temps` builds kernel by kernel: which kernels of the first build
are instruction for instruction the same in the second.  Labels, comments and the kernel's own (mangled) name are
normalised; a kernel whose name gained a defaulted template argument (`..., false>` / `..., -1, false>`) is matched to
its new name, and so is a kernel that became a template on one flag (`dense_fwd_kernel` -> `dense_fwd_kernel<false>`),
also where the flag came with a trailing `XTrainParams` argument (`kron_dense_group_kernel<3>(p, gsplit)` ->
`kron_dense_group_kernel<3, false>(p, gsplit, XTrainParams)`).  A unit the first build does not have is listed as new.  Metadata lines (.amdhsa_*) are reported separately from instructions.  --sgpr renames every SGPR
(`s12`, `s[28:29]`) to one placeholder first: a change to a kernel's arguments renumbers the scalar registers of the
whole kernel, and this leaves only the lines that changed otherwise.
usage: isa_diff.py [--sgpr] OLD_BUILD_DIR NEW_BUILD_DIR [UNIT ...]   (units default: every unit of build.SOURCES)"""
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodalfusion_amd import build as B   # noqa: E402


def kernels(path, sgpr=False):
    out = {}
    for m in re.finditer(r"; -- Begin function (\S+)\n(.*?); -- End function", open(path).read(), re.S):
        body = re.sub(r"\.Lfunc_end\d+|\.LBB\d+_\d+|\.Ltmp\d+|\.Lpost_getpc\d+", "L", m.group(2).replace(m.group(1), "FN"))
        if sgpr:
            body = re.sub(r"\bs(\d+|\[\d+:\d+\])(?![\w:])", "sX", body)
        lines = [l.split(";")[0].rstrip() for l in body.splitlines()]
        out[m.group(1)] = [l for l in lines if l]
    return out


def main():
    args = sys.argv[1:]
    sgpr = "--sgpr" in args
    args = [x for x in args if x != "--sgpr"]
    old, new = args[0], args[1]
    units = args[2:] or [s.replace(".hip", "") for s in B.SOURCES]
    for u in units:
        f = f"{u}-hip-amdgcn-amd-amdhsa-gfx950.s"
        if not os.path.exists(os.path.join(old, f)):
            print(f"{u}: new unit, {len(kernels(os.path.join(new, f)))} kernels")
            continue
        a, b = kernels(os.path.join(old, f), sgpr), kernels(os.path.join(new, f), sgpr)
        same = meta_only = 0
        for k, v in sorted(a.items()):
            tail = lambda n: re.sub(r"NS_\d+XTrainParamsE$", "", n)
            cands = [n for n in b if n == k or n.replace("Lb0EEEv", "EEv") == k or n.replace("ELb0EEEvNS", "EEvNS") == k
                     or n.replace("ILb0EEEvNS", "ENS") == k or tail(n).replace("ILb0EEEvNS", "ENS") == k
                     or tail(n).replace("Lb0E", "", 1) == k]
            if not cands:
                print(f"{u}: {k}: not found in the new build")
                continue
            w = b[cands[0]]
            if w == v:
                same += 1
                continue
            d = [l for l in difflib.unified_diff(v, w, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
            if all(".amdhsa_" in l for l in d):
                meta_only += 1
                print(f"{u}: {k}: instructions identical; metadata {' / '.join(l.strip() for l in d)}")
            else:
                print(f"{u}: {k}: {sum(1 for l in d if l.startswith('-'))} lines -> {sum(1 for l in d if l.startswith('+'))}")
        count = f"{len(a)} kernels" if len(a) == len(b) else f"{len(a)} -> {len(b)} kernels"
        print(f"{u}: {count}: {same} identical, {meta_only} identical instructions (metadata differs), "
              f"{len(a) - same - meta_only} differ")


if __name__ == "__main__":
    main()
