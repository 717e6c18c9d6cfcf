#!/usr/bin/env python3
"""The tuning build of the library: the product kernels with the launchers' MMF_* environment overrides compiled in
(-DMMF_TUNE, csrc/mmf_common.h: tune_int).  The shipped library reads no environment variable; the sweep tools under
tools/ load this one (tools/README.md lists the overrides).

    python tools/diag_build.py [tune]      # -> multimodalfusion_amd/_diag/libmmf_tune.so
    MMF_LIB_PATH=multimodalfusion_amd/_diag/libmmf_tune.so MMF_GATE_BIG_MIN=... python bench.py ...
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodalfusion_amd import build as B   # noqa: E402


def main():
    if sys.argv[1:] not in ([], ["tune"]):
        raise SystemExit("usage: diag_build.py [tune]")
    out_dir = os.path.join(B.HERE, "_diag")
    objdir = os.path.join(B.OBJ, "diag_tune")
    os.makedirs(out_dir, exist_ok=True)
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    objs = []
    for s in B.SOURCES:
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        jobs.append([B.HIPCC] + B.FLAGS + B.FILE_FLAGS.get(s, []) + ["-DMMF_TUNE", "-c", os.path.join(B.CSRC, s), "-o", obj])
    with ThreadPoolExecutor(max_workers=4) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            if r.returncode != 0:
                raise SystemExit(r.stderr[-3000:])
    lib = os.path.join(out_dir, "libmmf_tune.so")
    subprocess.check_call([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    print(lib)


if __name__ == "__main__":
    main()
