"""Build libvnface.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

    python -m vn_celeb_face_recognition_amd.build [--force] [--stamps]

The shared object lands next to this file so it travels with a repository snapshot; it is
git-ignored.  hipcc cross-compiles gfx950 without a GPU present.

--stamps compiles with -DVNF_STAMPS: the instrumented kernels and launchers behind the VNF_*_STAMP
variables (tools/stamp_patch.py, tools/stamp_ws.py).  Its objects live in a directory of their own, and
whichever kind was built last is what libvnface.so holds; the default build is the product.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "csrc", "build")
LIB = os.path.join(HERE, "libvnface.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
         "-fno-gpu-rdc", "-ffp-contract=off"]


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))


def _headers_mtime():
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hs.append(os.path.join(os.path.dirname(HERE), "include", "vnface.h"))
    return max(os.path.getmtime(h) for h in hs)


def build(force=False, verbose=True, stamps=False):
    obj_dir = os.path.join(OBJ, "stamps") if stamps else OBJ
    flags = FLAGS + (["-DVNF_STAMPS"] if stamps else [])
    kind_file = os.path.join(OBJ, "linked_kind")   # which kind of objects libvnface.so was last linked from
    kind = "stamps" if stamps else "default"
    os.makedirs(obj_dir, exist_ok=True)
    hm = _headers_mtime()
    jobs = []
    objs = []
    for src in _sources():
        sp = os.path.join(CSRC, src)
        op = os.path.join(obj_dir, src + ".o")
        objs.append(op)
        if force or not os.path.exists(op) or os.path.getmtime(op) < max(os.path.getmtime(sp), hm):
            cmd = [HIPCC] + flags + (["-x", "hip"] if src.endswith(".hip") else []) + ["-c", sp, "-o", op]
            jobs.append((src, cmd))

    def run(job):
        src, cmd = job
        r = subprocess.run(cmd, capture_output=True, text=True)
        return src, r.returncode, r.stdout + r.stderr

    if jobs:
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            for src, rc, out in ex.map(run, jobs):
                if verbose and out.strip():
                    print(out, file=sys.stderr)
                if rc != 0:
                    raise RuntimeError("hipcc failed on %s:\n%s" % (src, out))
    linked = open(kind_file).read().strip() if os.path.exists(kind_file) else None
    if jobs or not os.path.exists(LIB) or force or linked != kind:
        cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n" + r.stdout + r.stderr)
        with open(kind_file, "w") as f:
            f.write(kind + "\n")
        if verbose:
            print("built", LIB, "(%d objects, %d recompiled)" % (len(objs), len(jobs)))
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, stamps="--stamps" in sys.argv)
