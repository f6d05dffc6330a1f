#!/usr/bin/env python3
"""Record tests/golden/gallery_bits.json on the MI355X: per case of tests/gallery_bits.py (rows, search, mated search,
cluster, tracks, track sums x dim x chunking) the SHA-256 and absolute sum of every output array of the gallery family's
C ABI, the commit they were produced on and the torch / hipcc versions they were produced under.
tests/test_gpu_gallery_bits.py replays the cases against the file, so record it on the commit whose arithmetic is to be
kept, BEFORE a change to csrc/gallery_core.h or the kernels on it, never after.

    python tools/make_gallery_bits.py [--commit HASH] [output.json]

--commit: the commit the library was built from, for a tree that is no git checkout (default: git rev-parse HEAD).  In a
checkout it has to be HEAD, and the gallery sources have to be unmodified: the file names the commit whose bits it holds.
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from gallery_bits import CASES, run_case, versions  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("make_gallery_bits.py records on the MI355X: no GPU is visible")
    args = sys.argv[1:]
    git = lambda *a: subprocess.run(["git", "-C", REPO] + list(a), capture_output=True, text=True)
    head = git("rev-parse", "HEAD")
    if head.returncode == 0:
        if git("status", "--porcelain", "--", "vn_celeb_face_recognition_amd/csrc").stdout.strip():
            raise SystemExit("make_gallery_bits.py: csrc/ differs from HEAD; record on a commit, not on a modified tree")
        if args[:1] == ["--commit"] and args[1] != head.stdout.strip():
            raise SystemExit("make_gallery_bits.py: --commit %s is not this checkout's HEAD %s" % (args[1], head.stdout.strip()))
    elif args[:1] != ["--commit"]:
        raise SystemExit("make_gallery_bits.py: no git checkout here; name the commit the library was built from with --commit")
    commit = args[1] if args[:1] == ["--commit"] else head.stdout.strip()
    args = args[2:] if args[:1] == ["--commit"] else args
    out = dict(versions(), recorded_on_commit=commit, cases={c: run_case(c) for c in CASES})
    path = args[0] if args else os.path.join(REPO, "tests", "golden", "gallery_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
