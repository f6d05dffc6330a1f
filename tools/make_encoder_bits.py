#!/usr/bin/env python3
"""Record tests/golden/encoder_bits.json on the MI355X: the SHA-256 and absolute sum of the embeddings the seed-0
InceptionResnetV1 produces on the cases of tests/encoder_bits.py (compute dtype x VNF_FUSE x batch size), and the
torch / hipcc versions they were produced under.  tests/test_gpu_encoder_bits.py replays the cases against the file, so
record it on the commit whose arithmetic is to be kept, BEFORE a change to the fused-stack kernels, never after.

    python tools/make_encoder_bits.py [output.json]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from encoder_bits import CASES, case_id, run_case, versions  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("make_encoder_bits.py records on the MI355X: no GPU is visible")
    out = dict(versions(), cases={case_id(*c): run_case(*c) for c in CASES})
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "encoder_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
