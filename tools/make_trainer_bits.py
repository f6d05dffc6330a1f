#!/usr/bin/env python3
"""Record tests/golden/trainer_bits.json on the MI355X: the bits both on-device trainers produce on the seeded runs of
tests/trainer_bits.py (hashes of every parameter and Adam moment, losses in hex, hit counts, step counters) and the
torch / hipcc versions they were produced under.  tests/test_gpu_trainer_bits.py replays the runs against the file, so
record it on the commit whose arithmetic is to be kept, BEFORE a change to the trainers, never after.

    python tools/make_trainer_bits.py [output.json]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from trainer_bits import CASES, case_id, run_case, versions  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("make_trainer_bits.py records on the MI355X: no GPU is visible")
    out = dict(versions(), cases={case_id(kind, shape): run_case(kind, shape) for kind, shape in CASES})
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "trainer_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
