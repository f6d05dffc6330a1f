#!/usr/bin/env python3
"""Generate tests/golden/seir101_seed0.npz and tests/golden/seir101_keys.json by RUNNING THE REFERENCE in the build
container (like tools/make_golden.py, whose import shim and seeded inputs it reuses; /root/reference does not exist on
the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_seir101_golden.py

The reference's resnet101(use_se=True, img_size=112) (models/resnet_encoder.py:246-254) takes this repository's
generator weights by a strict load_state_dict and embeds two seeded images on the CPU.

  seir101_seed0.npz   input_seed, features (2, 512): the unit-norm rows the reference returns
  seir101_keys.json   the reference module's state_dict: [name, shape] per tensor, in its order

Only outputs are written: no weights, no reference text."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import OUT, install_shim, ref, seeded_normal  # noqa: E402
from vn_celeb_face_recognition_amd.weights import generate_state_dict  # noqa: E402

INPUT_SEED = 5101


def golden_seir101():
    m = ref("resnet_encoder").resnet101(use_se=True, pretrained=False, img_size=112).eval()
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    m.load_state_dict(generate_state_dict("seir101", seed=0, as_torch=True), strict=True)
    x = seeded_normal((2, 3, 112, 112), INPUT_SEED)
    with torch.no_grad():
        y = m(x).numpy()
    print("seir101:", len(keys), "tensors,", sum(int(np.prod(s)) for _, s in keys), "elements; row norms",
          np.linalg.norm(y, axis=1).tolist())
    np.savez_compressed(os.path.join(OUT, "seir101_seed0.npz"), input_seed=np.int64(INPUT_SEED), features=y)
    with open(os.path.join(OUT, "seir101_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    install_shim()
    torch.manual_seed(0)
    golden_seir101()
