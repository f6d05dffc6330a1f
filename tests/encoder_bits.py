"""Shared by tests/test_gpu_encoder_bits.py and tools/make_encoder_bits.py: the exact embeddings of the seed-0
InceptionResnetV1 through every fused-stack kernel (csrc/stem_mid*.hip, block35*.hip, trunk35.hip, trunk17*.hip,
block8.hip), recorded per case as the SHA-256 of the embedding bytes and their absolute sum in hex.  Only the public
model call is used, so the same run can be recorded on one commit and replayed on another.

A case is (compute dtype, VNF_FUSE, batch size):
  dtype     bf16 and f16 (the 16-bit kernels, both template instantiations), f16x2 (the planar split-f16 twins);
  VNF_FUSE  unset (the default switch: stem with conv2d_3b, Block35 stack or the per-block planar twin, Block17 stack,
            Block8 chain), 2 (the per-block Block35 kernel alone, off the default 16-bit path), 4 (the stem kernel
            without conv2d_3b, its other instantiation);
  batch     1 (all the per-image kernels need) and 4 (the smallest that gives Block8 a full group of three and a partial one).
No combination is dropped: f16x2 under VNF_FUSE=4 activates no fused stack (the planar stem kernel always carries
conv2d_3b), so it runs the per-convolution plan alone, which no other listed case does.

The switches are read when a handle is created, so each (dtype, VNF_FUSE) is a model of its own, max_batch = 8, with the
heuristic tiles (VNF_AUTOTUNE=0: quick creates, and no tile choice that depends on a timing); both batch sizes run on it."""
import hashlib
import os
import subprocess

import numpy as np
import torch

from conftest import seeded_normal

DTYPES = ("bf16", "f16", "f16x2")
FUSES = (None, "2", "4")          # None: VNF_FUSE unset
BATCHES = (1, 4)
CASES = tuple((dt, fuse, n) for dt in DTYPES for fuse in FUSES for n in BATCHES)
MAX_BATCH = 8
INPUT_SEED = 4242
_models = {}
_input = []


def case_id(dt, fuse, n):
    return "%s-fuse_%s-n%d" % (dt, "default" if fuse is None else fuse, n)


def _model(dt, fuse):
    if (dt, fuse) not in _models:
        from vn_celeb_face_recognition_amd.models import InceptionResnetV1
        keep = {k: os.environ.get(k) for k in ("VNF_FUSE", "VNF_AUTOTUNE")}
        os.environ["VNF_AUTOTUNE"] = "0"
        if fuse is None:
            os.environ.pop("VNF_FUSE", None)
        else:
            os.environ["VNF_FUSE"] = fuse
        try:
            m = InceptionResnetV1(pretrained=None, device="cuda:0", compute_dtype=dt, max_batch=MAX_BATCH).eval()
            m._ensure_handle()                           # the handle reads the switches here
        finally:
            for k, v in keep.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        _models[(dt, fuse)] = m
    return _models[(dt, fuse)]


def _x(n):
    """The first n of the seeded fp32 crops (image i is the same tensor at every batch size)."""
    if not _input:
        _input.append(seeded_normal((max(BATCHES), 3, 160, 160), INPUT_SEED).cuda())
    return _input[0][:n].contiguous()


def run_case(dt, fuse, n):
    emb = np.ascontiguousarray(_model(dt, fuse)(_x(n)).cpu().numpy(), dtype=np.float32)
    assert emb.shape == (n, 512) and np.isfinite(emb).all(), (dt, fuse, n, emb.shape)
    return {"sha256": hashlib.sha256(emb.tobytes()).hexdigest(), "abs_sum": float(np.abs(emb.astype(np.float64)).sum()).hex()}


def versions():
    """The toolchain a record was made under / a test runs under: torch and the hipcc that builds the library."""
    from vn_celeb_face_recognition_amd.build import HIPCC
    try:
        hipcc = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.strip()
    except OSError as e:
        hipcc = "unavailable: %s" % e
    return {"torch": torch.__version__, "hipcc": hipcc}
