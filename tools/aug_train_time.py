#!/usr/bin/env python3
"""What AugClassificationTrainer's training step costs on top of the frozen encoder.

For InceptionResnetV1 in f16x2 and bf16, at batch 64 and 256, in one process:
  step      images/s of the whole training step as the trainer runs it: the draws of transforms_facenet_aug on the
            host, their upload, vnf_augment_faces, the encoder, the fused MLP step and the read-back of the loss;
  encoder   emb/s of the same encoder alone on a resident batch of the same size and input dtype;
  augment   device time of vnf_augment_faces alone (HIP events around `--reps` launches) against the bytes it writes,
            n * 3 * T^2 * element size, the bound DESIGN.md 5 gives for it;
  draws     host time of draw_facenet_aug_params for one batch.

    python tools/aug_train_time.py [--steps 30] [--warmup 5] [--out profiles/aug_train_time.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vn_celeb_face_recognition_amd import _lib  # noqa: E402
from vn_celeb_face_recognition_amd import augment as A  # noqa: E402
from vn_celeb_face_recognition_amd.models import InceptionResnetV1  # noqa: E402
from vn_celeb_face_recognition_amd.trainer import TrainableMLP  # noqa: E402

DEV = "cuda:0"
X_DTYPE = {"f16x2": torch.float32, "bf16": torch.bfloat16}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--faces", type=int, default=2048, help="size of the synthetic resident data set")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_train_time.py measures on the MI355X: no GPU is visible")
    s = t = 160
    g = torch.Generator().manual_seed(5)
    faces = torch.randint(0, 256, (args.faces, s, s, 3), generator=g, dtype=torch.uint8).to(DEV)
    labels = torch.randint(0, args.classes, (args.faces,), generator=g)
    torch.manual_seed(123)
    lines = ["# InceptionResnetV1, %d resident %dx%d faces, %d classes, %d timed steps after %d warm-up" %
             (args.faces, s, s, args.classes, args.steps, args.warmup),
             "# dtype batch | step img/s | encoder emb/s | step/encoder | augment us  GB/s written | draws ms"]
    for cd in ("f16x2", "bf16"):
        enc = InceptionResnetV1(pretrained=None, compute_dtype=cd, max_batch=256).to(DEV).eval()
        xd = X_DTYPE[cd]
        for b in (64, 256):
            mlp = TrainableMLP(512, args.classes, lr=1e-4, weight_decay=1e-4, max_batch=b, device=DEV)

            def step():
                idx = torch.randint(0, args.faces, (b,))
                params = A.draw_facenet_aug_params(b, s, t)[0]
                emb = enc(A.augment_faces_device(faces, idx, params, t, dtype=xd))
                mlp.step(emb, labels[idx], train=True)
            t_step = timed(step, args.steps, args.warmup)
            x = A.augment_faces_device(faces, torch.arange(b), A.draw_facenet_aug_params(b, s, t)[0], t, dtype=xd)
            t_enc = timed(lambda: enc(x), args.steps, args.warmup)
            # the kernel alone: parameters and index already on the device
            params = A.draw_facenet_aug_params(b, s, t)[0]
            pdev = torch.from_numpy(params.view(np.uint8).reshape(-1).copy()).to(DEV)
            idev = torch.randint(0, args.faces, (b,), dtype=torch.int32).to(DEV)
            xo = torch.empty((b, 3, t, t), dtype=xd, device=DEV)
            lib, stream = _lib.load(), _lib.current_stream_ptr()
            call = (ctypes.c_void_p(faces.data_ptr()), args.faces, s, ctypes.c_void_p(idev.data_ptr()), ctypes.c_void_p(pdev.data_ptr()),
                    b, t, ctypes.c_void_p(xo.data_ptr()), _lib.torch_dtype_code(xd), None, stream)
            for _ in range(10):
                _lib.check(lib.vnf_augment_faces(*call))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                lib.vnf_augment_faces(*call)
            e1.record()
            torch.cuda.synchronize()
            t_aug = e0.elapsed_time(e1) * 1e-3 / args.reps
            out_bytes = b * 3 * t * t * torch.empty((), dtype=xd).element_size()
            t0 = time.perf_counter()
            for _ in range(20):
                A.draw_facenet_aug_params(b, s, t)
            t_draw = (time.perf_counter() - t0) / 20
            lines.append("%-5s %5d | %11.0f | %13.0f | %12.3f | %10.1f %13.1f | %8.2f" %
                         (cd, b, b / t_step, b / t_enc, t_enc / t_step, t_aug * 1e6, out_bytes / t_aug / 1e9, t_draw * 1e3))
            del mlp
        del enc
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
