#!/usr/bin/env python3
"""Throughput of the emotion network (ResNet-50, two heads) on one MI355X: faces/s and the plan's TFLOP/s at a batch
size per compute dtype, the per-op table of the profile hook, and the resident recognize path (u8 faces -> transform
-> network -> top-k).  Prints one JSON line per dtype; bench.py does not call this.

    python tools/emotion_time.py [--bs 256] [--dtypes bf16,f16x2] [--steps 20] [--warmup 5] [--profile] [--accuracy]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--dtypes", default="bf16,f16x2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--face_size", type=int, default=112)
    ap.add_argument("--profile", action="store_true", help="print the per-op table of one forward")
    ap.add_argument("--accuracy", action="store_true", help="relative L2 per row against tests/golden/rn50_2b_seed0.npz")
    args = ap.parse_args()
    from vn_celeb_face_recognition_amd import models
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x32 = torch.randn((args.bs, 3, 224, 224), generator=g)
    faces = torch.randint(0, 256, (args.bs, args.face_size, args.face_size, 3), generator=g, dtype=torch.uint8).to(dev)
    for dt in args.dtypes.split(","):
        m = models.resnet_2branch_50(num_classes=690, compute_dtype=dt, max_batch=max(args.bs, 2)).to(dev).eval()
        x = x32.to(dev).to({"bf16": torch.bfloat16, "f16": torch.float16}.get(dt, torch.float32))
        ms = timed(lambda: m(x), args.steps, args.warmup)
        ms_rec = timed(lambda: m.recognize(faces, 6), args.steps, args.warmup)
        alg, exe = m.flops_per_image()
        res = {"arch": "rn50_2b", "dtype": dt, "bs": args.bs, "ms_forward": round(ms, 4), "faces_per_s_forward": round(args.bs / ms * 1e3, 1),
               "tflops_alg": round(alg * args.bs / ms / 1e9, 1), "gflop_alg_per_image": round(alg / 1e9, 3),
               "gflop_exec_per_image": round(exe / 1e9, 3), "ms_recognize": round(ms_rec, 4),
               "faces_per_s_recognize": round(args.bs / ms_rec * 1e3, 1)}
        if args.accuracy:
            gd = np.load(os.path.join(REPO, "tests", "golden", "rn50_2b_seed0.npz"))
            xg = torch.randn((2, 3, 224, 224), generator=torch.Generator().manual_seed(int(gd["input_seed"])))
            c, p = m(xg.to(dev))
            for name, got, want in (("x_cls", c, gd["x_cls"]), ("x_proj", p, gd["x_proj"])):
                rel = np.linalg.norm(got.cpu().numpy() - want, axis=1) / np.linalg.norm(want, axis=1)
                res["rel_l2_" + name] = [float("%.3e" % r) for r in rel]
        print(json.dumps(res), flush=True)
        if args.profile:
            print(m.profile(x), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
