#!/usr/bin/env python3
"""Throughput of the SE-IR ResNet-101 encoder (models.resnet101(use_se=True)) on one MI355X, with iresnet100 beside it
for scale, and what its squeeze-and-excitation ops cost.  Writes profiles/seir101_time.txt; bench.py does not call this.

    python tools/seir101_time.py [--bs 256] [--dtypes bf16,f16x2] [--steps 20] [--warmup 5] [--out profiles/seir101_time.txt]

Per dtype: the two encoders are timed alternately in one process (device events around `steps` forwards after `warmup`
unrecorded ones, two rounds each; the lower is kept): ms per step, embeddings/s, algorithmic GFLOP per step and its
share of the 2.5 PFLOP/s dense 16-bit peak.  From one vnf_encoder_profile run (events between the plan's ops, so launch
gaps are in): the 33 SE ops' summed time, their algorithmic bytes (t read for the mean, t and the residual read again,
the result written: four tensors per block) and the rate that gives, beside the 6.29 TB/s of a plain device copy.
No number here is a pass / fail bar."""
import argparse
import os
import re
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_TFLOPS = 2500.0
COPY_TBS = 6.29


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seir101_time.txt"))
    args = ap.parse_args()
    from vn_celeb_face_recognition_amd import models
    dev = torch.device("cuda:0")
    x32 = torch.randn((args.bs, 3, 112, 112), generator=torch.Generator().manual_seed(0))
    lines = ["SE-IR ResNet-101 vs IResNet-100, %s, batch %d, %d warm-up + %d timed steps per round, two alternating rounds"
             % (torch.cuda.get_device_name(0), args.bs, args.warmup, args.steps)]
    for dt in args.dtypes.split(","):
        x = x32.to(dev).to({"bf16": torch.bfloat16, "f16": torch.float16}.get(dt, torch.float32))
        encs = {"resnet101_se": models.resnet101(use_se=True, compute_dtype=dt, max_batch=args.bs).to(dev).eval(),
                "iresnet100": models.iresnet100(compute_dtype=dt, max_batch=args.bs).to(dev).eval()}
        ms = {k: float("inf") for k in encs}
        for _ in range(2):
            for k, m in encs.items():
                ms[k] = min(ms[k], timed(lambda: m(x), args.steps, args.warmup))
        for k, m in encs.items():
            alg, _ = m.flops_per_image()
            gf = alg * args.bs / 1e9
            tf = gf / ms[k]
            lines.append("%-5s %-13s %8.3f ms/step %9.1f emb/s %9.1f GFLOP/step (algorithmic) %7.1f TFLOP/s = %4.1f %% of %.0f"
                         % (dt, k, ms[k], args.bs / ms[k] * 1e3, gf, tf, 100.0 * tf / PEAK_TFLOPS, PEAK_TFLOPS))
        rep = encs["resnet101_se"].profile(x)
        se_ms = se_mb = 0.0
        for ln in rep.splitlines():
            hit = re.search(r"\.se\s+se .* ([0-9.]+) ms\s+([0-9.]+) MB", ln)
            if hit:
                se_ms += float(hit.group(1))
                se_mb += float(hit.group(2))
        total = float(re.search(r"TOTAL ([0-9.]+) ms", rep).group(1))
        lines.append("%-5s resnet101_se  SE ops (33 x squeeze + excite/apply): %.3f ms of the profile's %.3f ms, %.1f MB algorithmic "
                     "-> %.2f TB/s (device copy: %.2f TB/s)" % (dt, se_ms, total, se_mb, se_mb / se_ms / 1e3 if se_ms else 0.0, COPY_TBS))
        by_stage = {}
        for ln in rep.splitlines():
            hit = re.search(r"(layer\d)\.\d+\.se\s+se (\S+) .* ([0-9.]+) ms\s+([0-9.]+) MB", ln)
            if hit:
                a = by_stage.setdefault(hit.group(1), [hit.group(2), 0, 0.0, 0.0])
                a[1] += 1; a[2] += float(hit.group(3)); a[3] += float(hit.group(4))
        for st, (shape, cnt, t, mb) in sorted(by_stage.items()):
            lines.append("%-5s   %s %-12s %2d blocks %8.4f ms %9.1f MB %6.2f TB/s" % (dt, st, shape, cnt, t, mb, mb / t / 1e3 if t else 0.0))
        del encs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
