#!/usr/bin/env python3
"""What the classification head costs: vnf_encoder_logprobs against vnf_embed on the SAME handle, InceptionResnetV1 with a
10575-way `logits` layer (the casia-webface width) at a batch size per compute dtype; and vnf_logits_eval alone on a
matrix of that shape.  A record (profiles/heads_time.txt), not a gate; bench.py does not call this.

    python tools/heads_time.py [--bs 256] [--classes 10575] [--dtypes bf16,f16x2] [--steps 20] [--warmup 5] > profiles/heads_time.txt
"""
import argparse
import os
import sys

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
    ap.add_argument("--classes", type=int, default=10575)
    ap.add_argument("--dtypes", default="bf16,f16x2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.classifier import logits_eval
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x32 = torch.randn((args.bs, 3, 160, 160), generator=g)
    print("# InceptionResnetV1(classify=True, num_classes=%d), bs %d: ms per call, %d calls after %d warm-up, one handle per dtype"
          % (args.classes, args.bs, args.steps, args.warmup))
    print("# dtype | vnf_embed ms | vnf_encoder_logprobs ms | head + log_softmax ms | share of the call | images/s with the head")
    for dt in args.dtypes.split(","):
        m = models.InceptionResnetV1(pretrained=None, classify=True, num_classes=args.classes, compute_dtype=dt,
                                     max_batch=args.bs).to(dev).eval()
        x = x32.to(dev).to({"bf16": torch.bfloat16, "f16": torch.float16}.get(dt, torch.float32))
        ms_e = timed(lambda: m.embed(x), args.steps, args.warmup)
        ms_l = timed(lambda: m.logprobs(x), args.steps, args.warmup)
        ms_e2 = timed(lambda: m.embed(x), args.steps, args.warmup)      # again, after: the order of the two legs does not matter
        ms_e = min(ms_e, ms_e2)
        print("%-6s | %12.4f | %23.4f | %21.4f | %15.2f %% | %10.1f"
              % (dt, ms_e, ms_l, ms_l - ms_e, 100.0 * (ms_l - ms_e) / ms_l, args.bs / ms_l * 1e3), flush=True)
        del m
        torch.cuda.empty_cache()
    logits = (torch.randn((args.bs, args.classes), generator=g) * 5).to(dev)
    t = torch.randint(0, args.classes, (args.bs,), generator=g)
    mb = args.bs * args.classes * 4 / 1e6
    for want, label in ((("amax", "prob", "nll", "hit", "sums"), "rows + sums, no logp"),
                        (("logp", "amax", "prob", "nll", "hit", "sums"), "rows + sums + logp")):
        ms = timed(lambda: logits_eval(logits, t, want=want), 10 * args.steps, args.warmup)
        traffic = mb * (2 if "logp" in want else 1)
        print("vnf_logits_eval (%d,%d) %-20s: %7.1f us per call incl. the label upload, %6.2f MB algorithmic, %6.1f GB/s"
              % (args.bs, args.classes, label, ms * 1e3, traffic, traffic / ms), flush=True)


if __name__ == "__main__":
    main()
