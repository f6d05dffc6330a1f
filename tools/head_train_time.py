#!/usr/bin/env python3
"""What training a frozen encoder's `logits` head costs: vnf_head_train_step alone at three shapes (device time per step
from events around a window of enqueued steps, the launches a step makes, and the bytes the update has to move:
parameter + two Adam moments, read and written = 6 * C * 512 * 4), and one epoch of train.py's facenet_aug loop with
IResNet-100 at batch 64 (augmentation -> encoder features -> step, per batch one loss / hit read by the host).
A record (profiles/head_train_time.txt), not a gate; bench.py does not call this.

    python tools/head_train_time.py [--steps 200] [--warmup 20] [--images 512] [--dtype bf16] > profiles/head_train_time.txt
"""
import argparse
import ctypes
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ((64, 1020), (64, 10575), (256, 1020))     # (b, C): the reference's size, the casia-webface width, a large batch
LAUNCHES = {True: 4, False: 3}                      # head_logits, softmax_nll, reduce_rows (+ head_update): csrc/head_train.hip


def step_times(b, c, steps, warmup):
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    w, bias = torch.randn(c, 512, generator=g) * 0.04, torch.randn(c, generator=g) * 0.04
    descs, n, keep = _lib.make_descs({"logits.weight": w, "logits.bias": bias})
    h = ctypes.c_void_p()
    _lib.check(lib.vnf_head_trainer_create(descs, n, c, b, 0.9, 0.999, 1e-8, 1e-4, ctypes.byref(h)))
    feat = torch.randn(b, 512, generator=g).to(dev)
    t = torch.randint(0, c, (b,), generator=g).to(dev)
    loss, hits = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = {}
    for train in (True, False):
        def fn():
            _lib.check(lib.vnf_head_train_step(h, ctypes.c_void_p(feat.data_ptr()), ctypes.c_void_p(t.data_ptr()), b, 1e-3, int(train),
                                               ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(hits.data_ptr()), _lib.current_stream_ptr()))
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[train] = e0.elapsed_time(e1) / steps * 1e3
    lib.vnf_destroy(h)
    return out


def epoch_time(images, dtype):
    """One epoch of ClassificationTrainer._train_epoch's body on `images` random 112 x 112 faces, batch 64, facenet_aug."""
    from vn_celeb_face_recognition_amd import augment, models
    from vn_celeb_face_recognition_amd.trainer import TrainableHead
    dev = torch.device("cuda:0")
    enc = models.iresnet100(n_classes=1020, freeze_weights=True, compute_dtype=dtype, max_batch=64).to(dev)
    head = TrainableHead(enc, lr=1e-3, weight_decay=1e-4, max_batch=64)
    g = torch.Generator().manual_seed(1)
    faces = torch.randint(0, 256, (images, 112, 112, 3), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 1020, (images,), generator=g)
    tf = augment.get_transform("facenet_aug")

    def epoch():
        for i in range(0, images, 64):
            index = torch.arange(i, min(i + 64, images))
            x = augment.augment_faces_device(faces, index, tf.params(int(index.numel()), 112, 112), 112, dtype=head.x_dtype)
            head.step(head.features(x), labels[index], train=True)
    epoch()                                         # warm-up: tile choice, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    epoch()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_train_time.py measures on the MI355X: no GPU is visible")
    print("# vnf_head_train_step: us per step (device events around %d enqueued steps after %d warm-up), launches per step" % (args.steps, args.warmup))
    print("# b | C | train us | launches | eval us | launches | update traffic MB (6*C*512*4) | GB/s of the whole training step")
    for b, c in SHAPES:
        us = step_times(b, c, args.steps, args.warmup)
        mb = 6.0 * c * 512 * 4 / 1e6
        print("%4d | %6d | %9.1f | %d | %9.1f | %d | %8.2f | %8.1f" % (b, c, us[True], LAUNCHES[True], us[False], LAUNCHES[False], mb,
                                                                      mb / us[True] * 1e3), flush=True)
    s = epoch_time(args.images, args.dtype)
    nb = (args.images + 63) // 64
    print("facenet_aug epoch, iresnet100(n_classes=1020, freeze_weights) %s, %d images in %d batches of 64: %.1f ms wall "
          "(%.2f ms per batch, %.0f images/s), host reads loss and hits every batch" % (args.dtype, args.images, nb, s * 1e3, s * 1e3 / nb, args.images / s))


if __name__ == "__main__":
    main()
