#!/usr/bin/env python3
"""What a gallery search costs: vnf_gallery_search (csrc/gallery.hip) at dim 512 for G in {1 000, 100 000, 1 000 000} x
F in {1, 64, 256} x k in {1, 16}: microseconds per search (device events, after a warm-up), the gallery's bytes
(G * dim * 4) over that time beside the 6.29 TB/s of a device copy, and, as a comparison line only,
torch.topk(q @ g.T, k) on the same (already normalised) tensors.  A record (profiles/gallery_time.txt), not a gate;
bench.py does not call this.

    python tools/gallery_time.py [--gs 1000,100000,1000000] [--fs 1,64,256] [--ks 1,16] [--steps 20] [--warmup 3] --out profiles/gallery_time.txt
"""
import argparse
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_TBS = 6.29     # device copy rate the other profiles quote
DIM = 512


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
    return e0.elapsed_time(e1) / steps * 1e3     # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gs", default="1000,100000,1000000")
    ap.add_argument("--fs", default="1,64,256")
    ap.add_argument("--ks", default="1,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    _lib.check(lib.vnf_init(0))
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = ["# vnf_gallery_search, dim %d fp32, default chunk_rows: us per search over %d calls after %d warm-up (device events)"
             % (DIM, args.steps, args.warmup),
             "# share: gallery bytes (G * dim * 4) / time beside the %.2f TB/s of a device copy; torch: topk(q @ g.T, k) on the same "
             "normalised tensors, comparison only" % COPY_TBS,
             "#       G |   F |  k | search us | gallery GB/s | share of copy | torch us | same top-1 rows"]
    for G in [int(v) for v in args.gs.split(",")]:
        h = ctypes.c_void_p()
        _lib.check(lib.vnf_gallery_create(DIM, G, ctypes.byref(h)))
        for g0 in range(0, G, 100000):
            n = min(100000, G - g0)
            rows = torch.randn((n, DIM), generator=gen, device=dev)
            labels = torch.arange(g0, g0 + n, dtype=torch.int32, device=dev)
            _lib.check(lib.vnf_gallery_add(h, ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(labels.data_ptr()), n, None))
        gm = torch.empty((G, DIM), dtype=torch.float32, device=dev)
        _lib.check(lib.vnf_gallery_rows(h, ctypes.c_void_p(gm.data_ptr()), 0, G, None))
        torch.cuda.synchronize()
        for F in [int(v) for v in args.fs.split(",")]:
            q = torch.randn((F, DIM), generator=gen, device=dev)
            qn = torch.nn.functional.normalize(q)
            for k in [int(v) for v in args.ks.split(",")]:
                nbytes = lib.vnf_gallery_search_workspace_bytes(F, k, G, 0)
                ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
                idx = torch.empty((F, k), dtype=torch.int32, device=dev)
                lab = torch.empty((F, k), dtype=torch.int32, device=dev)
                sc = torch.empty((F, k), dtype=torch.float32, device=dev)
                stream = _lib.current_stream_ptr()

                def ours():
                    _lib.check(lib.vnf_gallery_search(h, ctypes.c_void_p(q.data_ptr()), F, k, ctypes.c_void_p(idx.data_ptr()),
                                                      ctypes.c_void_p(lab.data_ptr()), ctypes.c_void_p(sc.data_ptr()), 0,
                                                      ctypes.c_void_p(ws.data_ptr()), nbytes, stream))

                us = timed(ours, args.steps, args.warmup)
                us_t = timed(lambda: torch.topk(qn @ gm.T, k), args.steps, args.warmup)
                same = int((torch.topk(qn @ gm.T, k).indices[:, 0].to(torch.int32) == idx[:, 0]).sum())
                gbs = G * DIM * 4 / us / 1e3
                lines.append("%9d | %3d | %2d | %9.1f | %12.1f | %11.1f %% | %8.1f | %d of %d"
                             % (G, F, k, us, gbs, 100.0 * gbs / (COPY_TBS * 1e3), us_t, same, F))
                print(lines[-1], flush=True)
        lib.vnf_destroy(h)
        del gm
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
