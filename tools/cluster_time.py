#!/usr/bin/env python3
"""What clustering a gallery costs: vnf_gallery_cluster (csrc/gallery_cluster.hip) at dim 512, threshold 0.5, min_samples 2,
for N in {10 000, 100 000, 300 000} rows of two kinds:

    sparse   random rows: almost no pair reaches the threshold, stage B's waves find nothing to do
    dense    100 identities of N / 100 near-duplicates each (cosine 0.92 inside one): every row is core, stage B unites
             N (N / 100 - 1) / 2 edges in 100 trees

The library runs its three stages in one call, so the stages are told apart by two timings of that call (device events,
after a warm-up): at threshold 2, which no cosine reaches, stage A (every pair scored, degrees, nearest neighbours) and
stage C run in full and stage B's waves leave at once; the call at threshold 0.5 less that is what stage B adds.  The
fp32 MFMA rate of a scoring stage is 2 N^2 512 FLOP over its time, set beside the 157 TFLOP/s peak and the 56-60 TFLOP/s
vnf_gallery_search reaches at F >= 64 (profiles/gallery_time.txt): the same stream, so a self-join well below it pays for
its epilogue, not for its stream.  In the dense case stage B scores about half the pairs (a wave of core rows stops at its
own last row), its rate is quoted for the pairs it does score.  torch: the neighbour count alone, (x[b] @ x.T >= t).sum(1)
over row blocks of the same unit rows, comparison only.  A record (profiles/cluster_time.txt), not a gate; bench.py does
not call this.  Every (N, kind) runs in a child process of its own under a time limit, and nothing runs after one fails.

    python tools/cluster_time.py [--ns 10000,100000,300000] [--steps 3] [--warmup 1] [--limit 240] --out profiles/cluster_time.txt
"""
import argparse
import ctypes
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_TF = 157.0
DIM = 512
T = 0.5


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
    return e0.elapsed_time(e1) / steps     # ms


def rows_of(kind, n, gen, dev):
    z = torch.nn.functional.normalize(torch.randn((n, DIM), generator=gen, device=dev))
    if kind == "sparse":
        return z
    centres = torch.nn.functional.normalize(torch.randn((100, DIM), generator=gen, device=dev))
    return centres[torch.arange(n, device=dev) % 100] + 0.3 * z


def one(kind, n, steps, warmup):
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    _lib.check(lib.vnf_init(0))
    gen = torch.Generator(device=dev).manual_seed(0)
    h = ctypes.c_void_p()
    _lib.check(lib.vnf_gallery_create(DIM, n, ctypes.byref(h)))
    x = rows_of(kind, n, gen, dev)
    labels = torch.zeros((n,), dtype=torch.int32, device=dev)
    _lib.check(lib.vnf_gallery_add(h, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(labels.data_ptr()), n, None))
    _lib.check(lib.vnf_gallery_rows(h, ctypes.c_void_p(x.data_ptr()), 0, n, None))     # x: the unit rows the library holds
    nbytes = lib.vnf_gallery_cluster_workspace_bytes(n, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    ints = [torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(3)]
    score = torch.empty((n,), dtype=torch.float32, device=dev)
    nc = torch.zeros((1,), dtype=torch.int32, device=dev)
    stream = _lib.current_stream_ptr()

    def ours(t):
        _lib.check(lib.vnf_gallery_cluster(h, t, 2, ctypes.c_void_p(ints[0].data_ptr()), ctypes.c_void_p(ints[1].data_ptr()),
                                           ctypes.c_void_p(ints[2].data_ptr()), ctypes.c_void_p(score.data_ptr()),
                                           ctypes.c_void_p(nc.data_ptr()), 0, ctypes.c_void_p(ws.data_ptr()), nbytes, stream))

    ms_ac = timed(lambda: ours(2.0), steps, warmup)
    ms_all = timed(lambda: ours(T), steps, warmup)
    deg, clusters = ints[1].clone(), int(nc.item())
    block = 2048

    def torch_count():
        return torch.cat([(x[i:i + block] @ x.T >= T).sum(1) for i in range(0, n, block)])

    ms_t = timed(torch_count, 1, 1)
    same = int((torch_count().to(torch.int32) - 1 == deg).sum())     # torch counts the row itself
    ms_b = max(ms_all - ms_ac, 0.0)
    flop = 2.0 * n * n * DIM
    tf_a = flop / (ms_ac * 1e-3) / 1e12
    pairs_b = 0.5 if kind == "dense" else 0.0
    tf_b = ("%6.1f" % (pairs_b * flop / (ms_b * 1e-3) / 1e12)) if pairs_b and ms_b > 0 else "   n/a"
    lib.vnf_destroy(h)
    return ("%7d | %-6s | %9.2f | %9.2f | %9.2f | %7.1f | %6.1f %% | %s | %8d | %10.1f | %9.2f | %d of %d"
            % (n, kind, ms_all, ms_ac, ms_b, tf_a, 100.0 * tf_a / PEAK_TF, tf_b, clusters, float(deg.float().mean()), ms_t, same, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000,300000")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help="kind:N -- what a child process measures")
    args = ap.parse_args()
    if args.one:
        kind, n = args.one.split(":")
        print(one(kind, int(n), args.steps, args.warmup), flush=True)
        return
    lines = ["# vnf_gallery_cluster, dim %d fp32, threshold %.1f, min_samples 2, default chunk_rows: ms per call over %d calls after %d "
             "warm-up (device events)" % (DIM, T, args.steps, args.warmup),
             "# A + C: the call at threshold 2 (every pair scored, no neighbours, stage B's waves leave at once); B: the call less that",
             "# TF/s: 2 N^2 512 FLOP per scoring stage over its time; peak %.0f; vnf_gallery_search reaches 56-60 at F >= 64" % PEAK_TF,
             "# torch: (x[b] @ x.T >= t).sum(1) over blocks of 2048 rows, the count alone, comparison only",
             "#     N | kind   |  total ms |  A + C ms |      B ms | A TF/s | of peak | B TF/s | clusters | mean degree |  torch ms | same degrees"]
    for n in [int(v) for v in args.ns.split(",")]:
        for kind in ("sparse", "dense"):
            r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", "%s:%d" % (kind, n),
                                "--steps", str(args.steps), "--warmup", str(args.warmup)], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("%s N=%d ended with status %d; nothing more is started\n%s" % (kind, n, r.returncode, r.stdout + r.stderr))
            lines.append(r.stdout.rstrip().splitlines()[-1])
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
