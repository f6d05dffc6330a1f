#!/usr/bin/env python3
"""What calibration's search costs: vnf_gallery_mated_search (csrc/gallery_mated.hip) beside vnf_gallery_search(k=1) on the
same handle and probes, at dim 512 for (F, G) = (1024, 100 000), (64, 1 000 000) and the self case F = G = 20 000 (the
gallery's own rows as probes, each excluded from its mates).  The search with k = 1 is the yardstick: it streams the same
rows through the same MFMAs and keeps one key per lane where the mated search keeps two and reads the rows' labels.

Per case: microseconds per call of each (device events; the two alternate, `--rounds` rounds of `--steps` calls after a
warm-up of both, the median round is reported with the spread of the rounds), their ratio, and the exact-fp32 MFMA rate
each implies (2 * F * G * 512 FLOP over the time).  The last column checks the two against each other: per probe, the
better of the mate and non-mate columns must be the search's top-1, index and score bits (without an exclusion).
A record (profiles/calibrate_time.txt), not a gate; bench.py does not call this.

    python tools/calibrate_time.py [--cases 1024x100000,64x1000000,self20000] [--steps 10] [--rounds 5] --out profiles/calibrate_time.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DIM = 512
ROWS_PER_LABEL = 100     # more than the 16 the top-k search can return: the non-mate is out of its reach


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3     # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x100000,64x1000000,self20000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    _lib.check(lib.vnf_init(0))
    gen = torch.Generator(device=dev).manual_seed(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    lines = ["# vnf_gallery_mated_search beside vnf_gallery_search(k=1), dim %d fp32, default chunk_rows, %d rows per label: us per call,"
             % (DIM, ROWS_PER_LABEL),
             "# median of %d alternating rounds of %d calls after %d warm-up calls of each (device events); min..max of the rounds in brackets"
             % (args.rounds, args.steps, args.warmup),
             "# TFLOP/s: 2 * F * G * %d over the time, exact-fp32 MFMA; agree: probes whose better column is the search's top-1, bit for bit" % DIM,
             "#     F |       G | case | search k=1 us [min..max] | mated us [min..max] | ratio | search TFLOP/s | mated TFLOP/s | agree"]
    for case in args.cases.split(","):
        self_case = case.startswith("self")
        F, G = (int(case[4:]),) * 2 if self_case else (int(v) for v in case.split("x"))
        h = ctypes.c_void_p()
        _lib.check(lib.vnf_gallery_create(DIM, G, ctypes.byref(h)))
        labels = (torch.randperm(G, generator=gen, device=dev) // ROWS_PER_LABEL).to(torch.int32)
        for g0 in range(0, G, 100000):
            n = min(100000, G - g0)
            rows = torch.randn((n, DIM), generator=gen, device=dev)
            _lib.check(lib.vnf_gallery_add(h, P(rows), P(labels[g0:g0 + n]), n, None))
        if self_case:
            q = torch.empty((G, DIM), dtype=torch.float32, device=dev)
            _lib.check(lib.vnf_gallery_rows(h, P(q), 0, G, None))
            ql, ex = labels.clone(), torch.arange(G, dtype=torch.int32, device=dev)
        else:
            q = torch.randn((F, DIM), generator=gen, device=dev)
            ql, ex = labels[torch.randint(0, G, (F,), generator=gen, device=dev)].contiguous(), None
        torch.cuda.synchronize()
        nb_s = lib.vnf_gallery_search_workspace_bytes(F, 1, G, 0)
        nb_m = lib.vnf_gallery_mated_search_workspace_bytes(F, G, 0)
        ws = torch.empty((max(nb_s, nb_m),), dtype=torch.uint8, device=dev)
        s_out = [torch.empty((F, 1), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
        m_out = [torch.empty((F, 2), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
        stream = _lib.current_stream_ptr()

        def search():
            _lib.check(lib.vnf_gallery_search(h, P(q), F, 1, P(s_out[0]), P(s_out[1]), P(s_out[2]), 0, P(ws), nb_s, stream))

        def mated(exclude=ex):
            _lib.check(lib.vnf_gallery_mated_search(h, P(q), P(ql), None if exclude is None else P(exclude), F, P(m_out[0]), P(m_out[1]),
                                                    P(m_out[2]), 0, P(ws), nb_m, stream))

        # the two against each other, without an exclusion: max(mate, non-mate) under the key order is the top-1
        search()
        mated(None)
        torch.cuda.synchronize()
        mi, ms = m_out[0].long(), m_out[2]
        first = (ms[:, 0] > ms[:, 1]) | ((ms[:, 0] == ms[:, 1]) & (mi[:, 0] < mi[:, 1])) | (mi[:, 1] < 0)
        first &= mi[:, 0] >= 0
        col = (~first).long().unsqueeze(1)
        agree = int(((mi.gather(1, col) == s_out[0].long()) & (ms.gather(1, col).view(torch.int32) == s_out[2].view(torch.int32))).sum())
        for _ in range(args.warmup):
            search()
            mated()
        torch.cuda.synchronize()
        ts, tm = [], []
        for _ in range(args.rounds):
            ts.append(timed(search, args.steps))
            tm.append(timed(mated, args.steps))
        us_s, us_m = statistics.median(ts), statistics.median(tm)
        flop = 2.0 * F * G * DIM
        lines.append("%7d | %7d | %4s | %10.1f [%.1f..%.1f] | %10.1f [%.1f..%.1f] | %5.3f | %14.1f | %13.1f | %d of %d"
                     % (F, G, "self" if self_case else "set", us_s, min(ts), max(ts), us_m, min(tm), max(tm), us_m / us_s,
                        flop / us_s / 1e6, flop / us_m / 1e6, agree, F))
        print(lines[-1], flush=True)
        lib.vnf_destroy(h)
        del q, ws
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
