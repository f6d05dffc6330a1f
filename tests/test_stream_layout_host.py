"""CPU: video.ExchangeLayout on its own -- what a rank's block of the stream's exchange holds and how the gathered blocks
are taken apart again.  The gather is emulated by stacking the ranks' blocks; every comparison is exact."""
import itertools
import types

import numpy as np
import pytest
import torch

from vn_celeb_face_recognition_amd.video import ExchangeLayout

CPU = torch.device("cpu")


def _payload(lay, rank, n):
    """rank's batch of n faces on 3 frames, every value distinct per (rank, face, column) -> (payload, expected rows)"""
    per_frame = [n // 3, n - n // 3 - n // 6, n // 6]                       # faces per frame, some frames without any
    assert sum(per_frame) == n
    face, col = np.arange(n, dtype=np.float32)[:, None], np.arange(lay.WIDTH, dtype=np.float32)[None, :]
    want = rank * 4096.0 + face * 32.0 + col / 1024.0                        # exact in fp32
    want[:, 516] = np.repeat(np.arange(3), per_frame)                       # the frame slot follows from the counts
    if lay.k:
        want[:, 517:517 + lay.k] = (rank * 1000 + face * 20 + np.arange(lay.k)[None, :])   # class indices: integers
    t = types.SimpleNamespace(emo_idx=torch.from_numpy(want[:, 517:517 + lay.k]).to(torch.int32),
                              emo_prob=torch.from_numpy(want[:, 517 + lay.k:]))
    got = lay.payload(per_frame, want[:, 512:516].copy(), torch.from_numpy(want[:, :512].copy()), t if lay.k else None, CPU)
    return got, want


@pytest.mark.parametrize("world,cap,k", list(itertools.product((1, 2, 3), (2, 4), (0, 6))))
def test_blocks_gathered_and_split_return_every_ranks_rows(world, cap, k):
    lay = ExchangeLayout(world, cap, k)
    assert lay.WIDTH == 517 + 2 * k
    sizes = (0, 1, cap, cap + 1, 2 * cap + 3)
    for ns in itertools.product(sizes, repeat=world):                       # all-zero included
        pay, want = zip(*(_payload(lay, r, n) for r, n in enumerate(ns)))
        for p, w in zip(pay, want):
            assert (p is None) == (w.shape[0] == 0)
            assert p is None or (p.dtype == torch.float32 and np.array_equal(p.numpy(), w))
        blocks, spills = zip(*(lay.cut(p, CPU) for p in pay))
        if world == 1:
            assert spills[0] is None and (blocks[0] is pay[0] if ns[0] else tuple(blocks[0].shape) == (0, lay.WIDTH))
            counts, rows = [ns[0]], blocks[0]
        else:
            assert all(tuple(b.shape) == (cap + 1, lay.WIDTH) and b.dtype == torch.float32 for b in blocks)
            assert all((s is None) == (n <= cap) and (s is None or s.shape[0] == n - cap) for s, n in zip(spills, ns))
            g = torch.cat(blocks).view(world, cap + 1, lay.WIDTH)            # what all_gather_into_tensor returns
            counts, rows = [int(round(float(c))) for c in g[:, 0, 0].tolist()], g[:, 1:, :].reshape(world * cap, lay.WIDTH)
            assert bool((g[:, 0, 1:] == 0).all())                              # the header row holds the count only
        assert counts == list(ns)
        m = max(0, max(ns) - cap) if world > 1 else 0                        # rows per rank of the follow-up gather
        more = None
        if m:
            more = np.zeros((world, m, lay.WIDTH), np.float32)
            for r, s in enumerate(spills):                                     # a rank's spill, zero rows behind it
                if s is not None:
                    more[r, :s.shape[0]] = s.numpy()
            more = more.reshape(world * m, lay.WIDTH)
        assert more is None or more.shape == (world * m, lay.WIDTH)
        rows = rows.numpy()
        for lo, hi in ((0, lay.WIDTH), (0, 512), (512, lay.WIDTH), (516, 517)):    # any column array splits the same way
            parts = lay.split(counts, rows[:, lo:hi], None if more is None else more[:, lo:hi])
            assert len(parts) == world and all(np.array_equal(p, w[:, lo:hi]) for p, w in zip(parts, want))
        for tail, w in zip(lay.split(counts, rows[:, 512:], None if more is None else more[:, 512:]), want):
            sel = np.arange(w.shape[0])[::2]
            kw = lay.emotions(tail, sel)
            if not k:
                assert kw == {}
                continue
            idx, prob = kw.pop("emotions")
            assert kw == {} and idx.dtype == np.int64 and prob.dtype == np.float32
            assert np.array_equal(idx, w[sel, 517:517 + k].astype(np.int64)) and np.array_equal(prob, w[sel, 517 + k:])


def test_payload_refuses_emotions_of_another_width():
    lay = ExchangeLayout(2, 4, 6)
    t = types.SimpleNamespace(emo_idx=torch.zeros((2, 5), dtype=torch.int32), emo_prob=torch.zeros((2, 5)))
    with pytest.raises(ValueError, match="emotions of shape"):
        lay.payload([2], np.zeros((2, 4), np.float32), torch.zeros((2, 512)), t, CPU)
