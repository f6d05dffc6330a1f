"""GPU: csrc/gallery.hip and GalleryModel against the float64 oracle tests/gallery_oracle.py.

Scores are held to tol = (dim + 4) 2^-23 (6.2e-5 at dim 512, derived in gallery_oracle.tol) and ranks to the tolerant
comparison of gallery_oracle.check_ranks, so no case is excluded.  Where identical indices are asserted the float64 margin
between best and second best is asserted on the CPU first, for every query.  Every raw search runs with guard bytes
around its three outputs and its workspace."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gallery_oracle as go
from vn_celeb_face_recognition_amd import _lib
from vn_celeb_face_recognition_amd.gallery import GalleryModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256


def _rows(n, dim, seed):
    """Random directions with norms between 0.1 and 30."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim))
    x *= (rng.uniform(0.1, 30.0, (n, 1)) / np.linalg.norm(x, axis=1, keepdims=True))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(G, dim=512):
    g = _rows(G, dim, 100 + G)
    q = _rows(37, dim, 7)
    labels = (np.arange(G) * 7 + 3) % 1013
    g.setflags(write=False); q.setflags(write=False); labels.setflags(write=False)
    return g, labels, q, go.scores(q, g)


class Guarded:
    """A device tensor with GUARD pattern bytes on both sides."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.n:] == 0xA5).all())


class RawGallery:
    """The C ABI directly: vnf_gallery_create / _add / _search / _rows."""

    def __init__(self, dim, capacity=0):
        self.lib = _lib.load()
        torch.cuda.set_device(0)
        _lib.check(self.lib.vnf_init(0))
        self.dim = dim
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.vnf_gallery_create(dim, capacity, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.lib.vnf_destroy(self.h)
            self.h = None

    __del__ = close

    def add(self, rows, labels):
        r = torch.from_numpy(np.array(rows, np.float32)).to(DEV)
        l = torch.from_numpy(np.ascontiguousarray(labels).astype(np.int32)).to(DEV)
        _lib.check(self.lib.vnf_gallery_add(self.h, ctypes.c_void_p(r.data_ptr()), ctypes.c_void_p(l.data_ptr()), r.shape[0],
                                            _lib.current_stream_ptr()))
        torch.cuda.synchronize()
        return self

    @property
    def size(self):
        n = ctypes.c_int64(-1)
        _lib.check(self.lib.vnf_gallery_size(self.h, ctypes.byref(n)))
        return n.value

    def rows(self, first, n):
        out = torch.empty((n, self.dim), dtype=torch.float32, device=DEV)
        _lib.check(self.lib.vnf_gallery_rows(self.h, ctypes.c_void_p(out.data_ptr()), first, n, _lib.current_stream_ptr()))
        return out.cpu().numpy()

    def search(self, q, k, chunk_rows=0):
        qd = torch.from_numpy(np.array(q, np.float32)).to(DEV)
        f = qd.shape[0]
        nbytes = self.lib.vnf_gallery_search_workspace_bytes(f, k, self.size, chunk_rows)
        assert nbytes >= 8
        outs = [Guarded((f, k), torch.int32), Guarded((f, k), torch.int32), Guarded((f, k), torch.float32)]
        ws = Guarded((nbytes,), torch.uint8)
        _lib.check(self.lib.vnf_gallery_search(self.h, ctypes.c_void_p(qd.data_ptr()), f, k, *[ctypes.c_void_p(o.t.data_ptr()) for o in outs],
                                               chunk_rows, ctypes.c_void_p(ws.t.data_ptr()), nbytes, _lib.current_stream_ptr()))
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs) and ws.intact(), "guard bytes overwritten"
        return tuple(o.t.cpu().numpy() for o in outs)


@pytest.mark.parametrize("G", [1, 15, 16, 17, 1000])
def test_shapes_meet_the_tolerant_rank_comparison(G):
    g, labels, q, s64 = _case(G)
    rg = RawGallery(512).add(g, labels)
    assert rg.size == G
    worst = 0.0
    for F in (0, 1, 15, 17, 37):
        for k in (1, 6, 16):
            idx, lab, sc = rg.search(q[:F], k)
            assert idx.shape == lab.shape == sc.shape == (F, k)
            worst = max(worst, go.check_ranks(idx, sc, s64[:F], k, go.tol(512)))
            valid = idx >= 0
            assert np.array_equal(lab[valid], labels[idx[valid]]) and (lab[~valid] == -1).all()
    print("G=%d: max |score - float64 oracle| = %.3g (tol %.3g)" % (G, worst, go.tol(512)))
    rg.close()


def test_dim_32_has_no_hard_coded_stride():
    g, labels, q, s64 = _case(50, 32)
    rg = RawGallery(32).add(g, labels)
    for k in (6, 16):
        idx, lab, sc = rg.search(q[:17], k, chunk_rows=16)
        go.check_ranks(idx, sc, s64[:17], k, go.tol(32))
        assert np.array_equal(lab, labels[idx])
    rg.close()


def test_create_refuses_bad_dims_and_search_bad_k():
    lib = _lib.load()
    for dim in (0, 8, 24, 520, 528, 1024):
        h = ctypes.c_void_p()
        assert lib.vnf_gallery_create(dim, 16, ctypes.byref(h)) == -1 and not h     # VNF_E_INVALID
    g, labels, q, _ = _case(16)
    rg = RawGallery(512).add(g, labels)
    qd = torch.from_numpy(q[:1].copy()).to(DEV)
    out = torch.empty((64,), dtype=torch.int32, device=DEV)
    for k in (0, 17):
        rc = lib.vnf_gallery_search(rg.h, ctypes.c_void_p(qd.data_ptr()), 1, k, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                    ctypes.c_void_p(out.data_ptr()), 0, ctypes.c_void_p(out.data_ptr()), 256, None)
        assert rc == -1
    rc = lib.vnf_gallery_search(rg.h, ctypes.c_void_p(qd.data_ptr()), 1, 16, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                ctypes.c_void_p(out.data_ptr()), 0, ctypes.c_void_p(out.data_ptr()), 8, None)
    assert rc != 0                                                                   # workspace too small
    rg.close()


def test_planted_matches_top1_equals_oracle():
    g, labels, _, _ = _case(1000)
    rng = np.random.default_rng(11)
    pick = rng.permutation(1000)[:37]
    unit = g[pick] / np.linalg.norm(g[pick], axis=1, keepdims=True)
    q = (unit * rng.uniform(0.1, 30.0, (37, 1)) + 0.002 * rng.standard_normal((37, 512))).astype(np.float32)
    s64 = go.scores(q, g)
    oi, ol, osc = go.topk(s64, labels, 2)
    assert (oi[:, 0] == pick).all()
    assert (osc[:, 0] - osc[:, 1] > 4 * go.tol(512)).all()          # every query, none left out
    rg = RawGallery(512).add(g, labels)
    idx, lab, sc = rg.search(q, 1)
    assert np.array_equal(idx[:, 0], oi[:, 0]) and np.array_equal(lab[:, 0], ol[:, 0])
    assert np.abs(sc[:, 0] - osc[:, 0]).max() <= go.tol(512)
    rg.close()


def test_chunkings_agree_bitwise():
    g, labels, q, s64 = _case(1000)
    rg = RawGallery(512).add(g, labels)
    for k in (1, 16):
        base = rg.search(q, k, chunk_rows=0)
        go.check_ranks(base[0], base[2], s64, k, go.tol(512))
        for cr in (16, 48, 1000):
            got = rg.search(q, k, chunk_rows=cr)
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(base, got)), cr
    rg.close()
    g97, l97 = g[:97], labels[:97]
    rg = RawGallery(512).add(g97, l97)
    a, b = rg.search(q, 6, chunk_rows=96), rg.search(q, 6, chunk_rows=0)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    go.check_ranks(a[0], a[2], s64[:, :97], 6, go.tol(512))
    assert (a[0] == 96).any()                                      # the row alone in the second chunk is found
    rg.close()


def test_rows_alone_equal_rows_in_a_batch_bitwise():
    g, labels, q, _ = _case(1000)
    rg = RawGallery(512).add(g, labels)
    batch = rg.search(q, 6)
    for i in (0, 15, 16, 36):
        alone = rg.search(q[i:i + 1], 6)
        assert all(np.array_equal(a[0].view(np.int32), b[i].view(np.int32)) for a, b in zip(alone, batch)), i
    rg.close()


def test_exact_ties_come_in_row_order():
    g, labels, q, _ = _case(1000)
    g = g.copy()
    v = _rows(1, 512, 5)[0]
    g[3] = g[40] = g[900] = v
    rg = RawGallery(512).add(g, labels)
    for cr in (0, 16):
        idx, lab, sc = rg.search(np.stack([v, np.zeros(512, np.float32)]), 6, chunk_rows=cr)
        assert idx[0, :3].tolist() == [3, 40, 900]
        assert len(set(sc[0, :3].view(np.int32).tolist())) == 1 and abs(sc[0, 0] - 1.0) <= go.tol(512)
        assert sc[0, 3] < sc[0, 2]
        assert idx[1].tolist() == [0, 1, 2, 3, 4, 5] and (sc[1] == 0).all()      # a zero query
    rg.close()


def test_a_nan_query_leaves_the_other_rows_alone():
    g, labels, q, _ = _case(1000)
    rg = RawGallery(512).add(g, labels)
    clean = q[:5].copy()
    dirty = clean.copy()
    dirty[2, 100] = np.nan
    a, b = rg.search(clean, 6), rg.search(dirty, 6)
    for i in (0, 1, 3, 4):
        assert all(np.array_equal(x[i].view(np.int32), y[i].view(np.int32)) for x, y in zip(a, b))
    assert b[0][2].tolist() == [0, 1, 2, 3, 4, 5] and np.isnan(b[2][2]).all()   # NaN scores tie: rows in order
    rg.close()


def test_add_grows_and_keeps_rows_and_labels():
    g, labels, q, s64 = _case(1000)
    rg = RawGallery(512, capacity=4)
    rg.add(g[:3], labels[:3])
    first = rg.rows(0, 3)
    assert np.abs(np.linalg.norm(first.astype(np.float64), axis=1) - 1).max() < 1e-6
    rg.add(g[3:20], labels[3:20])                 # past the capacity
    rg.add(g[20:1000], labels[20:1000])           # and again
    assert rg.size == 1000
    assert np.array_equal(rg.rows(0, 3).view(np.int32), first.view(np.int32))
    whole = RawGallery(512, capacity=1000).add(g, labels)
    assert np.array_equal(rg.rows(0, 1000).view(np.int32), whole.rows(0, 1000).view(np.int32))
    # ||x||^2 is 4 chains of 128 squares and two more sums: (128 + 3) 2^-24 relative at worst, its root half of that, the
    # division one more rounding -- under 70 * 2^-24 of each element
    unit = go.normalize(g)
    assert (np.abs(whole.rows(0, 1000).astype(np.float64) - unit) <= 70 * 2.0 ** -24 * np.abs(unit) + 1e-45).all()
    idx, lab, sc = rg.search(q, 16)
    assert np.array_equal(lab, labels[idx])
    go.check_ranks(idx, sc, s64, 16, go.tol(512))
    rg.close(); whole.close()


def _centroid_data():
    rng = np.random.default_rng(21)
    classes = np.array([2, 5, 9, 11, 30])
    labels = np.concatenate([np.full(8, 2), np.full(1, 5), np.full(7, 9), np.full(8, 11), np.full(5, 30)])
    order = rng.permutation(labels.shape[0])
    labels = labels[order]
    rows = _rows(labels.shape[0], 512, 22)
    return rows, labels, classes


def test_centroid_sums_repeat_and_append_equals_one_enrolment(tmp_path):
    rows, labels, classes = _centroid_data()
    a = GalleryModel(512, mode="centroid").to(DEV).add(rows, labels)
    b = GalleryModel(512, mode="centroid").to(DEV).add(torch.from_numpy(rows).to(DEV), labels)
    want, counts = go.class_sums(rows, labels, classes)
    assert np.array_equal(a._classes, classes) and np.array_equal(a._counts, counts) and counts.max() <= 8
    bound = 4.0 * counts[:, None] * 2.0 ** -23
    err = np.abs(a._sums.astype(np.float64) - want)
    print("centroid sums: max error / bound = %.3g" % (err / bound).max())
    assert (err <= bound).all()
    assert np.array_equal(a._sums.view(np.int32), b._sums.view(np.int32)) and np.array_equal(a._emb.view(np.int32), b._emb.view(np.int32))
    assert a.size == 5 and np.array_equal(a._labels, classes)                      # one row per class, ascending
    # save -> load -> append == everything at once
    first = GalleryModel(512, mode="centroid").to(DEV).add(rows[:17], labels[:17])
    p = str(tmp_path / "c.npz")
    first.save(p)
    again = GalleryModel.load(p).to(DEV).add(rows[17:], labels[17:])
    for name in ("_emb", "_sums"):
        assert np.array_equal(getattr(again, name).view(np.int32), getattr(a, name).view(np.int32)), name
    for name in ("_labels", "_classes", "_counts"):
        assert np.array_equal(getattr(again, name), getattr(a, name)), name
    q = torch.tensor(_case(16)[2]).to(DEV)
    ra, rb = a.search(q, 5), again.search(q, 5)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))
    s64 = go.scores(q.cpu().numpy(), a._sums)          # the searchable rows are the normalised fp32 sums
    go.check_ranks(ra[0].cpu().numpy(), ra[2].cpu().numpy(), s64, 5, go.tol(512))
    assert np.array_equal(ra[1].cpu().numpy(), classes[ra[0].cpu().numpy()])


def test_all_mode_save_load_append(tmp_path):
    g, labels, q, s64 = _case(1000)
    m = GalleryModel(512).to(DEV).add(g[:600], labels[:600])
    p = str(tmp_path / "g.npz")
    m.save(p)
    m2 = GalleryModel.load(p).to(DEV).add(g[600:], labels[600:])
    whole = GalleryModel(512).to(DEV).add(g, labels)
    assert m2.size == 1000 and np.array_equal(m2._emb.view(np.int32), whole._emb.view(np.int32))
    qd = torch.tensor(q).to(DEV)
    assert all(torch.equal(x, y) for x, y in zip(m2.search(qd, 6), whole.search(qd, 6)))
    whole.chunk_rows = 48
    assert all(torch.equal(x, y) for x, y in zip(m2.search(qd, 6), whole.search(qd, 6)))
    idx, lab, sc = whole.search(qd, 6)
    go.check_ranks(idx.cpu().numpy(), sc.cpu().numpy(), s64, 6, go.tol(512))
    with pytest.raises(ValueError, match="empty"):
        GalleryModel(512).to(DEV).search(qd)
    with pytest.raises(ValueError):
        whole.search(qd, 17)


def test_classify_contract_and_identify_names():
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.pipeline import identify_names, identify_person
    g, labels, _, _ = _case(1000)
    rng = np.random.default_rng(31)
    pick = rng.permutation(1000)[:9]
    known = (g[pick] + 0.002 * rng.standard_normal((9, 512))).astype(np.float32)
    q = np.concatenate([known, _rows(8, 512, 32)])
    s64 = go.scores(q, g)
    oi, ol, osc = go.topk(s64, labels, 2)
    thr = 0.5
    # labels are compared for the nine planted faces (margin asserted for each); the eight strangers only have to fall
    # below the threshold, whichever near-tied row is their best
    assert (osc[:9, 0] - osc[:9, 1] > 4 * go.tol(512)).all() and (np.abs(osc[:, 0] - thr) > go.tol(512)).all()
    assert (osc[:9, 0] > thr).all() and (osc[9:, 0] < thr).all()
    gal = models.GalleryModel(512).to(DEV).eval().add(g, labels)
    qd = torch.from_numpy(q).to(DEV)
    none, amax, prob = gal.classify(qd, want_logp=False)
    _, amax_m, prob_m = models.MLPModel(512, 10).to(DEV).eval().classify(qd, want_logp=False)
    assert none is None and amax.dtype == amax_m.dtype == torch.int32 and prob.dtype == prob_m.dtype == torch.float32
    assert amax.shape == amax_m.shape == (17,) and prob.shape == prob_m.shape == (17,) and amax.is_cuda and prob.is_cuda
    assert np.array_equal(amax.cpu().numpy()[:9], ol[:9, 0]) and np.abs(prob.cpu().numpy() - osc[:, 0]).max() <= go.tol(512)
    assert gal.num_classes == int(labels.max()) + 1
    df = {"label": list(range(1013)), "name": ["celeb_%d" % i for i in range(1013)]}
    want = identify_names(ol[:, 0], osc[:, 0], gal.num_classes, df, thr)
    assert want[9:] == ["Unknown"] * 8 and all(n == "celeb_%d" % l for n, l in zip(want[:9], ol[:9, 0]))
    assert identify_person(qd, gal, df, thr) == want
    per_class = {str(i): thr for i in range(1013)}
    assert identify_person(qd, gal, df, per_class) == want
    per_class[str(int(ol[0, 0]))] = 1.5                      # this class alone cannot be reached
    assert identify_person(qd, gal, df, per_class) == ["Unknown"] + want[1:]
