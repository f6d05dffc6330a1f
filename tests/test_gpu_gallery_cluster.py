"""GPU: vnf_gallery_cluster (csrc/gallery_cluster.hip) and GalleryModel.cluster against the float64 oracle
tests/gallery_cluster_oracle.py, on the rows of tests/gallery_cluster_data.py.

Cluster ids, degrees and the number of clusters are compared EXACTLY, which only means something when no pair sits within
rounding of the threshold and no border within rounding of a tie: every such comparison first asserts on the CPU that both
oracle margins exceed 4 * gallery_oracle.tol(dim) (2.46e-4 at dim 512).  Nearest neighbours are held to tol(dim) and to the
tolerant rank rule of gallery_oracle.check_ranks.  Bitwise claims compare int32 views.  Every raw call runs with guard
bytes around its five outputs and its workspace."""
import ctypes

import numpy as np
import pytest
import torch

import gallery_cluster_data as data
import gallery_cluster_oracle as gco
import gallery_oracle as go
from test_gpu_gallery import DEV, Guarded, RawGallery, _rows
from vn_celeb_face_recognition_amd import _lib
from vn_celeb_face_recognition_amd.gallery import GalleryModel

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -1, -4
T = data.T
TOL = go.tol(512)


def cluster(rg, t, min_samples, chunk_rows=0):
    """The C ABI with guards -> (cluster, degree, nn_idx, nn_score, n_clusters (1,)) as numpy."""
    g = rg.size
    nbytes = rg.lib.vnf_gallery_cluster_workspace_bytes(g, chunk_rows)
    assert nbytes >= 16
    outs = [Guarded((g,), torch.int32), Guarded((g,), torch.int32), Guarded((g,), torch.int32), Guarded((g,), torch.float32),
            Guarded((1,), torch.int32)]
    ws = Guarded((nbytes,), torch.uint8)
    _lib.check(rg.lib.vnf_gallery_cluster(rg.h, t, min_samples, *[ctypes.c_void_p(o.t.data_ptr()) for o in outs], chunk_rows,
                                          ctypes.c_void_p(ws.t.data_ptr()), nbytes, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs) and ws.intact(), "guard bytes overwritten"
    return tuple(o.t.cpu().numpy() for o in outs)


def _same(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def check(got, o, s64, tol):
    """Exact cluster / degree / n_clusters, tolerant nearest neighbour.  The oracle's margins were asserted by the caller."""
    cl, deg, nn_idx, nn_score, n = got
    assert np.array_equal(deg, o.degree), np.flatnonzero(deg != o.degree)[:10]
    assert int(n[0]) == o.n_clusters
    assert np.array_equal(cl, o.cluster), np.flatnonzero(cl != o.cluster)[:10]
    return gco.check_nearest(nn_idx, nn_score, s64, tol)


def _gallery(rows):
    return RawGallery(rows.shape[1]).add(rows, np.arange(rows.shape[0]) % 7)


@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 33, "small", "large"])
def test_shapes_meet_the_oracle(N):
    name = N if isinstance(N, str) else "small"
    x, s64 = data.case(name)
    n = x.shape[0] if isinstance(N, str) else N
    rg = _gallery(x[:n])
    worst = 0.0
    for ms in ((1, 3, 4) if isinstance(N, str) else (1, 2)):
        o = data.oracle(name, ms, None if isinstance(N, str) else n)          # asserts both margins > 4 tol on the CPU
        worst = max(worst, check(cluster(rg, T, ms), o, s64[:n, :n], TOL))
        print("N=%s min_samples=%d: %d clusters, %d borders, %d noise rows; margins %.3g / %.3g"
              % (N, ms, o.n_clusters, o.border.sum(), (o.cluster < 0).sum(), o.margin_t, o.margin_border))
    print("N=%s: max |nn_score - float64 oracle| = %.3g (tol %.3g)" % (N, worst, TOL))
    rg.close()


def _gap_threshold(s, lo, hi):
    """The middle of the widest gap between off-diagonal scores in [lo, hi]."""
    v = np.unique(s[~np.eye(s.shape[0], dtype=bool)])
    v = v[(v >= lo) & (v <= hi)]
    k = int(np.argmax(np.diff(v)))
    return float(np.float32((v[k] + v[k + 1]) / 2))


def test_dim_32_has_no_hard_coded_stride():
    x = _rows(50, 32, 41)
    s64 = go.scores(x, x)
    t = _gap_threshold(s64, 0.25, 0.45)
    rg = _gallery(x)
    for ms in (1, 3):
        o = gco.cluster_scores(s64, t, ms)
        assert o.margin_t > 4 * go.tol(32) and o.margin_border > 4 * go.tol(32), (o.margin_t, o.margin_border)
        assert o.degree.max() >= 2 and o.n_clusters >= 2 and (ms == 1 or o.border.sum() >= 2)
        for cr in (0, 16):
            check(cluster(rg, t, ms, chunk_rows=cr), o, s64, go.tol(32))
    rg.close()


def test_chunkings_agree_bitwise():
    x, s64 = data.case("large")
    rg = _gallery(x)
    for ms in (3, 4):
        base = cluster(rg, T, ms)
        check(base, data.oracle("large", ms), s64, TOL)
        for cr in (16, 18, 48, 96, 1000):       # 18: chunks that do not begin on a multiple of 4
            assert _same(base, cluster(rg, T, ms, chunk_rows=cr)), (ms, cr)
    rg.close()


def test_repeated_runs_agree_bitwise():
    """The order in which the links are met differs from run to run; the result must not."""
    x, s64 = data.case("large")
    rg = _gallery(x)
    base = cluster(rg, T, 3)
    check(base, data.oracle("large", 3), s64, TOL)
    for run in range(4):
        assert _same(base, cluster(rg, T, 3)), run
    rg.close()


def test_a_chain_crosses_every_boundary():
    """400 rows, each a neighbour of the next only, scattered among 600 noise rows: one cluster whose links span every
    chunk and workgroup boundary, with both ends as borders."""
    rng = np.random.default_rng(51)
    chain = data.chain_rows(400, rng)
    noise = rng.standard_normal((600, 512))
    where = rng.permutation(1000)[:400]              # where[k]: the row of chain element k
    x = np.zeros((1000, 512))
    x[where] = chain
    x[np.setdiff1d(np.arange(1000), where)] = noise
    x = x.astype(np.float32)
    s64 = go.scores(x, x)
    assert np.abs(s64 - T)[~np.eye(1000, dtype=bool)].min() > 4 * TOL
    want_deg = np.zeros(1000, np.int64)
    want_deg[where] = 2
    want_deg[where[[0, -1]]] = 1
    want = np.full(1000, -1, np.int64)
    want[where] = 0
    rg = _gallery(x)
    cl, deg, nn_idx, nn_score, n = cluster(rg, T, 3, chunk_rows=32)
    assert np.array_equal(deg, want_deg) and int(n[0]) == 1 and np.array_equal(cl, want)
    assert nn_idx[where[0]] == where[1] and nn_idx[where[-1]] == where[-2]       # the ends: borders of the one cluster
    o = gco.cluster_scores(s64, T, 3)
    assert o.border.sum() == 2 and o.border[where[[0, -1]]].all() and np.array_equal(o.cluster, want)
    cl4, _, _, _, n4 = cluster(rg, T, 4, chunk_rows=32)                           # nobody has three neighbours
    assert int(n4[0]) == 0 and (cl4 == -1).all()
    rg.close()


def test_scores_are_symmetric():
    """s(i,j) and s(j,i) have the same bits: seen where two rows are each other's nearest neighbour, and, with the
    threshold set to exactly such a score, in the degrees of both rows (a pair that is adjacent from one side only would
    miss one of them).  The 20 pairs used are those whose float64 score is farther than 4 tol from every other score in
    the two rows concerned, so that the oracle's count is beyond doubt but for the pair itself."""
    x, s64 = data.case("large")
    n = x.shape[0]
    rg = _gallery(x)
    _, _, nn_idx, nn_score, _ = cluster(rg, T, 3)
    pairs = [(i, int(nn_idx[i])) for i in range(n) if nn_idx[i] > i and nn_idx[nn_idx[i]] == i]
    assert len(pairs) >= 50
    bits = nn_score.view(np.int32)
    assert all(bits[i] == bits[j] for i, j in pairs)
    used = 0
    for i, j in pairs:
        others = np.ones(n, bool)
        others[[i, j]] = False
        if min(np.abs(s64[i, others] - s64[i, j]).min(), np.abs(s64[j, others] - s64[i, j]).min()) <= 4 * TOL:
            continue
        assert abs(float(nn_score[i]) - s64[i, j]) <= TOL
        _, deg, _, _, _ = cluster(rg, float(nn_score[i]), 3)                  # the threshold is this pair's score, bit for bit
        for a in (i, j):
            assert deg[a] == (s64[a, others] >= s64[i, j]).sum() + 1, (i, j, a)
        used += 1
        if used == 20:
            break
    assert used == 20
    rg.close()


def test_ties_and_duplicates():
    x = _rows(1000, 512, 61)
    v, w = _rows(2, 512, 62)
    x[[3, 7, 40, 900]] = v
    x[[5, 50, 60, 70]] = w
    s64 = go.scores(x, x)
    assert np.abs(s64 - T)[~np.eye(1000, dtype=bool)].min() > 4 * TOL
    rg = _gallery(x)
    for cr in (0, 16):
        cl, deg, nn_idx, nn_score, n = cluster(rg, T, 4, chunk_rows=cr)
        assert int(n[0]) == 2 and (cl[[3, 7, 40, 900]] == 0).all() and (cl[[5, 50, 60, 70]] == 1).all() and (cl >= 0).sum() == 8
        assert deg[[3, 7, 40, 900, 5, 50, 60, 70]].tolist() == [3] * 8 and deg.sum() == 24
        assert nn_idx[[3, 7, 40, 900]].tolist() == [7, 3, 3, 3] and nn_idx[[5, 50, 60, 70]].tolist() == [50, 5, 5, 5]
        assert len(set(nn_score[[3, 7, 40, 900]].view(np.int32).tolist())) == 1 and abs(nn_score[3] - 1.0) <= TOL
    rg.close()


def _tied_border(first_a):
    """A border with the same score, bit for bit, to a core of each of two clusters.  a lives in the first 256 dimensions, b
    is a moved to the last 256, x = (v, v): the products of <x, a> and <x, b> are the same numbers, 256 places apart --
    a whole number of the kernel's groups of 16 k -- and the rest are zeros.  Each core has three neighbours of its own
    (cosine 0.6 to it, 0.36 to each other and to x), so that it is core at min_samples 4 and they and x are not."""
    rng = np.random.default_rng(71)
    unit = lambda u: u / np.linalg.norm(u)
    half = unit(rng.standard_normal(256))
    z = np.zeros(256)
    a, b = np.concatenate([half, z]), np.concatenate([z, half])
    v = half + 0.6 * unit(rng.standard_normal(256))
    rows = {"a": a, "b": b, "x": np.concatenate([v, v])}
    for i in range(3):
        rows["a%d" % i] = np.concatenate([half + 1.33 * unit(rng.standard_normal(256)), z])
        rows["b%d" % i] = np.concatenate([z, half + 1.33 * unit(rng.standard_normal(256))])
    noise = rng.standard_normal((40, 512))
    order = ["a", "b"] if first_a else ["b", "a"]
    # rows 0..19 noise, then the first core, noise, the second core, noise, x and the cores' own neighbours
    x = np.concatenate([noise[:20], rows[order[0]][None], noise[20:30], rows[order[1]][None], noise[30:], rows["x"][None],
                        np.stack([rows["a%d" % i] for i in range(3)] + [rows["b%d" % i] for i in range(3)])])
    return x.astype(np.float32), 20, 31, 42


def test_a_tied_border_goes_to_the_smaller_index():
    for first_a in (True, False):      # were the two scores not tied, x would follow the same vector both times
        x, c0, c1, xi = _tied_border(first_a)
        s64 = go.scores(x, x)
        o = gco.cluster_scores(s64, T, 4)
        assert o.margin_t > 4 * TOL and abs(s64[xi, c0] - s64[xi, c1]) < 1e-12
        assert o.core[[c0, c1]].all() and o.core.sum() == 2 and o.n_clusters == 2 and o.degree[xi] == 2 and o.border.sum() == 7
        rg = _gallery(x)
        for cr in (0, 16):
            cl, deg, _, _, n = cluster(rg, T, 4, chunk_rows=cr)
            assert np.array_equal(deg, o.degree) and int(n[0]) == 2
            assert (cl[c0], cl[c1]) == (0, 1) and cl[xi] == 0, (first_a, cr)
            others = np.arange(x.shape[0]) != xi
            assert np.array_equal(cl[others], o.cluster[others])
        rg.close()


def test_a_nan_row_leaves_the_other_rows_alone():
    x, s64 = data.case("small")
    n, at = x.shape[0], 50
    clean = _gallery(x)
    dirty = _gallery(x[:at])
    bad = torch.from_numpy(clean.rows(at, 1)).to(DEV)
    bad[0, 100] = float("nan")
    lab = torch.zeros((1,), dtype=torch.int32, device=DEV)
    _lib.check(dirty.lib.vnf_gallery_add_unit(dirty.h, ctypes.c_void_p(bad.data_ptr()), ctypes.c_void_p(lab.data_ptr()), 1,
                                              _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    dirty.add(x[at:], np.zeros(n - at))
    assert dirty.size == n + 1
    keep = np.arange(n + 1) != at
    for ms in (1, 2, 3):
        for cr in (0, 16):
            a = cluster(clean, T, ms, chunk_rows=cr)
            cl, deg, nn_idx, nn_score, nc = cluster(dirty, T, ms, chunk_rows=cr)
            assert deg[at] == 0 and nn_idx[at] == 0 and np.isnan(nn_score[at])       # NaN scores tie: the first other row
            want_cl = a[0].copy()
            if ms == 1:                                                              # a cluster of its own, numbered by its row
                assert (cl == cl[at]).sum() == 1 and int(nc[0]) == int(a[4][0]) + 1
                want_cl[want_cl >= cl[at]] += 1
            else:
                assert cl[at] == -1 and int(nc[0]) == int(a[4][0])
            assert np.array_equal(cl[keep], want_cl) and np.array_equal(deg[keep], a[1])
            assert np.array_equal(nn_idx[keep], a[2] + (a[2] >= at)) and np.array_equal(nn_score[keep].view(np.int32), a[3].view(np.int32))
    clean.close(); dirty.close()


def test_through_the_model():
    x, s64 = data.case("small")
    m = GalleryModel(512, max_batch=37).to(DEV).add(x, np.arange(x.shape[0]))
    for cr in (0, 19):
        m.chunk_rows = cr
        cl, deg, nn_idx, nn_score, n = m.cluster(T, 3)
        assert all(t.is_cuda and t.shape == (x.shape[0],) for t in (cl, deg, nn_idx, nn_score)) and isinstance(n, int)
        assert cl.dtype == deg.dtype == nn_idx.dtype == torch.int32 and nn_score.dtype == torch.float32
        check((cl.cpu().numpy(), deg.cpu().numpy(), nn_idx.cpu().numpy(), nn_score.cpu().numpy(), [n]), data.oracle("small", 3), s64, TOL)
    assert m.cluster(T)[4] == data.oracle("small", 2).n_clusters                   # min_samples defaults to 2
    with pytest.raises(ValueError, match="empty"):
        GalleryModel(512).to(DEV).cluster(T)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            m.cluster(bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="min_samples"):
            m.cluster(T, bad)


def test_a_centroid_gallery_shows_a_person_enrolled_twice():
    rng = np.random.default_rng(81)
    unit = lambda u: u / np.linalg.norm(u, axis=-1, keepdims=True)
    centres = unit(rng.standard_normal((5, 512)))
    person = np.array([0, 1, 2, 3, 4, 4])                       # labels 4 and 5 are one person
    labels = np.repeat(np.arange(6), 6)
    rows = unit(centres[person[labels]] + 0.7 * unit(rng.standard_normal((36, 512)))).astype(np.float32)
    sums, _ = go.class_sums(rows, labels, np.arange(6))
    s64 = go.scores(sums, sums)
    o = gco.cluster_scores(s64, T, 2)
    assert o.margin_t > 4 * TOL and o.cluster.tolist() == [-1, -1, -1, -1, 0, 0]
    m = GalleryModel(512, mode="centroid").to(DEV).add(rows, labels)
    assert m.size == 6
    cl, deg, nn_idx, _, n = m.cluster(T, 2)
    assert cl.tolist() == [-1, -1, -1, -1, 0, 0] and n == 1 and deg.tolist() == [0, 0, 0, 0, 1, 1] and nn_idx[4:].tolist() == [5, 4]


def test_error_codes():
    x, _ = data.case("small")
    rg = _gallery(x[:33])
    lib = rg.lib
    out = [torch.empty((33,), dtype=torch.int32, device=DEV) for _ in range(4)]
    nc = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    need = lib.vnf_gallery_cluster_workspace_bytes(33, 16)
    assert need == 800 + 7 * 36 * 4                    # three chunks of 16 rows, a key per row (792 -> 800); seven arrays of 36 entries
    ws = torch.empty((need + 16,), dtype=torch.uint8, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(h=rg.h, t=T, ms=2, o0=P(out[0]), o1=P(out[1]), o2=P(out[2]), o3=P(out[3]), np_=P(nc), wp=P(ws), nbytes=need, cr=16):
        return lib.vnf_gallery_cluster(h, t, ms, o0, o1, o2, o3, np_, cr, wp, nbytes, None)

    assert call() == 0
    for kw in ("o0", "o1", "o2", "o3", "np_", "wp"):
        assert call(**{kw: None}) == INVALID, kw
    assert call(wp=P(ws, 4)) == INVALID and call(wp=P(ws, 8)) == INVALID      # workspace not 16-byte aligned
    assert call(nbytes=need - 4) == CAPACITY
    assert call(t=float("nan")) == INVALID
    assert call(ms=0) == INVALID and call(ms=-3) == INVALID
    assert call(cr=-1) == INVALID
    assert call(h=None) == INVALID
    assert lib.vnf_gallery_cluster_workspace_bytes(-1, 0) == INVALID
    assert lib.vnf_gallery_cluster_workspace_bytes(33, -1) == INVALID
    assert lib.vnf_gallery_cluster_workspace_bytes(0, 0) == 16
    torch.cuda.synchronize()
    assert int(nc.item()) == data.oracle("small", 2, 33).n_clusters
    empty = RawGallery(512)                            # G == 0: a no-op that writes n_clusters = 0 and looks at no other pointer
    assert lib.vnf_gallery_cluster(empty.h, T, 2, None, None, None, None, P(nc), 0, None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(nc.item()) == 0
    empty.close(); rg.close()
