"""Shared by tests/test_gpu_gallery_bits.py and tools/make_gallery_bits.py: the exact outputs of the gallery family's C
ABI (csrc/gallery.hip, gallery_mated.hip, gallery_cluster.hip, gallery_tracks.hip over csrc/gallery_core.h), recorded
per case as the SHA-256 of the raw bytes of every output array and its absolute sum in hex (a readable hint: NaN and
infinities are left out of it).  Only the C ABI is used, through the guarded raw callers the family's own GPU tests have,
so the same run can be recorded on one commit and replayed on another.

The shapes cross the seams and are no larger: dim 512 (the EXACT instantiation of every streaming kernel) and dim 32 (the
other one); G = 70 rows, past a wave's 16 rows, a 32-row tile and a 64-row chunk; F = 17 queries, a full wave and one
more; chunk_rows 0 (the library's choice: one chunk of 64 rows and one of 6) and 32 (three chunks).

  rows        vnf_gallery_add then vnf_gallery_rows: the stored unit rows
  search      vnf_gallery_search, k = 1 and k = 16
  mated       vnf_gallery_mated_search, with and without `exclude`
  cluster     vnf_gallery_cluster at threshold 0.5, min_samples 2: all five outputs
  tracks      vnf_gallery_tracks at threshold 0.5, max_gap 1 and 4, min_iou 0 (no boxes) and 0.3
  track_sums  vnf_gallery_track_sums on those outputs

The searched and clustered rows are gallery_cluster_data.make's (every DBSCAN role in 70 rows), the queries and the
tracked rows test_gpu_tracks.scene's (its 70-row scene: frames that straddle a wave and a tile, empty frames).

Known gap, for the next recording (which has to be made on a commit whose arithmetic is to be kept, not on a changed one):
at dim 32 the exclusions chosen here never name a probe's best mate, so mated-d32-exclude-* and mated-d32-all-* hold the
same hashes and the `exclude` path is pinned at dim 512 only.  Excluding each probe's best mate would pin it at both."""
import atexit
import functools
import hashlib
import subprocess

import numpy as np
import torch

import gallery_cluster_data as data
import test_gpu_gallery_cluster as tgc
import test_gpu_mated_search as tms
import test_gpu_tracks as tgt
from test_gpu_gallery import RawGallery

DIMS = (512, 32)
G, F = 70, 17
CHUNKS = (0, 32)
T = 0.5
# 31 blob rows + 3 satellites + 2 bridges + a chain of 12 + 19 noise rows + make()'s 3 duplicates = 70
ROWS = dict(seed=31, blobs=(17, 9, 5), chain=12, noise=19, satellites=3, bridges=2)


@functools.lru_cache(maxsize=None)
def _inputs(dim):
    """-> gallery rows (70,dim), their labels, queries (17,dim), query labels (7: nobody's), exclusions (-1: none)."""
    x = data.make(dim=dim, **ROWS)
    assert x.shape == (G, dim)
    labels = np.arange(G) % 7
    q = tgt.case(dim, tgt.SIZES)[0][:F]
    ql = (np.arange(F) * 3) % 8
    excl = np.array([-1 if f % 4 == 0 or ql[f] == 7 else int(np.flatnonzero(labels == ql[f])[f % 10]) for f in range(F)])
    return x, labels, q, ql, excl


@functools.lru_cache(maxsize=None)
def _gallery(dim):
    x, labels = _inputs(dim)[:2]
    rg = RawGallery(dim).add(x, labels)
    atexit.register(rg.close)                            # shared by the cases of a dim: closed with the process
    return rg


@functools.lru_cache(maxsize=None)
def _tracks(dim, max_gap, min_iou):
    x, f, b, _ = tgt.case(dim, tgt.SIZES)
    assert x.shape == (G, dim)
    rg = RawGallery(dim).add(x, f)
    got = tgt.tracks(rg, f, b if min_iou > 0 else None, T, min_iou, max_gap)
    rg.close()
    got["n_tracks"] = np.array([got["n_tracks"]], np.int32)
    return got


def _rows(dim):
    return {"rows": _gallery(dim).rows(0, G)}


def _search(dim, k, cr):
    return dict(zip(("idx", "label", "score"), _gallery(dim).search(_inputs(dim)[2], k, chunk_rows=cr)))


def _mated(dim, with_excl, cr):
    _, _, q, ql, excl = _inputs(dim)
    return dict(zip(("idx", "label", "score"), tms.mated(_gallery(dim), q, ql, excl if with_excl else None, chunk_rows=cr)))


def _cluster(dim, cr):
    return dict(zip(("cluster", "degree", "nn_idx", "nn_score", "n_clusters"), tgc.cluster(_gallery(dim), T, 2, chunk_rows=cr)))


def _links(dim, max_gap, min_iou):
    got = _tracks(dim, max_gap, min_iou)
    return {k: got[k] for k in ("prev", "next", "link_score", "track", "n_tracks")}


def _sums(dim, max_gap, min_iou):
    got = _tracks(dim, max_gap, min_iou)
    return {k: got[k] for k in ("sums", "counts")}


def _cases():
    out = {}
    for d in DIMS:
        out["rows-d%d" % d] = (_rows, d)
        for cr in CHUNKS:
            for k in (1, 16):
                out["search-d%d-k%d-chunk%d" % (d, k, cr)] = (_search, d, k, cr)
            for e in (True, False):
                out["mated-d%d-%s-chunk%d" % (d, "exclude" if e else "all", cr)] = (_mated, d, e, cr)
            out["cluster-d%d-chunk%d" % (d, cr)] = (_cluster, d, cr)
        for gap in (1, 4):
            for iou in (0.0, 0.3):
                out["tracks-d%d-gap%d-iou%g" % (d, gap, iou)] = (_links, d, gap, iou)
                out["track_sums-d%d-gap%d-iou%g" % (d, gap, iou)] = (_sums, d, gap, iou)
    return out


CASES = _cases()


def run_case(case):
    """-> {output name: {"sha256", "abs_sum", "dtype", "shape"}}"""
    fn, *args = CASES[case]
    rec = {}
    for name, a in fn(*args).items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.int32, np.float32), (case, name, a.dtype)
        v = a.astype(np.float64)
        rec[name] = {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "abs_sum": float(np.abs(v[np.isfinite(v)]).sum()).hex(),
                     "dtype": str(a.dtype), "shape": list(a.shape)}
    return rec


def versions():
    """The toolchain a record was made under / a test runs under: torch and the hipcc that builds the library."""
    from vn_celeb_face_recognition_amd.build import HIPCC
    try:
        hipcc = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.strip()
    except OSError as e:
        hipcc = "unavailable: %s" % e
    return {"torch": torch.__version__, "hipcc": hipcc}
