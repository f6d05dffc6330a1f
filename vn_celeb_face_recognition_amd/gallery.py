"""Gallery identification: enrol embeddings, identify by cosine similarity (csrc/gallery.hip).

The closed-set MLPModel has to be retrained whenever a person is added.  A GalleryModel holds the L2-normalised
embeddings the encoders emit, with a label per row, and names a face by its best cosine against them; a person is
added with .add().  It offers the call everything downstream uses,

    classify(emb, want_logp=False) -> (None, amax (F,) int32, prob (F,) fp32)

with `prob` the top-1 COSINE in [-1, 1] (not a probability), so identify_person, FacePipeline, video.run_stream, the
per-class thresholds, the tracker and the overlay work unchanged; thresholds compare cosines.  Where such a threshold comes
from: mated_search(emb, labels, exclude) gives every probe of known label its best mate and non-mate (csrc/gallery_mated.hip),
and calibration.py / calibrate.py read the threshold for a false-accept rate off those scores.  Where the labels come
from, or whether they are right: cluster(threshold, min_samples) groups the gallery's own rows into identities by DBSCAN
over their cosines (csrc/gallery_cluster.hip); clustering.py / cluster.py turn that into a label file or a report.

mode "all": every enrolled row is searchable.  mode "centroid": one row per enrolled class, the normalised sum of the
class's normalised rows, in ascending label order; the running sums and counts are kept (and saved), so a loaded
centroid gallery can be appended to without the original rows."""
import ctypes

import numpy as np
import torch

from . import _lib

MODES = ("all", "centroid")
MAX_K = 16


def check_rows(embeddings, labels, dim):
    """Host check of an enrolment batch before anything is uploaded: (n,dim) finite rows, n integer labels in [0, 2^31).
    Works on host arrays and on cuda tensors (the verdict is one scalar read back).  Returns the labels as int64 numpy."""
    if isinstance(embeddings, torch.Tensor):
        shape = tuple(embeddings.shape)
        finite = bool(torch.isfinite(embeddings).all()) if embeddings.numel() else True
    else:
        embeddings = np.asarray(embeddings)
        shape = embeddings.shape
        finite = bool(np.isfinite(embeddings).all())
    if len(shape) != 2 or shape[1] != dim:
        raise ValueError("expected (n,%d) embeddings, got %s" % (dim, shape))
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if lab.size == 0:
        lab = lab.astype(np.int64)
    if lab.dtype.kind not in "iu":
        raise ValueError("labels must be integers, got %s" % lab.dtype)
    lab = lab.reshape(-1)
    if lab.shape[0] != shape[0]:
        raise ValueError("%d labels for %d rows" % (lab.shape[0], shape[0]))
    if lab.size and (int(lab.min()) < 0 or int(lab.max()) >= 2 ** 31):
        raise ValueError("labels must lie in [0, 2^31)")
    if not finite:
        raise ValueError("embeddings hold non-finite values")
    return lab.astype(np.int64)


class GalleryModel:
    """GalleryModel(input_dim=512, num_classes=None, mode="all"|"centroid", max_batch=1024)."""

    def __init__(self, input_dim=512, num_classes=None, mode="all", max_batch=1024):
        self.input_dim = int(input_dim)
        if self.input_dim % 16 or not 16 <= self.input_dim <= 512:
            raise ValueError("input_dim must be a multiple of 16 in 16..512, got %d" % self.input_dim)
        if mode not in MODES:
            raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
        self.mode = mode
        self.max_batch = int(max_batch)
        self._num_classes = None if num_classes is None else int(num_classes)
        self.training = False
        self.device = torch.device("cpu")
        self.chunk_rows = 0          # 0: the library's default; tests move the chunk boundary
        self._handle = None
        self._handle_dev = None
        self._uploaded = 0           # rows of the host mirror the handle holds
        # host mirror: what .save() writes and what a handle is rebuilt from
        self._emb = np.zeros((0, self.input_dim), np.float32)   # unit rows, as the device produced them
        self._labels = np.zeros((0,), np.int64)
        self._classes = np.zeros((0,), np.int64)                # centroid mode: the enrolled labels, ascending
        self._sums = np.zeros((0, self.input_dim), np.float32)  #   their running sums of normalised rows
        self._counts = np.zeros((0,), np.int64)

    # -- the model interface the CLIs use ---------------------------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def to(self, device):
        self.device = torch.device(device)
        return self

    @property
    def size(self):
        return int(self._emb.shape[0])

    @property
    def num_classes(self):
        """The "Unknown" index of identify_names: max label + 1, or the constructor's num_classes when that is larger
        (enrolling a label beyond it raises it: people are added without ceremony)."""
        seen = int(self._labels.max()) + 1 if self._labels.size else 0
        return max(seen, self._num_classes or 0)

    def _drop(self):
        if self._handle is not None:
            _lib.load().vnf_destroy(self._handle)
            self._handle = None
        self._uploaded = 0

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def _dev(self):
        if self.device.type != "cuda":
            raise RuntimeError("GalleryModel runs on MI355X only: move it to a cuda device (there is no CPU path)")
        return self.device.index if self.device.index is not None else torch.cuda.current_device()

    def _ensure(self):
        """The device handle, holding every row of the host mirror."""
        dev = self._dev()
        lib = _lib.load()
        if self._handle is None or self._handle_dev != dev:
            self._drop()
            with torch.cuda.device(dev):
                _lib.check(lib.vnf_init(dev))
                h = ctypes.c_void_p()
                _lib.check(lib.vnf_gallery_create(self.input_dim, max(self.size, 1024), ctypes.byref(h)))
            self._handle, self._handle_dev = h, dev
        if self._uploaded < self.size:   # rows the handle has not seen (after load(), or on another device): unit rows
            with torch.cuda.device(dev):   # already, stored as they are
                rows = torch.from_numpy(self._emb[self._uploaded:]).to("cuda:%d" % dev)
                labs = torch.from_numpy(self._labels[self._uploaded:].astype(np.int32)).to("cuda:%d" % dev)
                _lib.check(lib.vnf_gallery_add_unit(self._handle, ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(labs.data_ptr()),
                                                    rows.shape[0], _lib.current_stream_ptr()))
                torch.cuda.current_stream().synchronize()
            self._uploaded = self.size
        return self._handle

    # -- enrolment ------------------------------------------------------------------------------------------------
    def add(self, embeddings, labels):
        """Enrol (n,input_dim) embeddings (host array or cuda tensor, any norm) under n integer labels."""
        lab = check_rows(embeddings, labels, self.input_dim)
        dev = self._dev()
        if lab.size == 0:
            return self
        cuda = torch.device("cuda:%d" % dev)
        rows = embeddings if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.array(embeddings, np.float32))
        rows = rows.to(cuda).float().contiguous()
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.vnf_init(dev))
            if self.mode == "all":
                self._add_rows(rows, lab, cuda)
            else:
                self._add_centroid(rows, lab, cuda)
        return self

    def _add_rows(self, rows, lab, cuda):
        lib = _lib.load()
        h = self._ensure()
        lab32 = torch.from_numpy(lab.astype(np.int32)).to(cuda)
        n0 = self.size
        _lib.check(lib.vnf_gallery_add(h, ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(lab32.data_ptr()), rows.shape[0],
                                       _lib.current_stream_ptr()))
        unit = torch.empty_like(rows)
        _lib.check(lib.vnf_gallery_rows(h, ctypes.c_void_p(unit.data_ptr()), n0, rows.shape[0], _lib.current_stream_ptr()))
        self._emb = np.concatenate([self._emb, unit.cpu().numpy()])
        self._labels = np.concatenate([self._labels, lab])
        self._uploaded = self.size

    def _add_centroid(self, rows, lab, cuda):
        lib = _lib.load()
        classes = np.union1d(self._classes, lab)                      # ascending
        sums = np.zeros((classes.shape[0], self.input_dim), np.float32)
        counts = np.zeros((classes.shape[0],), np.int64)
        old = np.searchsorted(classes, self._classes)
        sums[old], counts[old] = self._sums, self._counts
        sums_d = torch.from_numpy(sums).to(cuda)
        counts_d = torch.zeros((classes.shape[0],), dtype=torch.int32, device=cuda)
        compact = torch.from_numpy(np.searchsorted(classes, lab).astype(np.int32)).to(cuda)
        _lib.check(lib.vnf_gallery_class_sums(ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(compact.data_ptr()), rows.shape[0],
                                              self.input_dim, ctypes.c_void_p(sums_d.data_ptr()), ctypes.c_void_p(counts_d.data_ptr()),
                                              classes.shape[0], _lib.current_stream_ptr()))
        self._classes, self._sums = classes, sums_d.cpu().numpy()
        self._counts = counts + counts_d.cpu().numpy().astype(np.int64)
        # the searchable matrix: one row per class, the normalised sum -- rebuilt, it is small
        self._drop()
        self._emb = np.zeros((0, self.input_dim), np.float32)
        self._labels = np.zeros((0,), np.int64)
        self._add_rows(sums_d, classes, cuda)

    # -- search ---------------------------------------------------------------------------------------------------
    def _probes(self, emb, k=None):
        """What search() and mated_search() ask of `emb`, in one order -> (device index, emb as contiguous fp32).
        k: search()'s k, tested here, between the empty-gallery test and the tests of `emb`, because that is where search()
        has always refused it: a call wrong in two ways keeps raising what it raised.  mated_search() has no k."""
        dev = self._dev()
        if self.size == 0:
            raise ValueError("the gallery is empty: enrol embeddings with .add() first")
        if k is not None and not 1 <= int(k) <= MAX_K:
            raise ValueError("k must lie in 1..%d, got %r" % (MAX_K, k))
        if emb.device.type != "cuda":
            raise RuntimeError("embeddings must live on the gallery's cuda device")
        if emb.dim() != 2 or emb.shape[1] != self.input_dim:
            raise ValueError("expected (F,%d) embeddings, got %s" % (self.input_dim, tuple(emb.shape)))
        return dev, emb.float().contiguous()

    def search(self, emb, k=1):
        """(F,input_dim) cuda embeddings (any norm) -> (idx (F,k) int32, label (F,k) int32, score (F,k) fp32): the k best
        rows per query under (cosine descending, row index ascending); slots beyond the gallery hold -1, -1, -inf."""
        dev, emb = self._probes(emb, k)
        k = int(k)
        h = self._ensure()
        f = emb.shape[0]
        idx = torch.empty((f, k), dtype=torch.int32, device=emb.device)
        label = torch.empty((f, k), dtype=torch.int32, device=emb.device)
        score = torch.empty((f, k), dtype=torch.float32, device=emb.device)
        lib = _lib.load()
        with torch.cuda.device(dev):
            for f0 in range(0, f, self.max_batch):
                nn = min(self.max_batch, f - f0)
                ws = _lib.workspace(lib.vnf_gallery_search_workspace_bytes(nn, k, self.size, self.chunk_rows), emb.device)
                _lib.check(lib.vnf_gallery_search(h, ctypes.c_void_p(emb[f0:].data_ptr()), nn, k, ctypes.c_void_p(idx[f0:].data_ptr()),
                                                  ctypes.c_void_p(label[f0:].data_ptr()), ctypes.c_void_p(score[f0:].data_ptr()),
                                                  self.chunk_rows, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
        return idx, label, score

    def _probe_ints(self, values, f, what, device):
        """(f) integers (host sequence, array or tensor) -> int32 cuda tensor; a wrong length or dtype is refused."""
        if not isinstance(values, torch.Tensor):
            a = np.asarray(values)
            if a.dtype.kind not in "iu" and a.size:
                raise ValueError("%s must be integers, got %s" % (what, a.dtype))
            values = torch.from_numpy(a.astype(np.int64))
        t = values
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("%s must be integers, got %s" % (what, t.dtype))
        if t.dim() != 1 or t.shape[0] != f:
            raise ValueError("expected %d %s, got shape %s" % (f, what, tuple(t.shape)))
        if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
            raise ValueError("%s must fit in int32" % what)
        return t.to(device=device, dtype=torch.int32).contiguous()

    def mated_search(self, emb, labels, exclude=None):
        """Calibration's search (vnf_gallery_mated_search): (F,input_dim) cuda probes of known `labels` (F integers) ->
        (idx, label, score), each (F,2): column 0 the best row of the probe's own label other than row exclude[f] (the
        mate), column 1 the best row of any other label (the non-mate), under search()'s order; an absent one is
        -1, -1, -inf.  exclude: None, or F row indices with -1 for "none" -- a gallery searched with its own rows passes
        arange(G)."""
        dev, emb = self._probes(emb)
        f = emb.shape[0]
        lab = self._probe_ints(labels, f, "labels", emb.device)
        exc = None if exclude is None else self._probe_ints(exclude, f, "exclude", emb.device)
        h = self._ensure()
        idx = torch.empty((f, 2), dtype=torch.int32, device=emb.device)
        label = torch.empty((f, 2), dtype=torch.int32, device=emb.device)
        score = torch.empty((f, 2), dtype=torch.float32, device=emb.device)
        lib = _lib.load()
        with torch.cuda.device(dev):
            for f0 in range(0, f, self.max_batch):
                nn = min(self.max_batch, f - f0)
                ws = _lib.workspace(lib.vnf_gallery_mated_search_workspace_bytes(nn, self.size, self.chunk_rows), emb.device)
                _lib.check(lib.vnf_gallery_mated_search(h, ctypes.c_void_p(emb[f0:].data_ptr()), ctypes.c_void_p(lab[f0:].data_ptr()),
                                                        ctypes.c_void_p(exc[f0:].data_ptr()) if exc is not None else None, nn,
                                                        ctypes.c_void_p(idx[f0:].data_ptr()), ctypes.c_void_p(label[f0:].data_ptr()),
                                                        ctypes.c_void_p(score[f0:].data_ptr()), self.chunk_rows,
                                                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
        return idx, label, score

    def cluster(self, threshold, min_samples=2):
        """DBSCAN over the gallery's own rows (vnf_gallery_cluster, csrc/gallery_cluster.hip): rows i != j are neighbours
        where the fp32 dot of the stored rows is >= `threshold` (a cosine), a row is core when it has min_samples - 1
        neighbours, clusters are the connected components of the core rows, a non-core row joins its best core neighbour's
        cluster.  -> (cluster (G) int32, -1 for noise; degree (G) int32; nn_idx (G) int32 and nn_score (G) fp32, each row's
        best other row; n_clusters int).  The tensors stay on the device; n_clusters is the one host read."""
        dev = self._dev()
        if self.size == 0:
            raise ValueError("the gallery is empty: enrol embeddings with .add() first")
        threshold = float(threshold)
        if not np.isfinite(threshold):
            raise ValueError("threshold must be a finite cosine, got %r" % (threshold,))
        if int(min_samples) != min_samples or int(min_samples) < 1:
            raise ValueError("min_samples must be an integer >= 1, got %r" % (min_samples,))
        h = self._ensure()
        g = self.size
        cuda = torch.device("cuda:%d" % dev)
        cluster = torch.empty((g,), dtype=torch.int32, device=cuda)
        degree = torch.empty((g,), dtype=torch.int32, device=cuda)
        nn_idx = torch.empty((g,), dtype=torch.int32, device=cuda)
        nn_score = torch.empty((g,), dtype=torch.float32, device=cuda)
        n_clusters = torch.empty((1,), dtype=torch.int32, device=cuda)
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = _lib.workspace(lib.vnf_gallery_cluster_workspace_bytes(g, self.chunk_rows), cuda)
            _lib.check(lib.vnf_gallery_cluster(h, threshold, int(min_samples), ctypes.c_void_p(cluster.data_ptr()),
                                               ctypes.c_void_p(degree.data_ptr()), ctypes.c_void_p(nn_idx.data_ptr()),
                                               ctypes.c_void_p(nn_score.data_ptr()), ctypes.c_void_p(n_clusters.data_ptr()),
                                               self.chunk_rows, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
            n = int(n_clusters.item())
        return cluster, degree, nn_idx, nn_score, n

    def classify(self, emb, want_logp=False):
        """MLPModel.classify's contract for want_logp=False: (None, top-1 label (F,) int32, its cosine (F,) fp32)."""
        if want_logp:
            raise NotImplementedError("a gallery has no probability model: there are no log-probabilities, only cosines "
                                      "(classify(emb, want_logp=False) or search(emb, k))")
        _, label, score = self.search(emb, 1)
        return None, label[:, 0].contiguous(), score[:, 0].contiguous()

    def forward(self, emb):
        raise NotImplementedError("a gallery has no probability model: calling it for log-probabilities is not defined; use "
                                  "classify(emb, want_logp=False) or search(emb, k)")

    __call__ = forward

    # -- one .npz file --------------------------------------------------------------------------------------------
    def save(self, path):
        d = {"embeddings": self._emb.astype(np.float32), "labels": self._labels.astype(np.int64), "mode": np.array(self.mode),
             "num_classes": np.array(self.num_classes, np.int64)}
        if self.mode == "centroid":
            d["sums"], d["counts"] = self._sums.astype(np.float32), self._counts.astype(np.int64)
        with open(path, "wb") as fp:
            np.savez(fp, **d)

    @classmethod
    def load(cls, path, max_batch=1024):
        with np.load(path, allow_pickle=False) as z:
            for key in ("embeddings", "labels", "mode", "num_classes"):
                if key not in z.files:
                    raise ValueError("%s is not a gallery file: no '%s'" % (path, key))
            emb, labels, mode, nc = z["embeddings"], z["labels"], str(z["mode"]), int(z["num_classes"])
            sums = z["sums"] if "sums" in z.files else None
            counts = z["counts"] if "counts" in z.files else None
        if emb.ndim != 2 or emb.dtype != np.float32 or labels.shape != (emb.shape[0],) or labels.dtype.kind not in "iu":
            raise ValueError("%s: embeddings must be (G,dim) float32 with (G) integer labels" % path)
        g = cls(emb.shape[1], nc, mode, max_batch)
        lab = check_rows(emb, labels, g.input_dim)
        g._emb, g._labels = np.ascontiguousarray(emb), lab
        if mode == "centroid":
            if sums is None or counts is None or sums.shape != emb.shape or counts.shape != lab.shape:
                raise ValueError("%s: a centroid gallery needs sums (C,dim) and counts (C), one per row" % path)
            if not np.isfinite(sums).all() or (lab.size > 1 and not (np.diff(lab) > 0).all()):
                raise ValueError("%s: centroid rows must be finite and in ascending label order" % path)
            g._classes, g._sums, g._counts = lab.copy(), np.ascontiguousarray(sums, np.float32), counts.astype(np.int64)
        return g
