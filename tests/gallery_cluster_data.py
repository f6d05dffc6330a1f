"""The rows the clustering tests share (test_gpu_gallery_cluster.py, test_gpu_cluster_cli.py, test_clustering_host.py):
every DBSCAN role at threshold T = 0.5 and dim 512, with no pair near the threshold.

  blobs       unit(c + r z): a unit centre c, a unit random z, r uniform in [0.6, 0.8]; cosines inside a blob 0.56 .. 0.78
  satellites  m + 1.33 z on a blob member m: cosine 0.6 to m, below 0.5 to the rest of the blob -- borders
  bridges     m1 + 0.95 m2 + 0.9 z between members of two blobs: degree 2, core at min_samples 3 (the blobs merge), a
              contested border at min_samples 4
  chain       e_k + e_(k+1) + 0.55 e_(L+1), rotated by a random orthogonal matrix: consecutive cosines 0.566, all others
              0.131 -- one long cluster at min_samples <= 3, all noise at 4
  the rest    pure-noise rows, three exact duplicates of earlier rows, a random permutation, norms scaled to 0.1 .. 30

The seeds were chosen so that both oracle margins (gallery_cluster_oracle) exceed 4 tol(512) at min_samples 1, 3 and 4;
the tests assert that on the CPU before they compare anything."""
import functools

import numpy as np

import gallery_cluster_oracle as gco
import gallery_oracle as go

T = 0.5
DIM = 512
CASES = {"small": dict(seed=11, blobs=(17, 16, 5, 3, 2), chain=40, noise=20, satellites=4, bridges=2),
         "large": dict(seed=12, blobs=(300, 150, 64, 33, 32, 31, 9, 4, 3, 2), chain=180, noise=150, satellites=12, bridges=4)}


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def chain_rows(length, rng, dim=DIM):
    """`length` rows, each a neighbour of the next only."""
    assert length + 2 <= dim
    v = np.zeros((length, dim))
    v[np.arange(length), np.arange(length)] = 1.0
    v[np.arange(length), np.arange(length) + 1] = 1.0
    v[:, length + 1] = 0.55
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    return v @ q


def make(seed, blobs, chain, noise, satellites, bridges, dim=DIM):
    rng = np.random.default_rng(seed)
    members = []
    for size in blobs:
        c = _unit(rng.standard_normal(dim))
        members.append(_unit(c + rng.uniform(0.6, 0.8, (size, 1)) * _unit(rng.standard_normal((size, dim)))))
    rows = list(members)
    big = [m for m in members if m.shape[0] >= 5]
    sat = [big[i % len(big)][rng.integers(0, big[i % len(big)].shape[0])] + 1.33 * _unit(rng.standard_normal(dim))
           for i in range(satellites)]
    bri = []
    for i in range(bridges):
        a, b = big[i % len(big)], big[(i + 1) % len(big)]
        bri.append(a[rng.integers(0, a.shape[0])] + 0.95 * b[rng.integers(0, b.shape[0])] + 0.9 * _unit(rng.standard_normal(dim)))
    rows += [np.stack(sat), np.stack(bri), chain_rows(chain, rng, dim), _unit(rng.standard_normal((noise, dim)))]
    x = np.concatenate(rows)
    x = np.concatenate([x, x[rng.permutation(x.shape[0])[:3]]])                  # three exact duplicates
    x = x[rng.permutation(x.shape[0])]
    x = _unit(x) * rng.uniform(0.1, 30.0, (x.shape[0], 1))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rows (N,512) float32, float64 scores (N,N)), both read-only."""
    x = make(**CASES[name])
    s = go.scores(x, x)
    x.setflags(write=False); s.setflags(write=False)
    return x, s


@functools.lru_cache(maxsize=None)
def oracle(name, min_samples, n=None):
    """The oracle of the case's first n rows (all by default) at T, with its margins asserted."""
    x, s = case(name)
    n = x.shape[0] if n is None else n
    o = gco.cluster_scores(s[:n, :n], T, min_samples)
    assert o.margin_t > 4 * go.tol(DIM) and o.margin_border > 4 * go.tol(DIM), (name, min_samples, n, o.margin_t, o.margin_border)
    return o
