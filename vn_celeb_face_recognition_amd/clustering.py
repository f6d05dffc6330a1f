"""What cluster.py does with the cluster ids of GalleryModel.cluster (csrc/gallery_cluster.hip): plain Python and numpy, no GPU.

groups() turns the ids of unlabelled embeddings into the {label: [file names]} file enroll.py -l reads, cluster id for
label.  purity_report() sets the clusters of a labelled gallery against its labels: a row whose label is not its
cluster's majority label is a candidate for a wrong label, a cluster with several labels a candidate for one person
enrolled twice (or for a threshold that is too low), a label spread over several clusters the reverse.  Noise rows
(cluster -1) belong to no cluster and are listed on their own.  A majority is the most frequent label, the smallest one
among equally frequent ones."""
import json

import numpy as np


def _ids(cluster):
    c = np.asarray(cluster)
    if c.ndim != 1 or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("cluster must be a 1-d integer array, got %s %s" % (c.dtype, c.shape))
    c = c.astype(np.int64)
    if c.size and int(c.min()) < -1:
        raise ValueError("cluster ids are >= 0, or -1 for noise")
    return c


def groups(cluster, names):
    """-> ({"0": [names of cluster 0, in row order], "1": ...}, [names of the noise rows]); ids ascending."""
    c = _ids(cluster)
    names = list(names)
    if len(names) != c.shape[0]:
        raise ValueError("%d names for %d rows" % (len(names), c.shape[0]))
    out, noise = {}, []
    for k in sorted(set(c.tolist()) - {-1}):
        out[str(k)] = []
    for k, name in zip(c.tolist(), names):
        (noise if k < 0 else out[str(k)]).append(name)
    return out, noise


def purity_report(cluster, labels):
    """-> {"rows", "n_clusters", "noise_rows": [row...],
           "clusters": {id: {"size", "labels": {label: count}, "majority"}},
           "labels": {label: {"rows", "clusters": [id...], "noise"}},
           "suspect_rows": [{"row", "label", "cluster", "majority"}...],     # label != its cluster's majority label
           "mixed_clusters": [id...]}                                       # clusters that hold more than one label"""
    c = _ids(cluster)
    lab = np.asarray(labels)
    if lab.shape != c.shape or (lab.size and lab.dtype.kind not in "iu"):
        raise ValueError("expected %d integer labels, got %s %s" % (c.shape[0], lab.dtype, lab.shape))
    lab = lab.astype(np.int64)
    clusters, per_label = {}, {}
    for k in sorted(set(c.tolist()) - {-1}):
        values, counts = np.unique(lab[c == k], return_counts=True)           # ascending labels: argmax takes the smallest
        clusters[str(k)] = {"size": int(counts.sum()), "labels": {str(int(v)): int(n) for v, n in zip(values, counts)},
                            "majority": int(values[np.argmax(counts)])}
    for v in sorted(set(lab.tolist())):
        mine = c[lab == v]
        per_label[str(v)] = {"rows": int(mine.size), "clusters": sorted(set(mine[mine >= 0].tolist())), "noise": int((mine < 0).sum())}
    suspects = [{"row": int(i), "label": int(lab[i]), "cluster": int(c[i]), "majority": clusters[str(int(c[i]))]["majority"]}
                for i in np.flatnonzero(c >= 0) if clusters[str(int(c[i]))]["majority"] != lab[i]]
    return {"rows": int(c.size), "n_clusters": len(clusters), "noise_rows": [int(i) for i in np.flatnonzero(c < 0)],
            "clusters": clusters, "labels": per_label, "suspect_rows": suspects,
            "mixed_clusters": [int(k) for k, v in clusters.items() if len(v["labels"]) > 1]}


def write_groups(path, grouped):
    """The {cluster id: [file names]} json enroll.py -l reads."""
    with open(path, "w") as fp:
        json.dump(grouped, fp, indent=1)
        fp.write("\n")


def write_noise(path, noise):
    with open(path, "w") as fp:
        fp.write("".join(name + "\n" for name in noise))


def write_report(path, report):
    with open(path, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
