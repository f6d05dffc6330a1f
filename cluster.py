#!/usr/bin/env python3
"""Group unlabelled face embeddings into identities, or set a gallery's clusters against its labels (DBSCAN over cosines,
GalleryModel.cluster on the GPU):

    cluster.py -d faces_emb --threshold T [--min_samples 2] -o clusters.json [--noise_file noise.txt] [-r report.json] -dv GPU
    cluster.py -g gallery.npz --threshold T [--min_samples 2] -r report.json -dv GPU

-d: every <stem>.npz find_embedding.py wrote under faces_emb, in sorted order.  Two faces are neighbours where their cosine
is >= T, a face with min_samples - 1 neighbours is the core of a cluster, clusters are what such faces connect, a face
beside a cluster joins its best neighbour's, and the rest is noise.  clusters.json is {cluster id: [file names]}: what
enroll.py -l reads, so `enroll.py -d faces_emb -l clusters.json` enrols the clusters as labels; the noise files go to
--noise_file, one per line; -r adds every file's cluster, number of neighbours and best cosine to another file.
-g: the gallery's own rows are clustered and report.json says where clusters and labels disagree
(vn_celeb_face_recognition_amd/clustering.py): rows whose label is not their cluster's majority label, clusters that
hold several labels, labels spread over several clusters.
--threshold is a cosine and has no default: take the one calibrate.py prints for the same encoder."""
import argparse
from pathlib import Path

import numpy as np

from vn_celeb_face_recognition_amd import clustering
from vn_celeb_face_recognition_amd import models as model_md


def build_parser():
    ap = argparse.ArgumentParser(description='Cluster face embeddings into identities (DBSCAN over cosines)')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('-d', '--data_dir', default=None, help='the <stem>.npz files find_embedding.py writes')
    src.add_argument('-g', '--gallery', default=None, help='a gallery whose rows are clustered and compared with its labels')
    ap.add_argument('--threshold', type=float, required=True, help="neighbours have a cosine >= this (calibrate.py's threshold)")
    ap.add_argument('--min_samples', type=int, default=2, help='a core face has this many faces within the threshold, itself included')
    ap.add_argument('-o', '--output', default='clusters.json', help='-d: {cluster id: [file names]}, as enroll.py -l reads')
    ap.add_argument('--noise_file', default=None, help='-d: the files that joined no cluster, one per line')
    ap.add_argument('-r', '--report', default=None, help='-d: per-file detail; -g: the purity report (default report.json)')
    ap.add_argument('-dv', '--device', default='GPU')
    return ap


def check_args(args):
    if args.device != 'GPU':
        raise SystemExit("this build runs on MI355X only: use -dv GPU (there is no CPU path)")
    if not np.isfinite(args.threshold):
        raise SystemExit("--threshold: a finite cosine is needed, got {!r}".format(args.threshold))
    if args.min_samples < 1:
        raise SystemExit("--min_samples: must be >= 1, got {}".format(args.min_samples))


def load_dir(data_dir):
    """Every <stem>.npz under data_dir in sorted order, read as enroll.load_samples reads them -> (file names, (n,dim))."""
    paths = sorted(Path(data_dir).glob("*.npz"))
    if not paths:
        raise SystemExit("{} holds no .npz files: nothing to cluster".format(data_dir))
    embs = [np.asarray(np.load(str(p), allow_pickle=False)["arr_0"], np.float32).reshape(-1) for p in paths]
    for p, e in zip(paths, embs):
        if e.shape[0] != embs[0].shape[0]:
            raise SystemExit("{} holds {} values, the others {}".format(p, e.shape[0], embs[0].shape[0]))
    return [p.name for p in paths], np.stack(embs)


def run_cluster(gallery, args):
    """-> (cluster, degree, nn_idx, nn_score) as host arrays, n_clusters."""
    gallery.to("cuda:0")
    *out, n = gallery.cluster(args.threshold, args.min_samples)
    return [t.cpu().numpy() for t in out], n


def _score(v):
    return float(v) if np.isfinite(v) else None


def cluster_dir(args):
    names, emb = load_dir(args.data_dir)
    try:
        gallery = model_md.GalleryModel(emb.shape[1]).to("cuda:0").add(emb, np.zeros(len(names), np.int64))
    except ValueError as ex:
        raise SystemExit("embeddings refused: {}".format(ex))
    (cluster, degree, nn_idx, nn_score), n = run_cluster(gallery, args)
    grouped, noise = clustering.groups(cluster, names)
    clustering.write_groups(args.output, grouped)
    if args.noise_file:
        clustering.write_noise(args.noise_file, noise)
    borders = int(((cluster >= 0) & (degree + 1 < args.min_samples)).sum())
    print('{} files: {} clusters, {} border files, {} noise files at cosine >= {!r}, min_samples {}'.format(
        len(names), n, borders, len(noise), args.threshold, args.min_samples))
    for k in sorted(grouped, key=lambda k: (-len(grouped[k]), int(k)))[:5]:
        print('  cluster {}: {} files'.format(k, len(grouped[k])))
    if args.report:
        rows = [{"file": name, "cluster": int(c), "degree": int(d), "nn_file": names[j] if j >= 0 else None, "nn_score": _score(s)}
                for name, c, d, j, s in zip(names, cluster, degree, nn_idx, nn_score)]
        clustering.write_report(args.report, {"data_dir": args.data_dir, "threshold": args.threshold, "min_samples": args.min_samples,
                                              "n_clusters": n, "borders": borders, "noise": len(noise), "rows": rows})
    print('Clusters saved at {} ...'.format(args.output))
    return grouped, noise


def cluster_gallery(args):
    gallery = model_md.GalleryModel.load(args.gallery)
    if gallery.size == 0:
        raise SystemExit("{} is empty: nothing to cluster".format(args.gallery))
    (cluster, degree, _, nn_score), n = run_cluster(gallery, args)
    report = clustering.purity_report(cluster, gallery._labels)
    report.update({"gallery": args.gallery, "mode": gallery.mode, "threshold": args.threshold, "min_samples": args.min_samples,
                   "degree": [int(d) for d in degree], "nn_score": [_score(s) for s in nn_score]})
    path = args.report or 'report.json'
    clustering.write_report(path, report)
    print('{} rows of {} labels: {} clusters, {} noise rows, {} rows whose label is not their cluster\'s majority, {} clusters with '
          'several labels'.format(gallery.size, len(report["labels"]), n, len(report["noise_rows"]), len(report["suspect_rows"]),
                                  len(report["mixed_clusters"])))
    print('Report saved at {} ...'.format(path))
    return report


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    return cluster_dir(args) if args.data_dir is not None else cluster_gallery(args)


if __name__ == "__main__":
    main()
