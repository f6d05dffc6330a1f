"""GPU: gallery calibration through the CLIs -- enroll.py, then calibrate.py with a held-out probe set and again with
--self, on synthetic 512-d people (class centres plus noise, look-alikes in pairs), written as find_embedding.py writes
embeddings.  The float64 oracle (gallery_calibration_oracle.py) recomputes everything from the files; wherever a count or a
name is compared, the oracle's decisive gaps are asserted to exceed 4 tol first, for every probe."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import gallery_calibration_oracle as gco
import gallery_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIM, FAR = 512, 0.1
PEOPLE = [0, 1, 2, 3, 5, 6, 8, 9]       # enrolled labels: look-alike pairs (0,1) (2,3) (5,6) (8,9); 4 and 7 attract nobody
STRANGER = 7                            # sampled like the others, never enrolled
N_ENROL, N_PROBE, N_HELD = 6, 5, 3
TOL = go.tol(DIM)
ULP = 2.0 ** -23                        # of a float32 in [1, 2): an upper bound for cosines


def _people():
    """label -> (N_ENROL + N_PROBE + N_HELD, DIM) samples: a unit centre plus noise of norm about 0.5.  The two people of a
    pair share half of their centre (cosine about 0.5), so every probe has a non-mate score well above a stranger's."""
    rng = np.random.default_rng(2024)
    unit = lambda v: v / np.linalg.norm(v)
    out = {}
    labels = PEOPLE + [STRANGER]
    shared = {}
    for l in labels:
        pair = PEOPLE.index(l) // 2 if l in PEOPLE else -1
        if pair not in shared:
            shared[pair] = unit(rng.standard_normal(DIM))
        centre = unit(shared[pair] + unit(rng.standard_normal(DIM))) if pair >= 0 else unit(rng.standard_normal(DIM))
        n = N_ENROL + N_PROBE + N_HELD
        x = centre + 0.5 * rng.standard_normal((n, DIM)) / np.sqrt(DIM)
        out[l] = (x * rng.uniform(0.5, 20.0, (n, 1))).astype(np.float32)      # any norm: the encoders' are not unit either
    return out


def _run(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _write_set(tmp, name, samples):
    """samples: label -> (n,DIM).  <name>_emb/<label>_<i>.npz (arr_0) and <name>.json, as find_embedding.py / train.json."""
    d = tmp / (name + "_emb")
    d.mkdir()
    listing = {}
    for l, x in samples.items():
        for i, e in enumerate(x):
            np.savez_compressed(str(d / ("p%d_%d.npz" % (l, i))), e)
        listing[str(l)] = ["p%d_%d.png" % (l, i) for i in range(len(x))]
    lj = tmp / (name + ".json")
    lj.write_text(json.dumps(listing))
    return str(d), str(lj)


def _gaps_ok(s64, row_labels, idx, label, score, probe_labels, want):
    """The oracle's decisive gaps, every probe.  The count of impostors that pass is `a` on both sides once the a-th
    largest non-mate stands clear of the (a+1)-th, the pivot the threshold sits one ulp above (scores below the pivot may
    swap ranks among themselves: whichever becomes the pivot, the a above it pass and nothing else does).  Rank-1 and DIR
    need each mate clear of its non-mate and of its class's threshold."""
    non = np.sort(score[idx[:, 1] >= 0, 1])[::-1]
    a = int(np.floor(FAR * non.size + 1e-9))
    assert a >= 1 and non[a - 1] - non[a] > 4 * TOL
    m = idx[:, 0] >= 0
    assert (np.abs(score[m, 0] - score[m, 1]) > 4 * TOL).all()
    local = np.array([want["local"][str(int(l))] for l in probe_labels[m]])
    assert (np.abs(score[m, 0] - local) > 4 * TOL).all()
    # which class a stranger is charged to: the non-mate's label stands clear of every third label
    for p in range(len(probe_labels)):
        third = s64[p][(row_labels != probe_labels[p]) & (row_labels != label[p, 1])]
        assert third.size and score[p, 1] - third.max() > 4 * TOL, p


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("calibrate_cli")
    people = _people()
    enrol = {l: people[l][:N_ENROL] for l in PEOPLE}
    probe = {l: people[l][N_ENROL:N_ENROL + N_PROBE] for l in PEOPLE + [STRANGER]}     # the stranger's probes have no mate
    ed, ej = _write_set(tmp, "enrol", enrol)
    pd, pj = _write_set(tmp, "probe", probe)
    gal = str(tmp / "gallery.npz")
    _run([os.path.join(REPO, "enroll.py"), "-d", ed, "-l", ej, "-o", gal], str(tmp))
    w = {"tmp": tmp, "gallery": gal, "people": people}
    sys.path.insert(0, REPO)
    import enroll
    for name, extra in (("probe", ["-d", pd, "-l", pj]), ("self", ["--self"])):
        tj, rj = str(tmp / (name + "_thresholds.json")), str(tmp / (name + "_report.json"))
        so = _run([os.path.join(REPO, "calibrate.py"), "-g", gal, "--far", repr(FAR), "-o", tj, "-r", rj, "-dv", "GPU"] + extra, str(tmp))
        w[name] = {"stdout": so, "thresholds": json.load(open(tj)), "report": json.load(open(rj)), "thresholds_path": tj}
    with np.load(gal, allow_pickle=False) as z:
        w["rows"], w["labels"], w["nc"] = z["embeddings"], z["labels"], int(z["num_classes"])
    w["probe"]["emb"], w["probe"]["labels"] = enroll.load_samples(pd, pj)
    w["probe"]["exclude"] = None
    w["self"]["emb"], w["self"]["labels"], w["self"]["exclude"] = w["rows"], w["labels"], np.arange(len(w["labels"]))
    for name in ("probe", "self"):
        p = w[name]
        p["s64"] = go.scores(p["emb"], w["rows"])
        p["oracle_scores"] = gco.mated(p["s64"], w["labels"], p["labels"], p["exclude"])
        p["oracle"] = gco.calibrate(*p["oracle_scores"], p["labels"], FAR, w["nc"])
    return w


@pytest.mark.parametrize("name", ["probe", "self"])
def test_threshold_far_and_counts_equal_the_oracle(world, name):
    from vn_celeb_face_recognition_amd.gallery import GalleryModel
    p, want = world[name], world[name]["oracle"]
    rep, thr = p["report"], p["report"]["thr"]
    oi, ol, osc = p["oracle_scores"]
    _gaps_ok(p["s64"], world["labels"], oi, ol, osc, p["labels"], want)
    assert world["nc"] == 10 and len(world["labels"]) == len(PEOPLE) * N_ENROL
    print("%s: thr %r, oracle %r (tol %.3g)" % (name, thr, want["thr"], TOL))
    assert abs(thr - want["thr"]) <= TOL + ULP
    assert (rep["Fm"], rep["Fn"]) == (want["Fm"], want["Fn"])
    assert rep["Fm"] == (len(PEOPLE) * N_PROBE if name == "probe" else len(world["labels"])) and rep["Fn"] == len(p["labels"])
    assert (rep["achieved_far"], rep["dir"], rep["rank1"]) == (want["far"], want["dir"], want["rank1"])
    assert rep["far_target"] == FAR and rep["protocol"] == ("probe set" if name == "probe" else "self")
    pts = {q["far"]: q for q in rep["operating_points"]}
    assert sorted(pts) == [0.1] and (pts[0.1]["thr"], pts[0.1]["achieved_far"], pts[0.1]["dir"]) == (thr, rep["achieved_far"], rep["dir"])
    assert repr(thr) in p["stdout"] and "achieved FAR" in p["stdout"] and "DIR" in p["stdout"]
    # the per-class thresholds: the file's shape, each within tol + ulp of the oracle's, none below the global one
    local = p["thresholds"]
    assert list(local) == [str(c) for c in range(world["nc"])]
    assert all(abs(local[c] - want["local"][c]) <= TOL + ULP and local[c] >= thr for c in local)
    assert local["4"] == thr and local["7"] == thr                                # nobody's non-mate: the global threshold
    # the achieved FAR recounted from mated_search's own scores
    gal = GalleryModel.load(world["gallery"]).to(DEV)
    idx, _, sc = gal.mated_search(torch.from_numpy(np.ascontiguousarray(p["emb"])).to(DEV), p["labels"], p["exclude"])
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    has = idx[:, 1] >= 0
    passed = int((sc[has, 1] >= np.float32(thr)).sum())
    assert passed / has.sum() <= FAR and passed / has.sum() == rep["achieved_far"]
    assert np.array_equal(has, oi[:, 1] >= 0) and np.array_equal(idx[:, 0] >= 0, oi[:, 0] >= 0)


def test_calibrated_thresholds_name_the_enrolled_and_reject_the_stranger(world):
    from vn_celeb_face_recognition_amd import statistics
    from vn_celeb_face_recognition_amd.gallery import GalleryModel
    from vn_celeb_face_recognition_amd.pipeline import identify_names
    people = world["people"]
    held = np.concatenate([people[l][-N_HELD:] for l in PEOPLE] + [people[STRANGER][-N_HELD:]])
    truth = [l for l in PEOPLE for _ in range(N_HELD)]
    _, ol, osc = go.topk(go.scores(held, world["rows"]), world["labels"], len(world["labels"]))
    df = {"label": list(range(10)), "name": ["person_%d" % i for i in range(10)]}
    gal = GalleryModel.load(world["gallery"]).to(DEV).eval()
    _, amax, prob = gal.classify(torch.from_numpy(held).to(DEV), want_logp=False)
    for name in ("probe", "self"):
        local = statistics.build_thresholds(world[name]["thresholds_path"], world["nc"], 0.7)
        assert local == world[name]["thresholds"]
        for i in range(held.shape[0]):
            best = ol[i, 0]
            other = osc[i][ol[i] != best][0]                   # the best row of another label
            assert abs(osc[i, 0] - local[str(int(best))]) > 4 * TOL and osc[i, 0] - other > 4 * TOL, (name, i)
            if i < len(truth):
                assert best == truth[i] and osc[i, 0] > local[str(int(best))], (name, i)
            else:
                assert osc[i, 0] < local[str(int(best))], (name, i)
        names = identify_names(amax, prob, gal.num_classes, df, local)
        assert names == ["person_%d" % l for l in truth] + ["Unknown"] * N_HELD, name
