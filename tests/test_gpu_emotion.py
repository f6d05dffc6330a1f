"""GPU: the emotion network (ResNet-50, class + projection heads) against the reference golden, its three kernels
(padded max pool, Pillow-exact face transform, softmax top-k), batch behaviour, the resident recognize path, the
FacePipeline hook and demo_image.py --recog_emotion."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO, load_image, seeded_normal
from emotion_restatement import rn50_2b_forward

pytestmark = pytest.mark.gpu
NC, NP = 690, 300
DEV = "cuda:0"

# relative L2 per row against the reference golden, measured on the MI355X (worst of x_cls / x_proj over the golden's
# two rows); the test bounds are twice these, capped by what the project accepts for the dtypes on IRv1
MEASURED_BF16 = 3.65e-3   # x_cls 3.64e-3 3.65e-3, x_proj 3.61e-3 3.56e-3 -> bound 7.3e-3 (cap 6e-2)
MEASURED_F16 = 4.63e-4    # x_cls 4.63e-4 4.48e-4, x_proj 4.28e-4 4.14e-4 -> bound 9.3e-4 (cap 8e-3)


def _golden():
    return np.load(os.path.join(GOLDEN, "rn50_2b_seed0.npz"))


def _sd():
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    return generate_state_dict("rn50_2b", 0, as_torch=True, num_classes=NC, num_projections=NP)


_MODELS = {}


def _model(dt, max_batch=8):
    from vn_celeb_face_recognition_amd import models
    key = (dt, max_batch)
    if key not in _MODELS:
        _MODELS[key] = models.resnet_2branch_50(num_classes=NC, num_projections=NP, compute_dtype=dt, max_batch=max_batch).to(DEV).eval()
    return _MODELS[key]


def _rel(got, want):
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


@pytest.mark.parametrize("dt", ["f32", "f16x2"])
def test_matches_reference_golden_and_top6(dt):
    from vn_celeb_face_recognition_amd.pipeline import find_emotion
    g = _golden()
    x = seeded_normal((2, 3, 224, 224), int(g["input_seed"])).to(DEV)
    m = _model(dt)
    cls, proj = m(x)
    assert cls.is_cuda and proj.is_cuda and cls.dtype == proj.dtype == torch.float32
    assert tuple(cls.shape) == (2, NC) and tuple(proj.shape) == (2, NP)
    rc, rp = _rel(cls.cpu().numpy(), g["x_cls"]), _rel(proj.cpu().numpy(), g["x_proj"])
    print("rn50_2b %s: rel L2 per row  x_cls %s  x_proj %s" % (dt, rc, rp))
    assert (rc <= 1e-4).all() and (rp <= 1e-4).all(), (rc, rp)
    idx, prob = find_emotion(x, m, topk=6)
    print("rn50_2b %s: top-6 %s max prob err %.3e" % (dt, idx.tolist(), np.abs(prob - g["top6_prob"]).max()))
    assert np.array_equal(idx, g["top6_idx"].astype(np.int64))
    assert np.abs(prob - g["top6_prob"]).max() <= 1e-4


def test_stage_taps_f32_match_restatement():
    g = _golden()
    x = seeded_normal((2, 3, 224, 224), int(g["input_seed"]))
    want = {}
    rn50_2b_forward(_sd(), x, want)
    m = _model("f32")
    m(x.to(DEV))
    for name in ("stem", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool"):
        got = m.tap(name, 2)
        w = want[name].numpy()
        assert got.shape == w.shape, (name, got.shape, w.shape)
        err = float(np.abs(got - w).max())
        tol = 1e-4 * max(1.0, float(np.abs(w).max()))
        print("tap %-8s max abs err %.3e (tol %.3e, max |want| %.3f)" % (name, err, tol, np.abs(w).max()))
        assert err <= tol, (name, err)
    # the padded pool is an exact operation: the device's pool of the device's stem, bit for bit
    assert np.array_equal(m.tap("maxpool", 2), F.max_pool2d(torch.from_numpy(m.tap("stem", 2)), 3, 2, 1).numpy())


@pytest.mark.parametrize("dt,measured,cap", [("bf16", MEASURED_BF16, 6e-2), ("f16", MEASURED_F16, 8e-3)])
def test_16bit_dtypes_against_golden(dt, measured, cap):
    g = _golden()
    x = seeded_normal((2, 3, 224, 224), int(g["input_seed"])).to(DEV)
    cls, proj = _model(dt)(x)
    rc, rp = _rel(cls.cpu().numpy(), g["x_cls"]), _rel(proj.cpu().numpy(), g["x_proj"])
    print("rn50_2b %s: rel L2 per row  x_cls %s  x_proj %s" % (dt, rc, rp))
    bound = min(2 * measured, cap)
    assert max(rc.max(), rp.max()) <= bound, (rc, rp, bound)
    assert np.array_equal(cls.argmax(1).cpu().numpy(), g["top6_idx"][:, 0])


# ------------------------------------------------------------------------------------------------ padded max pool
def _pool(x_nhwc, code, planar=0):
    from vn_celeb_face_recognition_amd import _lib
    n, h, w, c = x_nhwc.shape[0], x_nhwc.shape[1], x_nhwc.shape[2], x_nhwc.shape[3]
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x_nhwc.shape[3]), dtype=x_nhwc.dtype, device=x_nhwc.device)
    _lib.check(_lib.load().vnf_maxpool3s2p1(ctypes.c_void_p(x_nhwc.data_ptr()), code, planar, n, h, w, c,
                                            ctypes.c_void_p(y.data_ptr()), _lib.current_stream_ptr()))
    return y


def _split(x):
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


@pytest.mark.parametrize("hw", [(13, 9), (12, 16), (1, 1)])
def test_padded_maxpool_all_layouts(hw):
    from vn_celeb_face_recognition_amd import _lib
    h, w = hw
    x = seeded_normal((3, 16, h, w), 7 + h)
    want = F.max_pool2d(x, 3, 2, 1)
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    got = _pool(xn, _lib.VNF_F32)
    assert torch.equal(got.cpu().permute(0, 3, 1, 2), want)               # exact in f32
    for tdt, code in ((torch.bfloat16, _lib.VNF_BF16), (torch.float16, _lib.VNF_F16)):
        got = _pool(xn.to(tdt), code)
        assert torch.equal(got.cpu().permute(0, 3, 1, 2).float(), F.max_pool2d(x.to(tdt).float(), 3, 2, 1))
    # split-f16 pairs: interleaved (hi, lo) per value, and the planar units [8 hi][8 lo] the encoders keep
    hi, lo = _split(xn)
    pairs = torch.stack([hi, lo], dim=-1).contiguous().view(torch.int32).view(xn.shape)
    o = _pool(pairs, _lib.VNF_F16X2).view(torch.float16).view(*want.permute(0, 2, 3, 1).shape, 2).float().sum(-1)
    xs = (hi.float() + lo.float()).cpu().permute(0, 3, 1, 2)
    assert torch.equal(o.cpu().permute(0, 3, 1, 2), F.max_pool2d(xs, 3, 2, 1))
    n, H, W, C = xn.shape
    planar = torch.stack([hi.view(n, H, W, C // 8, 8), lo.view(n, H, W, C // 8, 8)], dim=-2).contiguous().view(torch.int32).view(xn.shape)
    o = _pool(planar, _lib.VNF_F16X2, planar=1)
    o = o.view(torch.float16).view(n, o.shape[1], o.shape[2], C // 8, 2, 8).float().sum(-2).reshape(n, o.shape[1], o.shape[2], C)
    assert torch.equal(o.cpu().permute(0, 3, 1, 2), F.max_pool2d(xs, 3, 2, 1))


# ------------------------------------------------------------------------------------------------ face transform
def _resized_ref(a):
    try:
        from PIL import Image
        return np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR))
    except ImportError:
        from vn_celeb_face_recognition_amd.emotion import pillow_bilinear_resize
        return pillow_bilinear_resize(a)


@pytest.mark.parametrize("S", [96, 112, 150, 160, 181, 224])
def test_emotion_prep_is_pillow_exact(S):
    from vn_celeb_face_recognition_amd.emotion import emotion_prep_device
    from vn_celeb_face_recognition_amd.pipeline import trans_emotion_inf
    rng = np.random.default_rng(S)
    faces = rng.integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    img = load_image("mrDam_HaHo_recog.jpg")
    faces[2] = img[20:20 + S, 50:50 + S]
    mean, std = np.array([0.485, 0.456, 0.406], np.float64), np.array([0.229, 0.224, 0.225], np.float64)
    d = torch.from_numpy(faces).to(DEV)
    got = emotion_prep_device(d, torch.float32).cpu().numpy()
    assert got.shape == (3, 3, 224, 224)
    want_bytes = np.stack([_resized_ref(f) for f in faces])
    got_bytes = np.rint((got.transpose(0, 2, 3, 1).astype(np.float64) * std + mean) * 255.0).astype(np.int64)
    assert int((got_bytes != want_bytes).sum()) == 0
    want = np.stack([trans_emotion_inf(f).numpy() for f in faces])
    assert np.abs(got - want).max() <= 1e-6
    for tdt, mant in ((torch.float16, 10), (torch.bfloat16, 7)):
        g16 = emotion_prep_device(d, tdt).float().cpu().numpy()
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14))) - mant)
        assert (np.abs(g16 - want) <= ulp).all()
    assert emotion_prep_device(d[:0]).shape == (0, 3, 224, 224)
    with pytest.raises(Exception, match="224"):
        emotion_prep_device(torch.zeros((1, 225, 225, 3), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ softmax top-k
@pytest.mark.parametrize("C", [7, 690, 1000])
@pytest.mark.parametrize("k", [1, 6, 16])
def test_softmax_topk_matches_torch(C, k):
    from vn_celeb_face_recognition_amd import _lib
    from vn_celeb_face_recognition_amd.emotion import softmax_topk_device
    logits = (seeded_normal((37, C), 100 * C + k) * 5).to(DEV)
    if k > C:
        with pytest.raises(_lib.VnfError, match="-1"):
            softmax_topk_device(logits, k)
        return
    idx, prob = softmax_topk_device(logits, k)
    sm = torch.softmax(logits.cpu(), dim=1)
    wp, wi = sm.sort(dim=1, descending=True, stable=True)
    assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), wi[:, :k])
    assert (prob.cpu() - wp[:, :k]).abs().max() <= 1e-6


def test_softmax_topk_tie_rule_and_argument_checks():
    from vn_celeb_face_recognition_amd import _lib
    from vn_celeb_face_recognition_amd.emotion import softmax_topk_device
    row = torch.zeros(200)
    row[[150, 3, 77]] = 4.0           # three exact ties for the first place
    row[[199, 64]] = 2.5              # two for the fourth, one of them in another lane stride
    logits = torch.stack([row, torch.ones(200)]).to(DEV)
    idx, prob = softmax_topk_device(logits, 6)
    assert idx[0].tolist() == [3, 77, 150, 64, 199, 0] and idx[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert torch.allclose(prob[1].cpu(), torch.full((6,), 1 / 200.0), atol=1e-8)
    for k in (0, 17):
        with pytest.raises(_lib.VnfError):
            softmax_topk_device(logits, k)
    i0, p0 = softmax_topk_device(logits[:0], 3)
    assert i0.shape == (0, 3) and p0.shape == (0, 3)
    # no softmax exists for a row of -inf only: indices in order, probabilities 0; NaN logits are never picked
    odd = torch.full((2, 5), float("-inf"))
    odd[1] = torch.tensor([float("nan"), 1.0, float("nan"), 2.0, float("nan")])
    idx, prob = softmax_topk_device(odd.to(DEV), 3)
    assert idx[0].tolist() == [0, 1, 2] and prob[0].tolist() == [0.0, 0.0, 0.0]
    assert idx[1].tolist() == [3, 1, -1] and prob[1, 2].item() == 0.0
    assert torch.allclose(prob[1, :2].cpu(), torch.softmax(torch.tensor([2.0, 1.0]), 0), atol=1e-6)


# ------------------------------------------------------------------------------------------------ batches
def test_batch_behaviour():
    from vn_celeb_face_recognition_amd import _lib
    m = _model("f16x2", max_batch=4)
    x = seeded_normal((10, 3, 224, 224), 21).to(DEV)
    cls, proj = m(x)                                   # 10 > max_batch: chunks of 4, 4, 2
    assert tuple(cls.shape) == (10, NC) and tuple(proj.shape) == (10, NP)
    for i in (0, 5, 9):                                # every row is what the image gives alone
        c1, p1 = m(x[i:i + 1])
        assert (_rel(c1.cpu().numpy(), cls[i:i + 1].cpu().numpy()) <= 1e-6).all()
        assert (_rel(p1.cpu().numpy(), proj[i:i + 1].cpu().numpy()) <= 1e-6).all()
    c0, p0 = m(x[:0])
    assert tuple(c0.shape) == (0, NC) and tuple(p0.shape) == (0, NP)
    with pytest.raises(ValueError):
        m(torch.zeros((1, 3, 160, 160), device=DEV))
    with pytest.raises(RuntimeError):
        m(torch.zeros((1, 3, 224, 224)))
    # the ABI itself refuses a batch above max_batch, and takes either output as NULL
    lib, h = _lib.load(), m._ensure_handle()
    out = torch.empty((5, NC), device=DEV)
    rc = lib.vnf_emotion_forward(h, ctypes.c_void_p(x.data_ptr()), 5, _lib.VNF_F32, ctypes.c_void_p(out.data_ptr()), None,
                                 _lib.current_stream_ptr())
    assert rc == -4
    po = torch.empty((2, NP), device=DEV)
    _lib.check(lib.vnf_emotion_forward(h, ctypes.c_void_p(x.data_ptr()), 2, _lib.VNF_F32, None, ctypes.c_void_p(po.data_ptr()),
                                       _lib.current_stream_ptr()))
    assert torch.equal(po, proj[:2])
    faces = torch.zeros((5, 112, 112, 3), dtype=torch.uint8, device=DEV)
    ti, tp = torch.empty((5, 6), dtype=torch.int32, device=DEV), torch.empty((5, 6), device=DEV)
    rec = lambda n, s, k: lib.vnf_emotion_recognize(h, ctypes.c_void_p(faces.data_ptr()), n, s, k, ctypes.c_void_p(ti.data_ptr()),   # noqa: E731
                                                    ctypes.c_void_p(tp.data_ptr()), None, _lib.current_stream_ptr())
    assert rec(5, 112, 6) == -4 and rec(4, 112, 6) == 0 and rec(0, 112, 6) == 0
    assert rec(2, 225, 6) == -1 and rec(2, 112, 17) == -1 and rec(2, 112, 0) == -1
    assert lib.vnf_embed(h, ctypes.c_void_p(x.data_ptr()), 1, _lib.VNF_F32, ctypes.c_void_p(out.data_ptr()), _lib.current_stream_ptr()) == -1
    a, e = m.flops_per_image()
    assert 8.0e9 < a < 8.5e9 and a <= e < 1.15 * a       # ResNet-50 at 224: ~4.1 GMACs; the padded stem adds ~7 %
    assert "layer4.2.conv3" in m.profile(x[:2]) and "maxpool_pad1" in m.profile(x[:2])


def _faces(n, S, seed):
    img = load_image("mrDam_HaHo_recog.jpg")
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        y0, x0 = int(rng.integers(0, img.shape[0] - S)), int(rng.integers(0, img.shape[1] - S))
        out.append(np.ascontiguousarray(img[y0:y0 + S, x0:x0 + S]))
    return out


def test_recognize_emotion_device_path_equals_host_transform_path():
    from vn_celeb_face_recognition_amd.pipeline import recognize_emotion, trans_emotion_inf
    names = json.load(open(os.path.join(GOLDEN, "etag2idx.json")))["idx2key"]
    mp = np.vectorize(lambda i: names[i])
    m = _model("f16x2", max_batch=4)
    f = _faces(6, 112, 3)
    bth = [[f[0], f[1]], [], [f[2]], [f[3], f[4], f[5]]]          # 6 faces > max_batch 4
    tags_d, probs_d = recognize_emotion(bth, DEV, m, trans_emotion_inf, mp, topk=6)
    tags_h, probs_h = recognize_emotion(bth, DEV, m, lambda im: trans_emotion_inf(im), mp, topk=6)
    assert [np.shape(t) for t in tags_d] == [(2, 6), (0,), (1, 6), (3, 6)]
    for td, th, pd_, ph in zip(tags_d, tags_h, probs_d, probs_h):
        assert np.array_equal(np.asarray(td), np.asarray(th))
        assert np.shape(pd_) == np.shape(ph) and (len(pd_) == 0 or np.abs(np.asarray(pd_) - np.asarray(ph)).max() <= 1e-5)
    assert all(t in names for t in np.asarray(tags_d[3]).ravel())
    assert recognize_emotion([[], []], DEV, m, trans_emotion_inf, mp) == ([[], []], [[], []])
    # logits of the resident path are the network on the host transform
    d = torch.from_numpy(np.stack(f[:3])).to(DEV)
    idx, prob, logits = m.recognize(d, 6, want_logits=True)
    want, _ = m(torch.stack([trans_emotion_inf(a) for a in f[:3]]).to(DEV))
    assert (_rel(logits.cpu().numpy(), want.cpu().numpy()) <= 1e-6).all()


def test_face_pipeline_with_emotion_model():
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.pipeline import (FacePipeline, center_point_dict, parallel_detect_and_align,
                                                        recognize_emotion, trans_emotion_inf)
    a = load_image("mrDam_HaHo_recog.jpg")
    frames = torch.from_numpy(np.stack([a, np.ascontiguousarray(a[:, ::-1])])).to(DEV)
    det = models.MTCNN(keep_all=True, min_face_size=50, device=DEV, max_batch=2, max_height=a.shape[0], max_width=a.shape[1])
    enc = models.InceptionResnetV1(pretrained=None, max_batch=16).to(DEV).eval()
    clf = models.MLPModel(512, 1001).to(DEV).eval()
    l2n = {"label": list(range(1001)), "name": ["c%d" % i for i in range(1001)]}
    emo = _model("f16x2", max_batch=4)
    plain = FacePipeline(det, enc, clf, l2n, 160, 0.0)
    withe = FacePipeline(det, enc, clf, l2n, 160, 0.0, embed_batch=8, embed_lanes=2, emotion=emo, topk_emotions=6)
    assert withe.embed_batch == 0 and withe.embed_lanes == 1      # one buffer set in the emotion handle: one lane
    t0, t1 = plain.submit(frames), withe.submit(frames)
    c0, b0, e0, a0, p0 = t0.result()
    c1, b1, e1, a1, p1 = t1.result()
    assert t0.emo_idx is None and c0 == c1 == [2, 2] and np.array_equal(b0, b1)
    assert torch.equal(e0, e1) and torch.equal(a0, a1) and torch.equal(p0, p1)
    assert tuple(t1.emo_idx.shape) == (4, 6) and t1.emo_idx.dtype == torch.int32 and tuple(t1.emo_prob.shape) == (4, 6)
    faces, _ = parallel_detect_and_align([a, np.ascontiguousarray(a[:, ::-1])], det, center_point_dict["(160, 160)"], (160, 160))
    tags, probs = recognize_emotion(faces, DEV, emo, trans_emotion_inf, np.vectorize(lambda i: int(i)), topk=6)
    assert np.array_equal(np.concatenate([np.asarray(t) for t in tags]), t1.emo_idx.cpu().numpy())
    assert np.abs(np.concatenate([np.asarray(p) for p in probs]) - t1.emo_prob.cpu().numpy()).max() <= 1e-6
    blank = withe.submit(torch.zeros_like(frames[:1]))
    assert blank.result()[0] == [0] and tuple(blank.emo_idx.shape) == (0, 6)
    torch.cuda.synchronize()


def test_demo_image_cli_recog_emotion(tmp_path):
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    import pickle
    ck = str(tmp_path / "model_best.pth")
    torch.save({"arch": "MLPModel", "epoch": 3, "state_dict": generate_state_dict("mlp", 0, as_torch=True, num_classes=1001),
                "optimizer": {}, "monitor_best": 0.1, "config": {}}, ck)
    l2n = str(tmp_path / "label2name.csv")
    with open(l2n, "w") as f:
        f.write("label,name\n" + "".join("%d,celeb_%d\n" % (i, i) for i in range(0, 1001, 2)))
    eck = str(tmp_path / "emotion.pth")
    torch.save({"epoch": 9, "state_dict": {"module." + k: v for k, v in _sd().items()}}, eck)
    eargs = str(tmp_path / "emotion.json")
    with open(eargs, "w") as f:
        json.dump({"pretrained": False, "num_classes": NC, "checkpoint_path": eck, "max_batch": 8}, f)
    names = json.load(open(os.path.join(GOLDEN, "etag2idx.json")))["idx2key"]
    t2i = str(tmp_path / "etag2idx.pkl.keep")
    with open(t2i, "wb") as f:
        pickle.dump({"key2idx": {n: i for i, n in enumerate(names)}, "idx2key": dict(enumerate(names))}, f)
    out_png = str(tmp_path / "demo_recognition.png")
    args = [os.path.join(REPO, "demo_image.py"), "-i", os.path.join(GOLDEN, "images", "mrDam_HaHo_recog.jpg"), "-o", out_png,
            "-m", ck, "-l2n", l2n, "-enc", "InceptionResnetV1", "-eargs", os.path.join(REPO, "cfg/embedding/inception_resnet_v1.json"),
            "-dargs", os.path.join(REPO, "cfg/detection/mtcnn.json"), "-tg_fs", "160", "--inference_method", "par_fd_vs_aln",
            "--recog_emotion", "-emtargs", eargs, "-t2i", t2i, "--topk_emotions", "6"]
    r = subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Loaded emotion model from checkpoint path" in r.stdout and "Face recognized image saved at" in r.stdout
    assert os.path.exists(out_png)
    lines = [l for l in r.stdout.splitlines() if l.count(" - ") == 6 and l.count("%") == 6]
    assert len(lines) == 2, r.stdout                     # the picture's two faces, six tags each
    for l in lines:
        tags = [p.split(" - ")[0] for p in l.split(": ", 1)[1].split(", ")]
        assert len(tags) == 6 and all(t in names for t in tags)
    # the video CLIs still refuse the switch, naming the limitation
    r = subprocess.run([sys.executable, os.path.join(REPO, "demo_video.py"), "-i", str(tmp_path), "--recog_emotion", "-m", ck, "-l2n", l2n,
                        "--inference_method", "par_fd_vs_aln"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "demo_image.py only" in (r.stdout + r.stderr)
