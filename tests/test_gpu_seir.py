"""GPU: the SE-IR ResNet-101 encoder (models.resnet101(use_se=True)) against the reference's golden and the functional
restatement, its squeeze-and-excitation kernels at their own shapes (vnf_se_block) against torch on the CPU, and the two
CLIs that take the encoder from the plugin registry."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO, load_image, seeded_normal
from conv_reference import from_planar as _from_planar, to_planar as _to_planar
from seir_restatement import seir101_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PNGS = ["041bc30432964f95871d4c223eba8f7c.png", "318c7ec3b94b451c813a5665cfcfbda3.png", "33f2891da9694198a67aabd1660517c3.png"]
TAPS = ("conv1", "stem", "layer1", "layer2", "layer3", "layer4", "bn3")
# embedding L2 error against the reference golden, measured on MI355X (both rows of the golden; the larger)
MEASURED_BF16 = 1.05e-2
MEASURED_F16 = 1.31e-3

_models = {}


def _model(dt):
    """One handle per compute dtype for the whole module (max_batch 3)."""
    from vn_celeb_face_recognition_amd import models
    if dt not in _models:
        _models[dt] = models.resnet101(use_se=True, compute_dtype=dt, max_batch=3).to(DEV).eval()
    return _models[dt]


def _sd():
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    return generate_state_dict("seir101", 0, as_torch=True)


@pytest.fixture(scope="module")
def ref():
    """(golden, the two golden inputs + one more seeded image, restatement taps of the golden inputs): computed once."""
    g = np.load(os.path.join(GOLDEN, "seir101_seed0.npz"))
    x = torch.cat([seeded_normal((2, 3, 112, 112), int(g["input_seed"])), seeded_normal((1, 3, 112, 112), 77)])
    taps = {}
    y = seir101_forward(_sd(), x[:2], taps=taps).numpy()
    assert np.linalg.norm(y - g["features"], axis=1).max() <= 1e-5
    return g, x, taps


@pytest.mark.parametrize("dt", ["f32", "f16x2"])
def test_embedding_matches_reference_golden_1e4(ref, dt):
    """The exact-f32 and the split-f16 plans against embeddings the reference itself produced: L2 error <= 1e-4."""
    g, x, _ = ref
    y = _model(dt)(x[:2].to(DEV)).cpu().numpy()
    err = np.linalg.norm(y - g["features"], axis=1)
    print("seir101 %s: L2 error vs reference golden %s" % (dt, err))
    assert y.shape == (2, 512) and err.max() <= 1e-4, err
    assert np.allclose(np.linalg.norm(y, axis=1), 1.0, atol=1e-5)


def test_f32_stage_taps_match_restatement(ref):
    _, x, want = ref
    m = _model("f32")
    m(x[:2].to(DEV))
    for name in TAPS:
        got, w = m.tap(name, 2), want[name].numpy()
        got = got.reshape(w.shape) if name == "bn3" else got
        assert got.shape == w.shape, (name, got.shape, w.shape)
        err, tol = float(np.abs(got - w).max()), 1e-4 * max(1.0, float(np.abs(w).max()))
        print("tap %-7s max abs err %.3e (tol %.3e, max |want| %.3f)" % (name, err, tol, np.abs(w).max()))
        assert err <= tol, (name, err)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f16x2"])
def test_stem_maxpool_is_exact_in_every_layout(ref, dt):
    """nn.MaxPool2d(2, 2) (resnet_encoder.py:163) moves values and rounds nothing: 110 -> 55, bit for bit torch's pool of
    the handle's own conv1 tap, in every storage layout."""
    _, x, _ = ref
    m = _model(dt)
    m(x.to(DEV))
    got, want = m.tap("stem", 3), F.max_pool2d(torch.from_numpy(m.tap("conv1", 3)), 2, 2).numpy()
    assert got.shape == want.shape == (3, 64, 55, 55) and np.abs(want).max() > 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dt", ["bf16", "f16x2"])
def test_rows_do_not_depend_on_the_batch_around_them(ref, dt):
    """Eval-mode BatchNorm and a per-image SE gate: a row embedded alone is bit for bit the row inside a batch of 3;
    batches beyond max_batch are cut by the wrapper, the empty batch works, another input size is refused."""
    _, x, _ = ref
    m = _model(dt)
    xd = x.to(DEV)
    y3 = m(xd)
    for i in range(3):
        assert torch.equal(m(xd[i:i + 1])[0], y3[i]), i
    y5 = m(torch.cat([xd, xd[:2]]))
    assert y5.shape == (5, 512) and torch.equal(y5[:3], y3) and torch.equal(y5[3:], y3[:2])
    assert m(xd[:0]).shape == (0, 512)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 160, 160, device=DEV))


@pytest.mark.parametrize("dt,measured,cap", [("bf16", MEASURED_BF16, 6e-2), ("f16", MEASURED_F16, 8e-3)])
def test_16bit_dtypes_against_golden(ref, dt, measured, cap):
    """16-bit storage, fp32 accumulation.  Embedding L2 error against the reference golden measured on MI355X, per row:
    bf16 1.050e-2 / 0.996e-2, f16 1.312e-3 / 1.309e-3 (MEASURED_BF16 / MEASURED_F16 above).  The run is deterministic; the
    bar is twice the measured value (room for other inputs), never above what the project states for these dtypes."""
    g, x, _ = ref
    y = _model(dt)(x[:2].to(DEV)).cpu().numpy()
    err = np.linalg.norm(y - g["features"], axis=1)
    print("seir101 %s: L2 error vs reference golden %s" % (dt, err))
    assert measured is not None, "no measured value recorded for %s" % dt
    assert err.max() <= min(2 * measured, cap), (err, measured)
    assert (y * g["features"]).sum(axis=1).min() >= 0.998


def test_classifier_head_is_refused():
    """The reference's network has no `logits` layer: vnf_encoder_create_classifier says so for this arch."""
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    descs, n, keep = _lib.make_descs({"conv1.weight": np.zeros((64, 3, 3, 3), np.float32)})
    h = ctypes.c_void_p()
    rc = lib.vnf_encoder_create_classifier(_lib.VNF_ARCH_SEIR101, descs, n, _lib.VNF_F32, 1, 7, ctypes.byref(h))
    assert rc != 0 and not h.value and b"logits" in lib.vnf_last_error()


def test_flops_and_profile_name_the_se_ops(ref):
    _, x, _ = ref
    m = _model("bf16")
    alg, exe = m.flops_per_image()
    assert 1.4e10 < alg < 1.6e10 and exe >= alg          # ~7.5 GMAC of convolutions per image
    rep = m.profile(x.to(DEV))
    se = [ln for ln in rep.splitlines() if ".se " in ln]
    assert len(se) == 33 and all("TB/s" in ln for ln in se) and "TOTAL" in rep


# ------------------------------------------------------------------------------------------------ vnf_se_block
def _se_call(t, res, code, planar, n, h, w, c, wts, slope_se, slope_out):
    from vn_celeb_face_recognition_amd import _lib
    y = torch.empty_like(t)
    p = [ctypes.c_void_p(a.data_ptr()) for a in wts]
    _lib.check(_lib.load().vnf_se_block(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(res.data_ptr()), code, planar, n, h, w, c,
                                        p[0], p[1], slope_se, p[2], p[3], slope_out, ctypes.c_void_p(y.data_ptr()),
                                        _lib.current_stream_ptr()))
    return y


def _ordered16(t):   # 16-bit floats as integers in value order: neighbours differ by 1
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


@pytest.mark.parametrize("shape", [(1, 7, 7, 512), (3, 55, 55, 64), (2, 14, 14, 256), (2, 28, 28, 128)])
def test_se_block_kernels_all_layouts(shape):
    """y = prelu(t * gate + res), gate = sigmoid(W2 . prelu(W1 . mean_hw(t) + b1) + b2), at the four stage shapes of the
    network in the four storage layouts, against torch on the CPU in float64 on the STORED inputs (t and res as the layout
    holds them).  The kernels work in fp32: their result may differ from the exact one by 1e-6 of the magnitude of the
    sum's terms |t * gate| + |res| (that is 1e-6 relative wherever nothing cancels) -- the f32 bar.  The 16-bit layouts and
    the split-f16 pairs (22 bits: one unit = max(2^-21 |y|, 2^-24)) round that once more: one unit in the last place of
    the storage type on top, since a gate that differs in its last fp32 bit may round a product the other way.
    Two calls repeat bit for bit, and image 0 alone gives the bits it has inside the batch."""
    from vn_celeb_face_recognition_amd import _lib
    n, H, W, C = shape
    R = C // 16
    g = torch.Generator().manual_seed(C + H)
    t32 = torch.randn(shape, generator=g) + 0.5 * torch.randn((n, 1, 1, C), generator=g)   # per-image channel means
    r32 = torch.randn(shape, generator=g)
    # the two linear layers as the reference initialises them (xavier_normal_, resnet_encoder.py:183-185), so that the
    # gate's logit is a sum of O(1) terms and its fp32 evaluation is good to fp32's own precision (an fp32 dot product is
    # only as exact as the magnitudes it adds up); the biases are drawn non-zero, b2 wide: gates spread over (0,1)
    xav = (2.0 / (C + R)) ** 0.5
    w1 = torch.randn((R, C), generator=g) * xav
    b1 = torch.randn((R,), generator=g) * 0.05
    w2 = torch.randn((C, R), generator=g) * xav
    b2 = torch.randn((C,), generator=g) * 1.5
    slope_se, slope_out = 0.25, 0.2
    wts = [a.to(DEV) for a in (w1, b1, w2, b2)]

    def want(t, r):   # float64 on the stored values
        t, r = t.double(), r.double()
        y = F.prelu(F.linear(t.mean(dim=(1, 2)), w1.double(), b1.double()), torch.tensor([slope_se], dtype=torch.float64))
        gate = torch.sigmoid(F.linear(y, w2.double(), b2.double()))[:, None, None, :]
        out = F.prelu(t * gate + r, torch.tensor([slope_out], dtype=torch.float64))
        return out, 1e-6 * ((t * gate).abs() + r.abs())
    for name, code, tdt in (("f32", _lib.VNF_F32, torch.float32), ("bf16", _lib.VNF_BF16, torch.bfloat16), ("f16", _lib.VNF_F16, torch.float16)):
        ts, rs = t32.to(tdt), r32.to(tdt)
        y = _se_call(ts.to(DEV), rs.to(DEV), code, 0, n, H, W, C, wts, slope_se, slope_out)
        y2 = _se_call(ts.to(DEV), rs.to(DEV), code, 0, n, H, W, C, wts, slope_se, slope_out)
        y0 = _se_call(ts[:1].to(DEV), rs[:1].to(DEV), code, 0, 1, H, W, C, wts, slope_se, slope_out)
        assert torch.equal(y.view(torch.int16 if tdt != torch.float32 else torch.int32), y2.view(torch.int16 if tdt != torch.float32 else torch.int32))
        assert torch.equal(y0[0], y[0])
        w, f32_term = want(ts, rs)
        got = y.cpu()
        assert torch.isfinite(got.float()).all() and got.float().abs().max() > 1
        if tdt == torch.float32:
            excess = ((got.double() - w).abs() - f32_term).max().item()
            print("se %s f32: worst (|err| - bar) %.3e, max |err| %.3e" % (shape, excess, (got.double() - w).abs().max().item()))
            assert excess <= 0
        else:
            # within one storage step of the correctly rounded result, after allowing the fp32 term to move the value
            lo, hi = (w - f32_term).to(tdt), (w + f32_term).to(tdt)
            o = _ordered16(got)
            worst = torch.maximum(_ordered16(lo) - o, o - _ordered16(hi)).max().item()
            print("se %s %s: worst distance outside the fp32 band, in storage steps: %d" % (shape, name, worst))
            assert worst <= 1
    tp, tv = _to_planar(t32)
    rp, rv = _to_planar(r32)
    y = _se_call(tp.to(DEV), rp.to(DEV), _lib.VNF_F16X2, 1, n, H, W, C, wts, slope_se, slope_out)
    y2 = _se_call(tp.to(DEV), rp.to(DEV), _lib.VNF_F16X2, 1, n, H, W, C, wts, slope_se, slope_out)
    y0 = _se_call(tp[:1].to(DEV), rp[:1].to(DEV), _lib.VNF_F16X2, 1, 1, H, W, C, wts, slope_se, slope_out)
    assert torch.equal(y, y2) and torch.equal(y0[0], y[0])
    w, f32_term = want(tv, rv)
    got = _from_planar(y.cpu()).double()
    unit = torch.clamp(w.abs() * 2.0 ** -21, min=2.0 ** -24)
    excess = ((got - w).abs() - f32_term - unit).max().item()
    print("se %s planar split-f16: worst (|err| - bar) %.3e, max |err| %.3e" % (shape, excess, (got - w).abs().max().item()))
    assert excess <= 0
    # interleaved pairs are not a layout of the encoders: refused, as are channel counts the gate layers cannot have
    lib = _lib.load()
    a = ctypes.c_void_p(tp.to(DEV).data_ptr())
    p = [ctypes.c_void_p(x.data_ptr()) for x in wts]
    assert lib.vnf_se_block(a, a, _lib.VNF_F16X2, 0, n, H, W, C, p[0], p[1], 0.25, p[2], p[3], 0.2, a, None) != 0
    assert lib.vnf_se_block(a, a, _lib.VNF_F32, 0, n, H, W, C - 8, p[0], p[1], 0.25, p[2], p[3], 0.2, a, None) != 0


# ------------------------------------------------------------------------------------------------ CLIs
def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_find_embedding_cli_with_the_registry_encoder(tmp_path):
    """find_embedding.py -enc resnet101 -eargs cfg/embedding/resnet101_se.json: <stem>.npz with arr_0 (512,) fp32, within 1e-4
    of the restatement on the crop the CLI cuts (181 x 181 pictures, centre 112 x 112); -bz 2 over three files leaves
    a ragged last batch."""
    d = tmp_path / "data"; d.mkdir()
    for f in PNGS:
        shutil.copy(os.path.join(GOLDEN, "images", f), d / f)
    out = tmp_path / "emb"
    stdout = _run([os.path.join(REPO, "find_embedding.py"), "-d", str(d), "-bz", "2", "-o", str(out), "-dv", "GPU", "-enc", "resnet101",
                   "-eargs", os.path.join(REPO, "cfg", "embedding", "resnet101_se.json")], str(tmp_path))
    assert stdout.count("Save embedding for") == 3
    crops = []
    for f in PNGS:
        a = load_image(f)
        sy, sx = (a.shape[0] - 112) // 2, (a.shape[1] - 112) // 2
        crops.append(((np.float32(a[sy:sy + 112, sx:sx + 112]) - 127.5) / 128).transpose(2, 0, 1))
    want = seir101_forward(_sd(), torch.from_numpy(np.stack(crops))).numpy()
    for f, w in zip(PNGS, want):
        e = np.load(out / (f.split(".")[0] + ".npz"))["arr_0"]
        assert e.shape == (512,) and e.dtype == np.float32
        assert np.linalg.norm(e - w) <= 1e-4, (f, np.linalg.norm(e - w))


def test_demo_image_cli_with_the_registry_encoder(tmp_path):
    """demo_image.py -enc resnet101 -tg_fs 112 exits 0, and the picture it writes is the one drawn from the boxes and
    names of the step-wise path (detect + align at 112 x 112, embed, classify) run here on the same picture."""
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.classifier import load_model_classify
    from vn_celeb_face_recognition_amd.cli_utils import draw_boxes_on_image, read_json, read_label2name, read_rgb
    from vn_celeb_face_recognition_amd.pipeline import center_point_dict, parallel_detect_and_align, recognize_celeb, transforms_default
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    ck = str(tmp_path / "model_best.pth")
    torch.save({"arch": "MLPModel", "epoch": 3, "state_dict": generate_state_dict("mlp", 0, as_torch=True, num_classes=1001),
                "optimizer": {}, "monitor_best": 0.1, "config": {}}, ck)
    l2n = str(tmp_path / "label2name.csv")
    with open(l2n, "w") as f:
        f.write("label,name\n" + "".join("%d,celeb_%d\n" % (i, i) for i in range(0, 1001, 2)))
    src = os.path.join(GOLDEN, "images", "mrDam_HaHo_recog.jpg")
    out_png = str(tmp_path / "demo_recognition.png")
    eargs, dargs = os.path.join(REPO, "cfg", "embedding", "resnet101_se.json"), os.path.join(REPO, "cfg", "detection", "mtcnn.json")
    so = _run([os.path.join(REPO, "demo_image.py"), "-i", src, "-o", out_png, "-m", ck, "-l2n", l2n, "-enc", "resnet101", "-eargs", eargs,
               "-dargs", dargs, "-tg_fs", "112", "--inference_method", "par_fd_vs_aln"], str(tmp_path))
    assert "Face recognized image saved at" in so and os.path.exists(out_png)
    rgb = read_rgb(src)
    det = models.MTCNN(**dict(read_json(dargs), device=DEV)).eval()
    clf = load_model_classify(ck, models.MLPModel(512, 1001)).to(DEV)
    faces, boxes = parallel_detect_and_align([rgb], det, center_point_dict["(112, 112)"], (112, 112))
    names = recognize_celeb(faces, DEV, _model("f16x2"), clf, transforms_default, read_label2name(l2n), 0.0)
    assert len(names[0]) == 2 and all(n.startswith("celeb_") or n == "Unknown" for n in names[0])
    assert np.array_equal(read_rgb(out_png), draw_boxes_on_image(rgb, boxes[0], names[0]))
