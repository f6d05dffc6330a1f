"""GPU: vnf_logits_eval against torch on the CPU, the encoders' classification heads against the reference golden
(tools/make_heads_golden.py) and the batch behaviour of a headed handle."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, seeded_normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("logp", "amax", "prob", "nll", "hit", "sums")

# relative L2 per row of the log-probabilities against the reference golden, measured on the MI355X (worst of the
# golden's two rows); the test bounds are twice these, capped by what the project accepts for the dtypes on IRv1
MEASURED = {
    ("irv1_7", "bf16"): 3.35e-3,      # rows 1.64e-3 3.35e-3 -> bound 6.7e-3 (cap 6e-2)
    ("irv1_7", "f16"): 5.86e-4,       # rows 5.86e-4 4.13e-4 -> bound 1.2e-3 (cap 8e-3)
    ("irv1_8631", "bf16"): 1.34e-3,   # rows 1.34e-3 1.28e-3 -> bound 2.7e-3 (cap 6e-2)
    ("irv1_8631", "f16"): 1.53e-4,    # rows 1.46e-4 1.53e-4 -> bound 3.1e-4 (cap 8e-3)
}
CAP = {"bf16": 6e-2, "f16": 8e-3}


# ------------------------------------------------------------------------------------------------ vnf_logits_eval
def _logits(n, c, seed):
    """Seeded logits x5; one row with three exact ties at its maximum, another with a tie 64 columns apart."""
    x = (seeded_normal((n, c), seed) * 5.0).numpy()
    r3 = 1 if n > 1 else 0
    if c >= 3:
        x[r3, sorted({c // 3, c // 2, c - 1})] = x[r3].max() + 1.0
    if c >= 65 and n > 3:
        j = min(5, c - 65)
        x[3, [j, j + 64]] = x[3].max() + 0.5
    return x


def _want(x, t):
    lp = F.log_softmax(torch.from_numpy(x), dim=1).numpy()
    amax = np.argmax(x, axis=1).astype(np.int32)          # first occurrence
    rows = np.arange(x.shape[0])
    return {"logp": lp, "amax": amax, "prob": np.exp(lp[rows, amax]), "nll": -lp[rows, t], "hit": (amax == t).astype(np.int32)}


def _seq_sum(v):
    acc = np.float32(0.0)
    for e in np.asarray(v, dtype=np.float32):
        acc = np.float32(acc + e)
    return acc


@pytest.mark.parametrize("c", [1, 7, 64, 65, 1000, 8631])
def test_logits_eval_matches_torch(c):
    from vn_celeb_face_recognition_amd.classifier import logits_eval
    for n in (1, 5, 37):
        x = _logits(n, c, 100 + n)
        rng = np.random.default_rng(c * 64 + n)
        t = rng.integers(0, c, size=n)
        t[::2] = np.argmax(x, axis=1)[::2]               # some hits for sure
        want = _want(x, t)
        for pad in (0, 9):
            base = torch.full((n, c + pad), 1e30, dtype=torch.float32)      # the padding must never be read
            base[:, :c] = torch.from_numpy(x)
            xd = base.to(DEV)[:, :c]
            assert pad == 0 or (xd.stride(0) == c + 9 and not xd.is_contiguous()) or n == 1
            got = {k: v.cpu().numpy() for k, v in logits_eval(xd, t, want=ALL).items()}
            again = {k: v.cpu().numpy() for k, v in logits_eval(xd, t, want=ALL).items()}
            tag = "n=%d C=%d ld=%d" % (n, c, c + pad)
            assert np.array_equal(got["amax"], want["amax"]), tag
            assert np.array_equal(got["hit"], want["hit"]) and got["hit"].sum() >= (n + 1) // 2, tag
            for k in ("logp", "nll", "prob"):
                tol = 1e-6 * max(1.0, float(np.abs(want[k]).max()))
                err = float(np.abs(got[k] - want[k]).max())
                print("%s %-4s max abs err %.3e (tol %.3e)" % (tag, k, err, tol))
                assert got[k].shape == want[k].shape and err <= tol, (tag, k, err, tol)
            # the sums: the fp32 sum of the returned rows in index order, bit for bit; and the same bits again
            assert got["sums"].dtype == np.float32 and got["sums"].shape == (2,)
            assert got["sums"][0].tobytes() == _seq_sum(got["nll"]).tobytes(), (tag, got["sums"][0], _seq_sum(got["nll"]))
            assert got["sums"][1] == np.float32(got["hit"].sum()), tag
            for k in ALL:
                assert got[k].tobytes() == again[k].tobytes(), (tag, k)


def test_logits_eval_every_output_is_optional():
    from vn_celeb_face_recognition_amd.classifier import logits_eval
    n, c = 37, 65
    x = torch.from_numpy(_logits(n, c, 7)).to(DEV)
    t = np.random.default_rng(3).integers(0, c, size=n)
    full = {k: v.cpu() for k, v in logits_eval(x, t, want=ALL).items()}
    for k in ALL:
        one = logits_eval(x, t, want=(k,))
        assert list(one) == [k] and torch.equal(one[k].cpu(), full[k]), k
    # sums without the rows they add (the one-workgroup path), with one of them, and without targets at all
    for want in (("sums", "nll"), ("sums", "hit"), ("sums", "logp", "amax")):
        r = logits_eval(x, t, want=want)
        assert all(torch.equal(r[k].cpu(), full[k]) for k in want), want
    r = logits_eval(x, None, want=("logp", "amax", "prob"))
    assert all(torch.equal(r[k].cpu(), full[k]) for k in r)
    assert logits_eval(x, t, want=()) == {}
    with pytest.raises(ValueError, match="need a target"):
        logits_eval(x, None, want=("nll",))


def test_logits_eval_empty_batch_and_raw_argument_checks():
    from vn_celeb_face_recognition_amd import _lib
    from vn_celeb_face_recognition_amd.classifier import logits_eval
    r = logits_eval(torch.empty((0, 7), device=DEV), [], want=ALL)
    assert tuple(r["logp"].shape) == (0, 7) and tuple(r["amax"].shape) == (0,) and r["sums"].tolist() == [0.0, 0.0]
    lib = _lib.load()
    x = torch.zeros((2, 8), device=DEV)
    out = torch.zeros((2,), device=DEV)
    s = _lib.current_stream_ptr()
    p = lambda a: ctypes.c_void_p(a.data_ptr())   # noqa: E731
    assert lib.vnf_logits_eval(None, 0, 8, 8, None, None, None, None, None, None, None, s) == 0          # n == 0: no-op
    assert lib.vnf_logits_eval(p(x), 2, 8, 7, None, None, None, p(out), None, None, None, s) == -1        # ld < c
    assert lib.vnf_logits_eval(p(x), 2, 0, 8, None, None, None, p(out), None, None, None, s) == -1        # c < 1
    assert lib.vnf_logits_eval(p(x), 2, 8, 8, None, None, None, None, p(out), None, None, s) == -1        # nll without target
    assert b"target" in lib.vnf_last_error()
    assert lib.vnf_logits_eval(None, 2, 8, 8, None, None, None, p(out), None, None, None, s) == -1        # no logits
    torch.cuda.synchronize()


def test_logits_eval_large_logits_do_not_overflow():
    from vn_celeb_face_recognition_amd.classifier import logits_eval
    x = np.array([[3e4, 3e4 - 2.0, -3e4, 0.0], [-1e30, -1e30, -1e30, -1e30]], dtype=np.float32)
    r = logits_eval(torch.from_numpy(x).to(DEV), [1, 3], want=ALL)
    want = _want(x, np.array([1, 3]))
    assert np.isfinite(r["logp"][0, :2].cpu().numpy()).all() and r["amax"].tolist() == [0, 0] and r["hit"].tolist() == [0, 0]
    assert np.allclose(r["nll"].cpu().numpy(), want["nll"], rtol=1e-6, atol=1e-6)
    assert np.allclose(r["prob"].cpu().numpy(), want["prob"], rtol=1e-6)


# ------------------------------------------------------------------------------------------------ golden heads
def _golden(key):
    g = np.load(os.path.join(GOLDEN, "heads_ref.npz"))
    return {k: g[key + "/" + k] for k in ("input_seed", "logp", "argmax", "prob")}


_MODELS = {}


def _model(key, dt, max_batch=2):
    from vn_celeb_face_recognition_amd import models
    if (key, dt, max_batch) not in _MODELS:
        arch, c = key.split("_")
        if arch == "irv1":
            m = models.InceptionResnetV1(pretrained=None, classify=True, num_classes=int(c), compute_dtype=dt, max_batch=max_batch)
        else:
            m = models.iresnet100(n_classes=int(c), freeze_weights=True, compute_dtype=dt, max_batch=max_batch)
        _MODELS[(key, dt, max_batch)] = m.to(DEV).eval()
    return _MODELS[(key, dt, max_batch)]


def _run(key, dt):
    g = _golden(key)
    m = _model(key, dt)
    s = m.input_size
    x = seeded_normal((2, 3, s, s), int(g["input_seed"])).to(DEV)
    logp, amax, prob = m.logprobs(x)
    assert logp.is_cuda and logp.dtype == torch.float32 and tuple(logp.shape) == g["logp"].shape
    assert amax.dtype == torch.int32 and prob.dtype == torch.float32
    assert torch.equal(m(x), logp)                      # __call__ returns the log-probabilities
    return g, logp.cpu().numpy(), amax.cpu().numpy(), prob.cpu().numpy()


@pytest.mark.parametrize("key,dt", [("irv1_7", "f32"), ("irv1_7", "f16x2"), ("irv1_8631", "f32"), ("irv1_8631", "f16x2"),
                                    ("ir100_1020", "f32")])
def test_head_matches_reference_golden(key, dt):
    g, logp, amax, prob = _run(key, dt)
    tol = 1e-4 * max(1.0, float(np.abs(g["logp"]).max()))
    err = float(np.abs(logp - g["logp"]).max())
    perr = float(np.abs(prob - g["prob"]).max())
    print("%s %s: max |logp - golden| %.3e (tol %.3e), max prob err %.3e, argmax %s" % (key, dt, err, tol, perr, amax.tolist()))
    assert err <= tol, (err, tol)
    assert np.array_equal(amax, g["argmax"])
    assert perr <= 1e-4


@pytest.mark.parametrize("key,dt", sorted(MEASURED))
def test_head_16bit_dtypes_against_golden(key, dt):
    g, logp, amax, prob = _run(key, dt)
    rel = np.linalg.norm(logp - g["logp"], axis=1) / np.linalg.norm(g["logp"], axis=1)
    bound = min(2 * MEASURED[(key, dt)], CAP[dt])
    print("%s %s: rel L2 per row %s (bound %.3e)" % (key, dt, rel, bound))
    assert rel.max() <= bound, (rel, bound)
    assert np.array_equal(amax, g["argmax"])


# ------------------------------------------------------------------------------------------------ behaviour
def test_chunks_rows_empty_batch_and_embeddings():
    from vn_celeb_face_recognition_amd import models
    m = _model("irv1_7", "f16x2", max_batch=2)
    x = seeded_normal((5, 3, 160, 160), 31).to(DEV)
    logp, amax, prob = m.logprobs(x)                    # chunks of 2, 2 and 1
    assert tuple(logp.shape) == (5, 7) and tuple(amax.shape) == (5,) and tuple(prob.shape) == (5,)
    for i in range(5):
        one, a1, p1 = m.logprobs(x[i:i + 1])
        tol = 1e-6 * max(1.0, float(one.abs().max()))
        assert float((logp[i] - one[0]).abs().max()) <= tol, i
        assert int(a1[0]) == int(amax[i]) and abs(float(p1[0]) - float(prob[i])) <= 1e-6
    assert torch.equal(amax.long(), logp.argmax(dim=1)) and torch.allclose(prob, logp.max(dim=1).values.exp(), rtol=1e-6)
    assert torch.allclose(logp.exp().sum(dim=1), torch.ones(5, device=DEV), atol=1e-5)
    e = m.logprobs(x[:0])
    assert tuple(e[0].shape) == (0, 7) and tuple(m(x[:0]).shape) == (0, 7)
    with pytest.raises(ValueError):
        m(x[:, :, :150])
    with pytest.raises(RuntimeError, match="cuda"):
        m(x.cpu())
    # the embeddings of the headed handle are those of a head-less encoder of the same weights and dtype
    plain = models.InceptionResnetV1(pretrained=None, compute_dtype="f16x2", max_batch=2).to(DEV).eval()
    emb = m.embed(x)
    assert tuple(emb.shape) == (5, 512) and torch.equal(emb, plain(x))
    assert torch.equal(m.logprobs(x)[0], logp)           # and vnf_embed in between left the head's path as it was


def test_raw_abi_capacity_and_headless_handle():
    from vn_celeb_face_recognition_amd import _lib, models
    lib = _lib.load()
    m = _model("irv1_7", "f16x2", max_batch=2)
    x = seeded_normal((3, 3, 160, 160), 5).to(DEV)
    logp = torch.empty((3, 7), device=DEV)
    args = (ctypes.c_void_p(x.data_ptr()), 3, _lib.VNF_F32, ctypes.c_void_p(logp.data_ptr()), None, None, _lib.current_stream_ptr())
    assert lib.vnf_encoder_logprobs(m._ensure_handle(), *args) == -4          # VNF_E_CAPACITY
    assert lib.vnf_encoder_logprobs(m._ensure_handle(), None, 0, _lib.VNF_F32, None, None, None, _lib.current_stream_ptr()) == 0
    plain = models.InceptionResnetV1(pretrained=None, compute_dtype="f16x2", max_batch=4).to(DEV).eval()
    assert lib.vnf_encoder_logprobs(plain._ensure_handle(), *args) == -1      # VNF_E_INVALID: no head
    assert b"head" in lib.vnf_last_error()
    # weights without logits.* cannot make a headed handle: VNF_E_MISSING names the tensor
    descs, n, keep = _lib.make_descs(plain.state_dict())
    h = ctypes.c_void_p()
    assert lib.vnf_encoder_create_classifier(_lib.VNF_ARCH_IRV1, descs, n, _lib.VNF_F16X2, 2, 7, ctypes.byref(h)) == -2
    assert b"logits.weight" in lib.vnf_last_error() and not h.value
    torch.cuda.synchronize()
