"""mixed_6a branch 1 in one launch (mixed6a_chain_kernel, bit 7 of VNF_FUSE) against the three plan convolutions it
replaces: branch1.0 (1x1 256 -> 192), branch1.1 (3x3 pad 1) and branch1.2 (3x3 stride 2, to channels 384..639 of the 8 x 8
mixed_6a output).  The kernel uses the plan's MFMA, k order, epilogue and rounding points, so every tensor behind it must be
the same bytes: no comparison here has a tolerance.

A workgroup owns one 17 x 17 image, so the image shape is fixed by the network and the cases are small batches: n = 1, 2
and 5 on max_batch = 5 handles.  Inputs are seeded N(0,1) crops in the compute dtype.  Every element of the tap is compared:
a lost border tap, a padding pixel row read as a neighbour or a wrong stride-2 gather changes channels 384..639 of it, a
store outside the kernel's range the others.

The switches are read when a handle is created, so each form is a model of its own from the same seeded state dict, with the
heuristic tiles (VNF_AUTOTUNE=0: quick creates).  One handle per (dtype, switch) serves every case of this file; the case
that is about what an earlier call left behind says in which order it calls it."""
import os

import numpy as np
import pytest
import torch

from conftest import seeded_normal

pytestmark = pytest.mark.gpu

CROPS = {"bf16": torch.bfloat16, "f16": torch.float16, "f16x2": torch.float32}
MAX_N = 5
C0, C1 = 384, 640          # the kernel's channel range of the mixed_6a output
_models = {}
_inputs = {}
_runs = {}


def _model(dt, fuse):
    """The max_batch = 5 model of (dtype, VNF_FUSE); fuse None: the default switch."""
    key = (dt, fuse)
    if key not in _models:
        from vn_celeb_face_recognition_amd.models import InceptionResnetV1
        keep = {k: os.environ.get(k) for k in ("VNF_FUSE", "VNF_AUTOTUNE")}
        os.environ["VNF_AUTOTUNE"] = "0"
        if fuse is None:
            os.environ.pop("VNF_FUSE", None)
        else:
            os.environ["VNF_FUSE"] = str(fuse)
        try:
            m = InceptionResnetV1(pretrained=None, device="cuda:0", compute_dtype=dt, max_batch=MAX_N).eval()
            m._ensure_handle()                           # the handle reads the switches here
        finally:
            for k, v in keep.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        _models[key] = m
    return _models[key]


def _x(dt, n):
    """The first n of the 5 seeded crops of a dtype (image i is the same tensor at every batch size)."""
    if dt not in _inputs:
        _inputs[dt] = seeded_normal((MAX_N, 3, 160, 160), 606).to(CROPS[dt]).cuda()
    return _inputs[dt][:n].contiguous()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _embed(m, x):
    return _bits(m(x).cpu().numpy())


def _run(dt, fuse, n):
    """Embedding and the two taps of the first n crops under a switch, computed once per (dtype, switch, n)."""
    key = (dt, fuse, n)
    if key not in _runs:
        m = _model(dt, fuse)
        emb = _embed(m, _x(dt, n))
        _runs[key] = (emb, _bits(m.tap("mixed_6a", n)), _bits(m.tap("repeat_2", n)))
    return _runs[key]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d elements differ, the first at" % len(bad), bad[:4].tolist())


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_chain_kernel_is_bitwise_the_three_plan_convolutions(dt, n):
    emb, m6, r2 = _run(dt, 128, n)
    want_emb, want_m6, want_r2 = _run(dt, 0, n)
    assert m6.shape == (n, 896, 8, 8)
    own = m6[:, C0:C1].view(np.float32)
    assert np.isfinite(own).all() and (own > 0).any(), (dt, n)
    _same(m6[:, C0:C1], want_m6[:, C0:C1], (dt, n, "mixed_6a channels 384..639"))
    _same(r2, want_r2, (dt, n, "repeat_2"))
    assert np.isfinite(emb.view(np.float32)).all()
    _same(emb, want_emb, (dt, n, "embedding"))


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_chain_kernel_writes_nothing_outside_its_channel_range(dt, n):
    m6, want_m6 = _run(dt, 128, n)[1], _run(dt, 0, n)[1]
    _same(m6[:, :C0], want_m6[:, :C0], (dt, n, "mixed_6a channels 0..383 (branch0)"))
    _same(m6[:, C1:], want_m6[:, C1:], (dt, n, "mixed_6a channels 640..895 (max pool)"))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_default_switch_embeds_like_the_switch_without_bit_7(dt):
    got = _embed(_model(dt, None), _x(dt, 5))
    want = _embed(_model(dt, 95), _x(dt, 5))
    assert np.isfinite(got.view(np.float32)).all() and got.any()
    _same(got, want, (dt, "embedding"))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rows_an_earlier_larger_batch_left_behind_do_not_reach_a_smaller_one(dt):
    """n = 5 fills every row of the handle's buffers; the n = 2 call behind it finds images 2..4 of the earlier batch
    behind its own."""
    m = _model(dt, 128)
    _embed(m, _x(dt, 5))
    emb = _embed(m, _x(dt, 2))
    m6, r2 = _bits(m.tap("mixed_6a", 2)), _bits(m.tap("repeat_2", 2))
    want_emb, want_m6, want_r2 = _run(dt, 0, 2)
    _same(m6, want_m6, (dt, "mixed_6a"))
    _same(r2, want_r2, (dt, "repeat_2"))
    _same(emb, want_emb, (dt, "embedding"))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_an_image_embeds_the_same_alone_as_at_every_position_of_a_batch(dt):
    m = _model(dt, 128)
    x = _x(dt, 5)
    batch = _embed(m, x)
    for i in range(5):
        alone = _embed(m, x[i:i + 1].contiguous())
        assert np.array_equal(alone[0], batch[i]), (dt, i)


def _rows(m, x):
    """The label column of the profile's mixed_6a rows and of the Block35 stack's row."""
    rows = []
    for line in m.profile(x).splitlines():
        if "mixed_6a" in line:
            rows.append(line.rstrip())
    return rows


def test_profile_rows_follow_the_switch_and_the_dtype():
    for dt in ("bf16", "f16"):
        rows = _rows(_model(dt, None), _x(dt, 5))
        labels = [r[:28].strip() for r in rows]
        assert len([l for l in labels if "chain" in l]) == 1, rows
        assert [l for l in labels if "chain" in l][0].startswith("mixed_6a.branch1.0"), rows
        assert not [l for l in labels if l.endswith("branch1.1") or l.endswith("branch1.2")], rows
        assert labels.count("mixed_6a.branch0") == 1, rows
        assert not [r for r in rows if "+ mixed_6a.branch1.0 in one launch" in r], rows
    for m, dt in ((_model("f16x2", None), "f16x2"), (_model("bf16", 0), "bf16")):
        rows = _rows(m, _x(dt, 5))
        labels = [r[:28].strip() for r in rows]
        assert not [r for r in rows if "chain" in r], rows
        for part in ("branch1.0", "branch1.1", "branch1.2", "branch0"):
            assert labels.count("mixed_6a." + part) == 1, (part, rows)
    rows = _rows(_model("bf16", 255), _x("bf16", 5))
    labels = [r[:28].strip() for r in rows]
    assert len([r for r in rows if "+ mixed_6a.branch1.0 in one launch" in r]) == 1, rows
    assert not [r for r in rows if "chain" in r], rows
    assert "mixed_6a.branch1.0" not in labels, rows
    i = [k for k, r in enumerate(rows) if "+ mixed_6a.branch1.0 in one launch" in r][0]
    assert labels[i + 1:i + 3] == ["mixed_6a.branch1.1", "mixed_6a.branch1.2"], rows


def test_flops_per_image_do_not_depend_on_the_switch():
    want = _model("bf16", 0).flops_per_image()
    assert _model("bf16", None).flops_per_image() == want
    assert _model("bf16", 95).flops_per_image() == want
    assert _model("bf16", 223).flops_per_image() == want
