"""conv2d_1a from LDS-staged input rows (stem_conv1a_rows_kernel, VNF_STEM1A_MFMA=2, the default) against the two older
forms of the same layer: the f32 MFMA with per-lane gathers (=1) and the packed-FMA VALU kernel (=0).  The staged form
only changes how the B operand reaches the lanes, so the conv2d_1a tensor and every embedding behind it must be the
same bytes -- no tolerance anywhere in this file.

Per compute dtype (bf16 on bf16 crops, f16 on f16 crops, planar split-f16 on fp32 crops) and batch:
  n = 1   one image: 20 bands of 4 output rows, the last with 79 mod 4 = 3 (its fourth wave idles), and the last
          16-pixel group of every row holds 15 pixels; 20 workgroups, one band each;
  n = 3, 5  60 and 100 bands: grids that are a multiple of nothing.
The launcher starts at most 1024 workgroups, so up to 51 images every workgroup has one band.  One more case per crop
width, n = 104 (2080 bands: workgroups take a second band out of the other LDS buffer and 32 of them a third out of the
first again), checks that walk against the gather kernel on the seeded input; it is the only case above batch 8.
Two inputs each: seeded N(0,1), and a ramp in which a mis-addressed tap cannot cancel.  For fp32 crops every element of
the ramp is distinct ((i - N/2) * 2^-12, exact below 2^24).  A 16-bit format has fewer codes (< 65,536) than one image
has elements (76,800), so there the ramp cycles through 2039 distinct values that bf16 and f16 both hold exactly
(+-2^e (1 + m/128), e in [-4, 4)): two elements are equal only where their flat distance is a multiple of the prime
2039, which no column (1), row (160), plane (25,600), image (76,800) or LDS channel (9 x 160) stride is.

The switch is read when a handle is created, so each form is a model of its own from the same seeded state dict, on the
per-convolution plan (VNF_FUSE=0: conv2d_1a readable as a tap) with the heuristic tiles (VNF_AUTOTUNE=0: quick creates;
the layers behind conv2d_1a are the same launches in all three models)."""
import numpy as np
import pytest
import torch

from conftest import seeded_normal

pytestmark = pytest.mark.gpu

CROPS = {"bf16": torch.bfloat16, "f16": torch.float16, "f16x2": torch.float32}
CYCLE = 2039


def _ramp(n, crop):
    total = n * 3 * 160 * 160
    i = torch.arange(total, dtype=torch.int64)
    if crop == torch.float32:
        x = (i - total // 2).to(torch.float32) * 2.0 ** -12
        assert x.unique().numel() == total
    else:
        e = torch.arange(-4, 4, dtype=torch.float32).view(8, 1)
        mag = (2.0 ** e * (1 + torch.arange(128, dtype=torch.float32).view(1, 128) / 128)).reshape(-1)
        codes = torch.cat([-mag.flip(0), mag])[:CYCLE]           # ascending, 2039 of the 2048
        assert codes.unique().numel() == CYCLE and torch.equal(codes.to(crop).float(), codes)
        for stride in (1, 160, 25600, 76800, 17 * 160, 9 * 160):
            assert stride % CYCLE
        x = codes[i % CYCLE]
    return x.view(n, 3, 160, 160).to(crop)


def _model(monkeypatch, dt, n, mode):
    from vn_celeb_face_recognition_amd.models import InceptionResnetV1
    monkeypatch.setenv("VNF_FUSE", "0")
    monkeypatch.setenv("VNF_AUTOTUNE", "0")
    monkeypatch.setenv("VNF_STEM1A_MFMA", str(mode))
    m = InceptionResnetV1(pretrained=None, device="cuda:0", compute_dtype=dt, max_batch=n).eval()
    m._ensure_handle()                               # the handle reads the switch here
    return m


def _run(m, x, n):
    y = m(x)
    t = m.tap("conv2d_1a", n)
    assert t.shape == (n, 32, 79, 79)
    return t.view(np.uint32), y.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f16x2"])
def test_staged_rows_conv2d_1a_is_bitwise_the_gather_and_valu_kernels(monkeypatch, dt, n):
    crop = CROPS[dt]
    inputs = {"normal": seeded_normal((n, 3, 160, 160), 170 + n).to(crop).cuda(), "ramp": _ramp(n, crop).cuda()}
    got = {}
    for mode in (2, 1, 0):
        m = _model(monkeypatch, dt, n, mode)
        for name, x in inputs.items():
            assert x.data_ptr() % 16 == 0
            got[mode, name] = _run(m, x, n)
    for name in inputs:
        tap, emb = got[2, name]
        assert np.isfinite(tap.view(np.float32)).all() and tap.any() and np.isfinite(emb.view(np.float32)).all()
        for other in (1, 0):
            otap, oemb = got[other, name]
            bad = np.argwhere(tap != otap)
            assert len(bad) == 0, (dt, n, name, other, len(bad), bad[:4], tap[tuple(bad[0])], otap[tuple(bad[0])])
            assert np.array_equal(emb, oemb), (dt, n, name, other)


@pytest.mark.parametrize("dt", ["bf16", "f16x2"])
def test_workgroups_that_walk_to_a_second_and_third_band_give_the_gather_kernels_bits(monkeypatch, dt):
    n, crop = 104, CROPS[dt]
    assert 2 * 1024 < n * 20 <= 3 * 1024
    x = seeded_normal((n, 3, 160, 160), 41).to(crop).cuda()
    tap, emb = _run(_model(monkeypatch, dt, n, 2), x, n)
    otap, oemb = _run(_model(monkeypatch, dt, n, 1), x, n)
    assert tap.any()
    bad = np.argwhere(tap != otap)
    assert len(bad) == 0, (dt, len(bad), bad[:4])
    assert np.array_equal(emb, oemb)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f16x2"])
def test_a_crop_tensor_that_is_not_16_byte_aligned_takes_the_gather_kernel_and_gives_the_same_bits(monkeypatch, dt):
    """A contiguous (n,3,160,160) view that starts one element into a larger allocation: its base is 2 or 4 bytes past a
    16-byte boundary, the Python wrapper passes it on as it is (contiguous() of a contiguous view is the view; asserted),
    and launch_stem_conv1a sends it to the gather form.  Same bytes as the aligned tensor through the staged form."""
    n, crop = 3, CROPS[dt]
    x = seeded_normal((n, 3, 160, 160), 29).to(crop).cuda()
    store = torch.zeros(x.numel() + 8, dtype=crop, device="cuda:0")
    shifted = store[1:1 + x.numel()].view(n, 3, 160, 160)
    shifted.copy_(x)
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == x.element_size() and shifted.is_contiguous()
    m = _model(monkeypatch, dt, n, 2)
    assert m._checked_input(shifted).data_ptr() == shifted.data_ptr()      # no copy on the way to vnf_embed
    tap, emb = _run(m, x, n)
    stap, semb = _run(m, shifted, n)
    assert tap.any()
    assert np.array_equal(tap, stap)
    assert np.array_equal(emb, semb)
