"""The persistent Block17 kernels (trunk17.hip for bf16 / f16, trunk17s.hip for the planar split-f16 dtype) bit for bit
against the exact-arithmetic network of tests/exact_net.py: weights, biases and images on dyadic grids on which every
convolution from conv2d_1a to repeat_2 is exact in fp32, so the bits every tap must hold follow from the kernels'
documented rounding points alone -- no plan, no oracle order, no recorded output, no tolerance.  The data is checked on
the host by tests/test_exact_net_host.py: exact, rounding in >= 1 % of every stored tensor, and every fault this test
exists for (a 1x7 / 7x1 tap lost at one border, two channels of a wave's tile swapped, a k-step of the next block's
weights, a neighbour's bias, a trunk rounded between blocks, a truncating store) moves the expected bits.

Cases, per dtype in {bf16, f16, f16x2}: one live Block17 at each of the ten positions (the other nine are identities);
runs {0,1}, {4,5}, {8,9} and all ten blocks live (the longest run the self-check admits is the whole stack, in every
dtype).  The fused model (default VNF_FUSE; VNF_FUSE=1, the trunk kernel alone, for f16x2) must give the carry="fp32"
expectation: the trunk unrounded across live blocks, one rounding at the final store.  For L = {0}, {9} and every run a
VNF_FUSE=0 model on the same state dict must give carry="stored", which rounds the trunk after every block: the
restatement and the folding assumptions proved against the per-convolution plan.  The taps in front of repeat_2 are
compared as well (conv2d_1a, conv2d_3b, conv2d_4b, repeat_1, mixed_6a): they localise a failure and give the fused stem,
Block35 and mixed_6a kernels a plan-independent check.  Every comparison is np.array_equal on the fp32 bits Encoder.tap
returns (a 16-bit value or a split pair's hi + lo is an fp32 value).

n = 2 distinct images in a max_batch = 3 handle, VNF_AUTOTUNE=0 (quick creates); the host expectation of a dtype's
upstream is computed once.  Figures from the MI355X run are at the end of this file."""
import os
import time

import numpy as np
import pytest
import torch

import exact_net as en

pytestmark = pytest.mark.gpu

MAX_N = 3
FUSED = {"bf16": None, "f16": None, "f16x2": "1"}       # VNF_FUSE of the fused model; None: the default switch
_created = [0]
_t0 = [None]


def _model(case, fuse):
    """A max_batch = 3 model of the case's state dict; fuse None: the default switch.  The switches are read when the
    handle is created, so the environment is restored right behind it."""
    from vn_celeb_face_recognition_amd.models import InceptionResnetV1
    if _t0[0] is None:
        _t0[0] = time.time()
    keep = {k: os.environ.get(k) for k in ("VNF_FUSE", "VNF_AUTOTUNE")}
    os.environ["VNF_AUTOTUNE"] = "0"
    if fuse is None:
        os.environ.pop("VNF_FUSE", None)
    else:
        os.environ["VNF_FUSE"] = str(fuse)
    try:
        m = InceptionResnetV1(pretrained=None, device="cuda:0", compute_dtype=case.dt, max_batch=MAX_N).eval()
        m.load_state_dict(case.sd)
        m._ensure_handle()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _created[0] += 1
    return m


def _same_bits(got, want, what):
    """got: the fp32 array of a tap; want: float64 NCHW tensor.  Reports count, first (image, channel, row, column)."""
    g, w = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), en.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in bad[:6]]
        raise AssertionError("%s: %d of %d elements differ; (image, channel, row, column), got, want: %s" % (what, len(bad), g.size, first))


def _check(m, case, x, want_r2, what, images=None):
    """One forward; every tap of the path against the case's expectation (images: which of the case's images x holds)."""
    n = x.shape[0]
    idx = list(range(n)) if images is None else images
    m(x.float().cuda())
    torch.cuda.synchronize()
    for t in en.TAPS:
        want = want_r2 if t == "repeat_2" else case.taps[t]
        _same_bits(m.tap(t, n), want[idx], "%s %s" % (what, t))


def _report(case):
    live = [r for r in case.log if not r.name.endswith(".up") and r.name != "repeat_2.store"]
    print("%s L=%s: budget use %.4f, rounded shares %.3f .. %.3f, final store %.3f, handles so far %d, %.1f s" % (
        case.dt, "".join(map(str, case.live)), max(r.use for r in case.log), min(r.rounded for r in live), max(r.rounded for r in live),
        case.log[-1].rounded, _created[0], time.time() - _t0[0]))


@pytest.mark.parametrize("k", range(10))
@pytest.mark.parametrize("dt", en.DTYPES)
def test_one_live_block17_is_bit_exact_at_every_position_of_the_stack(dt, k):
    case = en.make_case(dt, (k,))
    want = en.expected(case, "fp32", check=True)
    what = "%s L={%d}" % (dt, k)
    _check(_model(case, FUSED[dt]), case, case.x, want, what + " fused")
    if k in (0, 9):   # one live block: the plan's expectation is the same bits
        assert torch.equal(en.expected(case, "stored"), want)
        _check(_model(case, "0"), case, case.x, want, what + " plan")
    _report(case)


@pytest.mark.parametrize("live", en.RUNS, ids=lambda l: "L" + "".join(map(str, l)))
@pytest.mark.parametrize("dt", en.DTYPES)
def test_a_run_of_live_blocks_carries_the_trunk_in_fp32_and_the_plan_in_16_bits(dt, live):
    case = en.make_case(dt, live)
    want = en.expected(case, "fp32", check=True)
    plan = en.expected(case, "stored")
    if dt != "f16x2":
        assert not torch.equal(plan, want)
    what = "%s L=%s" % (dt, set(live))
    fused, unfused = _model(case, FUSED[dt]), _model(case, "0")
    _check(fused, case, case.x, want, what + " fused")
    _check(unfused, case, case.x, plan, what + " plan")
    if live == en.LONGEST:   # the fused model did run the persistent kernel, the other one the forty convolutions
        x = case.x.float().cuda()
        assert "repeat_2 (persistent trunk)" in fused.profile(x) and "repeat_2 (persistent trunk)" not in unfused.profile(x)
        assert "repeat_2.9.branch1.2" in unfused.profile(x)
    _report(case)


@pytest.mark.parametrize("dt", en.DTYPES)
def test_an_image_gives_the_same_bits_at_every_batch_position_and_after_a_larger_batch(dt):
    case = en.make_case(dt, (4, 5))
    want = en.expected(case, "fp32", check=True)
    m = _model(case, FUSED[dt])
    _check(m, case, case.x[[0, 0, 0]], want, "%s image 0 at positions 0, 1, 2" % dt, images=[0, 0, 0])
    _check(m, case, case.x[[1, 0, 1]], want, "%s images 1, 0, 1" % dt, images=[1, 0, 1])
    _check(m, case, case.x[[1]], want, "%s a batch of one behind a batch of three" % dt, images=[1])
    _report(case)


def test_the_default_split_f16_plan_gives_the_exact_bits_as_well():
    """With the default switch the f16x2 stem and Block35 kernels (stem_mids.hip, block35s.hip) run too.  They are not
    bitwise the plan on ordinary data (another summation order), so no other test can ask them for bits; on exact data
    the order does not matter and every tap must come out as expected."""
    case = en.make_case("f16x2", en.LONGEST)
    _check(_model(case, None), case, case.x, en.expected(case, "fp32", check=True), "f16x2 default switch, ten live blocks")
    _report(case)


# Figures of the run on the MI355X (46 cases, all bit-exact, none skipped).  Per case: the largest budget use
# max(sum|x*w| + |bias| + |residual|) / 2^(22-q) of any convolution of the live blocks, the smallest .. largest share of
# elements that needed rounding among the live blocks' stored tensors (branch0, branch1.0, 1x7, 7x1), and the share at the
# final repeat_2 store.  f16x2 rounds nowhere by construction (a pair holds every value the budget admits).
#
#   case           bf16: use     rounded         store   f16: use      rounded         store   f16x2: use
#   L={k}, k=0..9  0.0018-0.0023 0.014 .. 0.028  0.17-0.19    0.0135-0.0181 0.013 .. 0.027  0.16-0.17    0.0135-0.0181
#   L={0,1}        0.0043        0.019 .. 0.039  0.194        0.0321        0.017 .. 0.036  0.182        0.0321
#   L={4,5}        0.0040        0.017 .. 0.041  0.188        0.0332        0.014 .. 0.034  0.177        0.0332
#   L={8,9}        0.0040        0.017 .. 0.039  0.197        0.0300        0.017 .. 0.037  0.186        0.0301
#   L={0..9}       0.0252        0.019 .. 0.158  0.361        0.2622        0.017 .. 0.163  0.351        0.2846
#
# Longest live run admitted by the self-check: all ten blocks, in every dtype (up-projection weights +-1 for runs of more
# than two blocks; the single blocks and the pairs use +-1 and +-1/2).  The single-block f16 cases reach the 1 % rounding
# share as well (smallest share of any stored tensor: 1.3 %).
# Handle creations: 64 (21 per dtype: 10 + 2 for the single blocks, 2 per run, 1 for the batch positions; 1 for the
# default-switch f16x2 plan).
# Wall time of the module: 37 s, of which the slowest case (f16x2, ten live blocks, two handles) takes 2.3 s.
