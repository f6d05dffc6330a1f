"""Live Block35 (trunk35.hip, block35.hip, block35s.hip), mixed_7a, Block8 (block8.hip and the plan's convolutions) and
the average pool bit for bit against the exact-arithmetic network of tests/exact_net.py: data on dyadic grids on which
every convolution up to block8 is exact in fp32 in any order, so the bits of every tap follow from the kernels'
documented rounding points alone -- no plan to compare with, no shared weight fold, no recorded output, no tolerance.
The data is checked on the host by tests/test_exact_tail_host.py: exact, no dead channel, rounding in >= 1 % of every
stored tensor, negative values in block8's tap, and every fault this test exists for (a 3x3 tap lost at the last column
or row, the last pixel's taps shifted, a bias from the other parity buffer, an unfolded residual scale, mixed_7a's
second reader at the wrong channel offset, a 1x3 / 3x1 tap that leaks into the next image of a Block8 workgroup, a ReLU
or a 0.2 in block8, a pool over 8 pixels, ...) moves the expected bits.

Cases, per dtype in {bf16, f16, f16x2}, on n = 4 distinct images (a Block8 chain workgroup owns three: one full group
and a group of one) in max_batch = 5 handles, VNF_AUTOTUNE=0:
  A  one live Block35 at each of the five positions, and all five; default switch (bf16 / f16: trunk35.hip, f16x2:
     block35s.hip), and for {0}, {4}, {0..4} VNF_FUSE=2 (block35.hip, bf16 / f16) and VNF_FUSE=0 (the plan).  For {0..4}
     also VNF_FUSE=127: the default leaves mixed_6a.branch1.0 outside the stack kernel (bit 5 is off), this run puts it
     inside.  One expectation for every form: x is carried between the blocks as stored values.
  B  one live Block8 at each of the six positions (5: block8, scale 1.0, no ReLU), and all six; default switch (bf16 /
     f16: the chain kernel, f16x2: plan convolutions), and VNF_FUSE=0 for {0}, {5}, {0..5} in bf16 / f16.
  C  L35 = {2}, L17 = {4, 5}, L8 = {0, 5} in one network, default switch.
  D  batch positions [0,0,0,0], [3,1,0,2] and a batch of one behind a batch of four -- on all five Block35 and on all six
     Block8 in a case each: the two runs in one network do not pass the self-check (exact_net.CASES_D says why).
Every comparison is np.array_equal on the fp32 bits Encoder.tap returns, on the ten taps of exact_net.TAIL_TAPS.
Figures from the MI355X run are at the end of this file."""
import os
import time

import pytest
import torch

import exact_net as en
from test_gpu_trunk17_exact import _same_bits

pytestmark = pytest.mark.gpu

MAX_N = 5
SIXTEEN = ("bf16", "f16")
_created = [0]
_t0 = [None]


def _model(case, fuse):
    """A max_batch = 5 model of the case's state dict; fuse None: the default switch.  The switches are read when the
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


def _check(m, case, what, images=None):
    """One forward; every tap against the case's expectation (images: which of the case's images the batch holds)."""
    idx = list(range(case.x.shape[0])) if images is None else images
    m(case.x[idx].float().cuda())
    torch.cuda.synchronize()
    for t in en.TAIL_TAPS:
        _same_bits(m.tap(t, len(idx)), case.taps[t][idx], "%s %s" % (what, t))


def _report(case, t_case):
    blocks = ["repeat_1.%d" % i for i in case.L35] + [en.block_name("repeat_3", k) for k in case.L8]
    live = [r for r in case.log if r.name.rsplit(".", 1)[0] in blocks or r.name.rsplit(".", 2)[0] in blocks]
    m7a = [r for r in case.log if r.name.startswith("mixed_7a.")]
    print("%s: budget use %.4f, rounded shares: live blocks %.3f .. %.3f, mixed_7a %.3f .. %.3f, pool %.3f; handles so far %d, case %.1f s, module %.1f s" % (
        case.name, max(r.use for r in case.log), min(r.rounded for r in live), max(r.rounded for r in live),
        min(r.rounded for r in m7a), max(r.rounded for r in m7a), case.log[-1].rounded, _created[0], time.time() - t_case, time.time() - _t0[0]))


@pytest.mark.parametrize("L35", [c[0] for c in en.CASES_A], ids=lambda l: "L" + "".join(map(str, l)))
@pytest.mark.parametrize("dt", en.DTYPES)
def test_live_block35_is_bit_exact_in_every_form(dt, L35):
    case = en.make_tail_case(dt, L35)
    t_case = time.time()
    what = "%s L35=%s" % (dt, set(L35))
    default = _model(case, None)
    _check(default, case, what + " default switch")
    extra = {}
    if L35 in ((0,), (4,), en.ALL35):
        for fuse in (("2", "0") if dt in SIXTEEN else ("0",)) + (("127",) if dt in SIXTEEN and L35 == en.ALL35 else ()):
            extra[fuse] = _model(case, fuse)
            _check(extra[fuse], case, what + " VNF_FUSE=" + fuse)
    if L35 == en.ALL35:   # each model did run the form it stands for
        x = case.x.float().cuda()
        p = default.profile(x)
        assert "repeat_1 (fused blocks)" in p and ("x in registers" if dt in SIXTEEN else "one launch per block") in p
        assert "mixed_6a.branch1.0" in p and "+ mixed_6a.branch1.0 in one launch" not in p
        p = extra["0"].profile(x)
        assert "repeat_1 (fused blocks)" not in p and "repeat_1.4.branch2.2" in p
        if dt in SIXTEEN:
            p = extra["2"].profile(x)
            assert "repeat_1 (fused blocks)" in p and "one launch per block" in p and "repeat_2 (persistent trunk)" not in p
            assert "+ mixed_6a.branch1.0 in one launch" in extra["127"].profile(x)
    _report(case, t_case)


@pytest.mark.parametrize("L8", [c[2] for c in en.CASES_B], ids=lambda l: "L" + "".join(map(str, l)))
@pytest.mark.parametrize("dt", en.DTYPES)
def test_live_block8_is_bit_exact_in_the_chain_kernel_and_in_the_plan(dt, L8):
    case = en.make_tail_case(dt, (), (), L8)
    t_case = time.time()
    what = "%s L8=%s" % (dt, set(L8))
    default = _model(case, None)
    _check(default, case, what + " default switch")
    plan = None
    if dt in SIXTEEN and L8 in ((0,), (5,), en.ALL8):
        plan = _model(case, "0")
        _check(plan, case, what + " VNF_FUSE=0")
    if L8 == en.ALL8:     # bf16 / f16: the chain kernel against the plan's three convolutions; f16x2 has the plan only
        x = case.x.float().cuda()
        p = default.profile(x)
        chain = all(en.block_name("repeat_3", k) + " chain (reduce+1x3+3x1)" in p for k in range(6))
        assert chain == (dt in SIXTEEN) and ("block8.branch1.2" in p) == (dt not in SIXTEEN)
        if plan is not None:
            p = plan.profile(x)
            assert "chain (reduce+1x3+3x1)" not in p and "block8.branch1.2" in p and "repeat_3.0.branch1.1" in p
    _report(case, t_case)


@pytest.mark.parametrize("dt", en.DTYPES)
def test_live_blocks_of_all_three_stacks_in_one_network(dt):
    case = en.make_tail_case(dt, *en.CASE_C)
    t_case = time.time()
    _check(_model(case, None), case, "%s L35={2} L17={4,5} L8={0,5}" % dt)
    _report(case, t_case)


@pytest.mark.parametrize("stacks", en.CASES_D, ids=("block35", "block8"))
@pytest.mark.parametrize("dt", en.DTYPES)
def test_an_image_gives_the_same_bits_at_every_batch_position_and_after_a_larger_batch(dt, stacks):
    case = en.make_tail_case(dt, *stacks)
    t_case = time.time()
    m = _model(case, None)
    _check(m, case, "%s image 0 at positions 0 .. 3" % dt, images=[0, 0, 0, 0])
    _check(m, case, "%s images 3, 1, 0, 2" % dt, images=[3, 1, 0, 2])
    _check(m, case, "%s the four images" % dt)
    _check(m, case, "%s a batch of one behind a batch of four" % dt, images=[2])
    _report(case, t_case)


# Figures of the run on the MI355X (48 tests, all bit-exact on all ten taps, none skipped).  Per case: the largest budget
# use max(sum|x*w| + |bias| + |residual|) / 2^(22-q) of any convolution of the network, the smallest .. largest share of
# elements that needed rounding among the stored tensors of the live blocks (Block35: reducer thirds, three 3x3, the
# block's output; Block8: reducer halves, 1x3, 3x1, the block's output) and among mixed_7a's seven, and the share at the
# pool's store.  f16x2 rounds nowhere in front of the pool by construction (a pair holds every value the budget admits);
# its pool store rounds in 0.23 .. 0.46 of the elements.
#
#   case             bf16: use      live blocks    mixed_7a       pool    f16: use       live blocks    mixed_7a       pool    f16x2: use
#   L35={i}, i=0..4  0.0038-0.0045  0.013 .. 0.126 0.115 .. 0.197 0.81-0.82    0.0302-0.0386  0.012 .. 0.116 0.106 .. 0.175 0.81-0.83    0.0302-0.0386
#   L35={0..4}       0.0855         0.013 .. 0.439 0.460 .. 0.474 0.912        0.8398         0.012 .. 0.426 0.458 .. 0.475 0.916        0.8408
#   L8={k}, k=0..5   0.0023-0.0031  0.030 .. 0.180 0.036 .. 0.073 0.88-0.89    0.0187-0.0246  0.028 .. 0.164 0.032 .. 0.066 0.88-0.89    0.0187-0.0246
#   L8={0..5}        0.0177         0.034 .. 0.299 0.036 .. 0.073 0.926        0.1485         0.033 .. 0.301 0.032 .. 0.066 0.933        0.1441
#   C                0.0472         0.013 .. 0.388 0.172 .. 0.234 0.918        0.4036         0.013 .. 0.365 0.163 .. 0.222 0.919        0.8051
#
# Settings that were needed (exact_net.Settings): up-projection weights +-1 alone for runs of more than two blocks, as for
# Block17; Block35 biases calibrated at the quantiles (0.5, 0.6, 0.6) -- at Block17's (0.8, 0.85, 0.85) the outputs of a
# Block35 on the small conv2d_4b trunk stay under 2^8 grid units and 0.14 % of the bf16 reducer rounds; up-projection
# biases positive, and mixed_7a's biases calibrated per case, so that no channel is dead; 14 weights per row in the Block8
# reducer (192 rows have to cover 1792 k positions).  All five Block35 take 0.84 of the f16 budget: the longest run fits,
# with little to spare.  Five live Block35 in front of six live Block8 do not fit (case D runs them in a case each).
# Handle creations: 71 (A: 13 per 16-bit dtype, 9 for f16x2; B: 10 per 16-bit dtype, 7 for f16x2; C: 3; D: 6).
# Wall time of the module: 53 s, of which the slowest test (bf16, L35 = {0}, three handles and the first host stem) takes
# 2.5 s; the slowest run of a case on the GPU alone (f16, all five Block35, four handles and four profiles) 1.1 s.
