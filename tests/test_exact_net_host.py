"""Host checks of the exact-arithmetic network (tests/exact_net.py) for every case tests/test_gpu_trunk17_exact.py runs:
the data is exact (self-check of every convolution), the rounding it is there to exercise happens, the multi-block
cases tell the persistent kernels' fp32 trunk from the plan's 16-bit one, and each fault the GPU test exists for -- put
into the restatement, never into a kernel -- moves the expected repeat_2 bits.  Every test prints its figures (-s).

Rounding in f16x2: a split pair holds every value the budget allows, so nothing rounds there and the two mutations that
are about rounding (round_trunk, truncate_7x1) cannot move a bit; for that type the test asks instead that the lo halves
are in use (values an f16 alone could not hold) in at least 1 % of every stored tensor.  Single-block cases reach the
1 % share in f16 as well (the smallest share of any stored tensor of any case is printed by the case's test)."""
import numpy as np
import pytest
import torch

import exact_net as en
from conv_reference import _FMT, rne

CASES = [(dt, live) for dt in en.DTYPES for live in en.SINGLES + en.RUNS]
_ids = ["%s-L%s" % (dt, "".join(map(str, live))) for dt, live in CASES]


def test_the_batchnorm_of_the_generator_folds_to_exactly_one_and_the_bias():
    b = np.array([-3.125, 0.0, 0.875, 1234.625], np.float32)
    one, zero = np.ones(4, np.float32), np.zeros(4, np.float32)
    s, t = en.bn_fold(one, b, zero, np.full(4, 0.999, np.float32))
    assert s.dtype == np.float32 and np.all(s == np.float32(1.0)) and np.array_equal(t, b)
    # the assertion has teeth: the float32 above 0.999 and the variance 1 of a fresh BatchNorm do not fold to 1
    v = np.float32(0.999)
    for other in (np.nextafter(v, np.float32(2)), np.float32(1.0)):
        s, _ = en.bn_fold(one, b, zero, np.full(4, other, np.float32))
        assert np.all(s != np.float32(1.0)), other
    # and the double-precision fold is the one of csrc/plan.cpp: eps is the float 1e-3f, not the double 1e-3
    sc = 1.0 / np.sqrt(np.float64(v) + np.float64(np.float32(1e-3)))
    assert np.float32(sc) == np.float32(1.0) and sc != 1.0


def test_the_residual_scale_folds_back_to_the_grid_weight():
    for g in (1.0, -1.0, 0.5, -0.5, 0.25, 0.375, 15 / 8, -127 / 64):
        assert np.float32(np.float32(10.0 * g) * np.float32(0.10)) == np.float32(g), g


@pytest.mark.parametrize("dt", en.DTYPES)
def test_upstream_of_repeat_2_is_exact_and_the_identity_blocks_are_identities(dt):
    x, taps, log = en.upstream_cached(dt, 2, check=True)
    assert torch.equal(rne(x, *_FMT["bf16" if dt == "bf16" else "f16"]), x)       # the images are 16-bit values as well
    for r in log:
        print("%-5s %-20s q=%d budget use %.5f rounded %.4f non-zero %.2f" % (dt, r.name, r.q, r.use, r.rounded, r.nonzero))
        assert 0 < r.use < 1.0 and r.nonzero > 0.2
    assert torch.equal(taps["repeat_1"], taps["conv2d_4b"])
    assert not torch.equal(x[0], x[1]) and torch.equal(en.images(dt, 3)[:2], x)
    sd = en.base_state_dict(dt)
    assert en.live_set(sd) == ()
    m = taps["mixed_6a"]
    for carry in ("fp32", "stored"):
        assert torch.equal(en.repeat_2(sd, m, dt, carry), m)
    assert taps["mixed_6a"].shape == (2, 896, 8, 8) and float((m != 0).double().mean()) > 0.3


@pytest.mark.parametrize("dt,live", CASES, ids=_ids)
def test_case_is_exact_rounds_discriminates_and_sees_the_faults(dt, live):
    case = en.make_case(dt, live)
    want = en.expected(case, "fp32", check=True)          # AssertionError: the data set is rejected
    assert en.live_set(case.sd) == live
    use = max(r.use for r in case.log)
    print("%s L=%s: largest budget use %.4f (finest grid 2^-%d), repeat_2 max %g" % (dt, live, use, max(r.q for r in case.log), want.max().item()))
    assert 0 < use < 1.0
    # ---- rounding bites in every stored tensor of every live block and at the final store
    stored_recs = [r for r in case.log if not r.name.endswith(".up")]
    assert len(stored_recs) == 4 * len(live) + 1 and stored_recs[-1].name == "repeat_2.store"
    dead = [(r.name, r.dead) for r in stored_recs[:-1] if r.dead]
    assert not dead, dead                                   # every channel of every intermediate carries values
    if dt in ("bf16", "f16"):
        for r in stored_recs:
            assert r.rounded >= 0.01, (r.name, r.rounded)
        print("   rounded shares: " + " ".join("%s %.3f" % (r.name.replace("repeat_2.", ""), r.rounded) for r in stored_recs))
    else:
        assert all(r.rounded == 0.0 for r in stored_recs)
        lo = float((rne(want, *_FMT["f16"]) != want).double().mean())
        print("   nothing rounds; repeat_2 values that need the lo half: %.3f" % lo)
        assert lo >= 0.01
    # ---- the two trunks differ where both exist
    plan = en.expected(case, "stored")
    diff = float((plan != want).double().mean())
    print("   fp32 trunk != 16-bit trunk in %.4f of repeat_2" % diff)
    if len(live) >= 2 and dt in ("bf16", "f16"):
        assert diff >= 0.01
    else:
        assert diff == 0.0       # one live block: one rounding in either mode; a split pair: none
    # ---- every fault moves the expected bits
    moved = {}
    for mut in en.MUTATIONS:
        if mut == "round_trunk" and (len(live) < 2 or dt == "f16x2"):
            continue             # no second block behind the rounding / nothing to round
        if mut == "truncate_7x1" and dt == "f16x2":
            continue
        moved[mut] = int((en.bits(en.expected(case, "fp32", mut=mut)) != en.bits(want)).sum())
    print("   elements moved: " + " ".join("%s %d" % kv for kv in moved.items()))
    for mut, cnt in moved.items():
        assert cnt > 0, mut
    # a mutation in the last live block is seen as well as one in the first
    if len(live) >= 2:
        last = int((en.bits(en.expected(case, "fp32", mut="bias_shifted", mut_block=live[-1])) != en.bits(want)).sum())
        assert last > 0


def test_a_data_set_over_the_budget_is_rejected():
    """The self-check refuses, it does not weaken: with |g| = 1/8 the grid gets three bits finer per block, and ten live
    f16 blocks no longer fit."""
    from dataclasses import replace
    st = replace(en.SETTINGS["f16"], up_g=(0.125,))
    case = en.make_case("f16", en.LONGEST, settings=st)
    with pytest.raises(AssertionError, match="budget"):
        en.expected(case, "fp32", check=True)


def test_truncation_and_bits_helpers():
    v = torch.tensor([1.0, 257.0, 258.0, 259.0, 0.0, 3.140625], dtype=torch.float64)
    assert en.truncated(v, "bf16").tolist() == [1.0, 256.0, 258.0, 258.0, 0.0, 3.140625]
    assert en.bits(torch.tensor([1.0, 0.0], dtype=torch.float64)).tolist() == [0x3F800000, 0]
    assert en.grid_q(torch.tensor([0.0, 1.5, -0.375], dtype=torch.float64)) == 3
