"""Host checks of the exact-arithmetic network behind repeat_2 and of its live Block35 (tests/exact_net.py), for every
case tests/test_gpu_exact_tail.py runs: the data is exact (self-check of every convolution, budget use < 1), no channel
of a live block is dead, the rounding the case is there to exercise happens, block8's tap has negative values, the
pool's quotient tells a division by 9 from a multiplication by fl32(1/9), and each fault the GPU test exists for -- put
into the restatement, never into a kernel -- moves the expected bits of the tap behind it.  These are conditions on the
data: a case that misses one needs other generator settings, not another threshold.  Every test prints its figures (-s).

Rounding in f16x2: a split pair holds every value the budget allows, so nothing rounds in front of the pool (the
self-check asserts it) and the mutations that are about rounding cannot move a bit; there the lo halves must be in use
in >= 1 % of the repeat_1, mixed_7a and block8 taps, and the pool's store -- a quotient by 9 is not on the grid -- must
round in >= 1 %.

One fault cannot reach a 16-bit tap: fl32(s / 9) and fl32(s * fl32(1/9)) differ by one fp32 ulp, which the bf16 / f16 store
of the pool erases (no quotient by 9 lies within an fp32 ulp of a 16-bit rounding boundary).  For those types the test asserts
that the mutation moves the fp32 quotient and leaves the tap alone; the f16x2 pair keeps ~22 bits and its tap moves.

The refactoring of exact_net.py into stage functions kept the bits of the 46 cases of tests/test_gpu_trunk17_exact.py:
tests/golden/exact_net_trunk17_hashes.json holds the SHA-256 of bits(expected(case, carry)) for every (dtype, live set)
and both carries, and of the base state dict, recorded before the split."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import exact_net as en
from conv_reference import _FMT, rne

CASES = [(dt,) + c for dt in en.DTYPES for c in en.TAIL_CASES]
_ids = ["%s-L35_%s-L17_%s-L8_%s" % ((dt,) + tuple("".join(map(str, l)) or "none" for l in c)) for dt, *c in CASES]
HASHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_net_trunk17_hashes.json")


def _moved(case, mut, mut_block=None):
    want, got = en.mutated(case, mut, mut_block)
    return int((en.bits(got) != en.bits(want)).sum())


@pytest.mark.parametrize("dt", en.DTYPES)
def test_the_stage_functions_give_the_bits_the_trunk17_cases_had_before_the_split(dt):
    want = json.load(open(HASHES))
    sd = en.base_state_dict(dt)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(np.asarray(sd[k])).tobytes())
    assert h.hexdigest() == want["%s-base" % dt]
    n = 0
    for live in en.SINGLES + en.RUNS:
        case = en.make_case(dt, live)
        for carry in ("fp32", "stored"):
            got = hashlib.sha256(en.bits(en.expected(case, carry)).tobytes()).hexdigest()
            assert got == want["%s-L%s-%s" % (dt, "".join(map(str, live)), carry)], (dt, live, carry)
            n += 1
    assert n == 28 and len(want) == 3 * 29


def test_the_residual_scales_of_block35_and_block8_fold_back_to_the_grid_weight():
    for scale in (np.float32(0.17), np.float32(0.2)):
        for g in (1.0, -1.0, 0.5, -0.5, 0.25):
            assert np.float32(np.float32(np.float32(g) / scale) * scale) == np.float32(g), (scale, g)
    # not every grid value folds back: the generator draws biases only from those that do, and asserts it per tensor
    for dt in en.DTYPES:
        step = en.SETTINGS[dt].in_step
        for scale in (en.RES_SCALE35, en.RES_SCALE8):
            ok = en._foldback_grid(scale, step)
            print(dt, float(scale), "bias grid values that fold back:", ok.tolist())
            assert 8 <= len(ok) <= 15
    sd = {}
    with pytest.raises(AssertionError, match="scale"):
        en._set_up(sd, "p", np.ones((1, 1), np.float32), np.array([7 / 8], np.float32), np.float32(0.17))   # 7 is not in the list


def test_an_identity_block8_is_the_identity_without_its_relu():
    """block8 has no ReLU: a zero up-projection gives x + 0 = x on the stored trunk; repeat_3() asserts the trunk in front
    of every identity block is non-negative and stored, and hands it on untouched."""
    case = en.make_tail_case("bf16", (), (), (4,))
    assert en.live8(case.sd) == (4,) and en._is_identity(case.sd, "block8")
    assert torch.equal(case.taps["block8"], case.taps["repeat_3"]) and bool((case.taps["block8"] >= 0).all())
    prm = en.block8_params(case.sd, 5, "bf16")
    assert not bool(prm["up"][0].any()) and not bool(prm["up"][1].any())
    y = en.block8(prm, case.taps["repeat_3"], "bf16", "block8", relu=False)
    assert torch.equal(y, case.taps["repeat_3"])
    with pytest.raises(AssertionError, match="identity Block8"):
        en.repeat_3(en.tail_state_dict("bf16"), -case.taps["mixed_7a"], "bf16")


@pytest.mark.parametrize("dt,L35,L17,L8", CASES, ids=_ids)
def test_case_is_exact_rounds_has_no_dead_channel_and_sees_the_faults(dt, L35, L17, L8):
    case = en.make_tail_case(dt, L35, L17, L8)              # AssertionError: the data set is rejected
    assert case.x.shape == (4, 3, 160, 160) and len({en.bits(case.x[i]).tobytes() for i in range(4)}) == 4
    use = max(r.use for r in case.log)
    print("%s: largest budget use %.4f (finest grid 2^-%d)" % (case.name, use, max(r.q for r in case.log)))
    assert 0 < use < 1.0
    # ---- which records belong to live blocks, to mixed_7a, to the pool
    blocks = ["repeat_1.%d" % i for i in L35] + ["repeat_2.%d" % k for k in L17] + [en.block_name("repeat_3", k) for k in L8]
    of_live = [r for r in case.log if r.name.rsplit(".", 1)[0] in blocks or r.name.rsplit(".", 2)[0] in blocks]
    assert len(of_live) == 7 * len(L35) + 5 * len(L17) + 5 * len(L8)
    m7a = [r for r in case.log if r.name.startswith("mixed_7a.")]
    pool = case.log[-1]
    assert len(m7a) == 7 and pool.name == "avgpool_1a"
    # the up-projection of a Block17 is not a stored tensor: trunk17.hip carries it in fp32
    stored_recs = [r for r in of_live + m7a if not (r.name.startswith("repeat_2.") and r.name.endswith(".up"))] + [pool]
    dead = [(r.name, r.dead) for r in stored_recs if r.dead]
    assert not dead, dead
    # ---- rounding
    if dt in ("bf16", "f16"):
        low = min(stored_recs, key=lambda r: r.rounded)
        print("   smallest rounded share %.4f (%s), mixed_7a %.3f .. %.3f, pool %.3f" % (
            low.rounded, low.name, min(r.rounded for r in m7a), max(r.rounded for r in m7a), pool.rounded))
        for r in stored_recs:
            assert r.rounded >= 0.01, (r.name, r.rounded)
    else:
        assert all(r.rounded == 0.0 for r in stored_recs[:-1])
        lo = {t: float((rne(case.taps[t], *_FMT["f16"]) != case.taps[t]).double().mean()) for t in ("repeat_1", "mixed_7a", "block8")}
        print("   nothing rounds in front of the pool; lo halves in use: %s; the pool store rounds in %.3f" % (lo, pool.rounded))
        assert min(lo.values()) >= 0.01 and pool.rounded >= 0.01
    # ---- block8 without its ReLU, the pool's quotient
    b8 = case.taps["block8"]
    neg = float((b8 < 0).double().mean())
    s32, exact = en.pool_sums(b8)
    differ = float((s32 / 9.0 != s32 * (torch.tensor(1.0) / 9.0)).double().mean())
    print("   block8 tap negative in %.3f; fl32(s / 9) != fl32(s * fl32(1/9)) in %.3f of the pool" % (neg, differ))
    assert exact and differ >= 0.01
    assert neg >= 0.10 if 5 in L8 else neg == 0.0
    # ---- every fault moves the expected bits of the tap behind it
    muts = list(en.MUT7A + en.MUTPOOL)
    if L35:
        muts += [m for m in en.MUT35 if not (
            (m == "b35_bias_other_parity" and len(L35) < 3) or (m == "b35_carry_unrounded" and (len(L35) < 2 or dt == "f16x2")) or
            (m == "b35_truncate_b2" and dt == "f16x2"))]
    if L8:
        muts += [m for m in en.MUT8 if not (
            (m in ("b8_relu_in_block8", "b8_scale_in_block8") and 5 not in L8) or (m == "b8_scale_unfolded" and L8[0] == 5))]
    moved = {m: _moved(case, m) for m in muts}
    if dt != "f16x2":   # a 16-bit store hides one fp32 ulp: there the fault moves the quotient in front of the store
        assert moved["pool_reciprocal"] == 0
        moved["pool_reciprocal"] = int((en.bits(en.avgpool(b8, "f32", mut="pool_reciprocal")) != en.bits(en.avgpool(b8, "f32"))).sum())
    print("   elements moved: " + " ".join("%s %d" % kv for kv in moved.items()))
    for m, cnt in moved.items():
        assert cnt > 0, m
    # in a run, a fault in the first block is seen as well as one in the last (the default), and the other way round
    if len(L35) >= 2:
        assert _moved(case, "b35_tap_col16", L35[0]) > 0 and _moved(case, "b35_swap_channels", L35[0]) > 0
    if len(L8) >= 2:
        assert _moved(case, "b8_bias_shifted", L8[-1]) > 0 and _moved(case, "b8_tap_1x3_left", L8[-1]) > 0


def test_the_mutation_lists_are_the_faults_the_cases_run():
    assert len(en.MUT35) == 10 and len(en.MUT7A) == 3 and len(en.MUT8) == 9 and len(en.MUTPOOL) == 2
    # every Block35 and Block8 mutation runs in some case (the run of each stack takes all of them, f16x2 aside)
    assert en.ALL35 in [c[0] for c in en.TAIL_CASES] and en.ALL8 in [c[2] for c in en.TAIL_CASES]
    assert set(en.CASES_D) <= set(en.TAIL_CASES)


def test_the_leak_mutations_read_the_image_the_workgroup_holds_next():
    """Groups of three images from image 0 on: with four images, image 3 is a group of one."""
    t = torch.arange(4.0, dtype=torch.float64).reshape(4, 1, 1, 1) + 1.0
    assert en._next_image(t).flatten().tolist() == [2.0, 3.0, 0.0, 0.0]
    assert en._next_image(t, single_reads=2).flatten().tolist() == [2.0, 3.0, 0.0, 3.0]


@pytest.mark.parametrize("dt", ("f16", "f16x2"))
def test_a_data_set_over_the_budget_is_rejected(dt):
    """The self-check refuses, it does not weaken: behind five live Block35 the six live Block8 do not fit -- why the
    batch-position cases take the two stacks one at a time (exact_net.CASES_D)."""
    with pytest.raises(AssertionError, match="budget"):
        en.make_tail_case(dt, *en.CASE_D_REJECTED)


def test_the_pool_restatement_divides_once_and_rounds_once():
    b8 = torch.zeros((1, 2, 3, 3), dtype=torch.float64)
    b8[0, 0] = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, -9.5]])
    b8[0, 1, 2, 2] = 1.0
    out = en.avgpool(b8, "bf16", check=True)
    want = [float(torch.tensor(np.float32(26.5) / np.float32(9)).bfloat16()), float(torch.tensor(np.float32(1) / np.float32(9)).bfloat16())]
    assert out.shape == (1, 2, 1, 1) and out.flatten().tolist() == want
    assert en.avgpool(b8, "bf16", mut="pool_8_of_9").flatten().tolist()[1] == 0.0
    a, b = np.float32(17.0) / np.float32(9.0), np.float32(17.0) * (np.float32(1.0) / np.float32(9.0))
    assert a != b       # 17: the smallest integer on which the reciprocal multiply shows
