"""GPU: the exact bits of both on-device trainers (csrc/mlp_train.hip + trainer.TrainableMLP, csrc/head_train.hip +
trainer.TrainableHead) against tests/golden/trainer_bits.json, which tools/make_trainer_bits.py recorded before the
two trainers came to share csrc/adam_params.h.  Every parameter, Adam moment, loss, hit count and step counter of the
seeded runs of tests/trainer_bits.py must be what it was then; a difference is a changed operation order (or a
changed toolchain: the failure message shows both version sets)."""
import json
import os

import pytest

from conftest import GOLDEN
from trainer_bits import CASES, case_id, run_case, versions

pytestmark = pytest.mark.gpu
IDS = [case_id(kind, shape) for kind, shape in CASES]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "trainer_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs():
    """Each case is run once; the tests below read the result and leave it unchanged."""
    done = {}

    def get(kind, shape):
        if (kind, shape) not in done:
            done[(kind, shape)] = run_case(kind, shape)
        return done[(kind, shape)]
    return get


def _toolchains(recorded):
    now = versions()
    return "\nrecorded under torch %s, %s\nrunning under  torch %s, %s" % (recorded["torch"], recorded["hipcc"], now["torch"], now["hipcc"])


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_every_bit_is_the_recorded_one(recorded, runs, kind, shape):
    want, got = recorded["cases"][case_id(kind, shape)], runs(kind, shape)
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    for k in wrong:
        print("%s %s:\n  recorded %s\n  got      %s" % (case_id(kind, shape), k, want[k], got[k]))
    assert not wrong, "%s differs from the recording in %s%s" % (case_id(kind, shape), wrong, _toolchains(recorded))


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_evaluation_step_leaves_the_state_alone(runs, kind, shape):
    got = runs(kind, shape)
    assert got["after_eval"] == got["after_step3"]
    assert got["step_count_after_step3"] == got["step_count_after_eval"] == 3
    assert got["after_step4"] != got["after_step3"] and got["step_count_after_step4"] == 4


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_checkpoint_round_trip_continues_bit_for_bit(runs, kind, shape):
    got = runs(kind, shape)
    assert got["resumed_after_step4"] == got["after_step4"]
    assert (got["resumed_loss"], got["resumed_hits"], got["resumed_step_count"]) == (got["loss"][4], got["hits"][4], 4)
