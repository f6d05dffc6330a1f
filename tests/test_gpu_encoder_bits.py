"""GPU: the exact embeddings of InceptionResnetV1 through the fused-stack kernels against tests/golden/encoder_bits.json,
which tools/make_encoder_bits.py recorded before the eight kernels came to share csrc/fused_device.h, one fragment
schedule per family and one repack template per twin pair.  The other GPU tests hold the 16-bit stem, Block35 and Block8
to the plan bit for bit, but Block17 and the planar split-f16 twins only within tolerances; here every case of
tests/encoder_bits.py must give the bytes it gave then.  A difference is a changed weight stream or operation order (or
a changed toolchain: the failure message shows both version sets)."""
import json
import os

import pytest

from conftest import GOLDEN
from encoder_bits import CASES, case_id, run_case, versions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "encoder_bits.json")) as f:
        return json.load(f)


def test_the_recording_holds_exactly_the_cases(recorded):
    assert sorted(recorded["cases"]) == sorted(case_id(*c) for c in CASES)


@pytest.mark.parametrize("dt,fuse,n", CASES, ids=[case_id(*c) for c in CASES])
def test_embedding_bytes_are_the_recorded_ones(recorded, dt, fuse, n):
    want, got = recorded["cases"][case_id(dt, fuse, n)], run_case(dt, fuse, n)
    print("%s:\n  recorded %s\n  got      %s" % (case_id(dt, fuse, n), want, got))
    if got != want:
        now = versions()
        pytest.fail("%s differs from the recording\nrecorded under torch %s, %s\nrunning under  torch %s, %s"
                    % (case_id(dt, fuse, n), recorded["torch"], recorded["hipcc"], now["torch"], now["hipcc"]))
