"""GPU: the exact outputs of the gallery family (search, mated search, clustering, tracks, track sums) against
tests/golden/gallery_bits.json, which tools/make_gallery_bits.py recorded on the commit named in the file, before the
five streaming kernels came to share one lane descriptor, one keyed maximum, one key decoder and one stage C in
csrc/gallery_core.h.  The family's other GPU tests hold scores to a tolerance and decisions to a float64
oracle; here every case of tests/gallery_bits.py must give the bytes it gave then.  A difference is a changed operation
order or a changed tie rule (or a changed toolchain: the failure message shows both version sets)."""
import json
import os

import pytest

from conftest import GOLDEN
from gallery_bits import CASES, run_case, versions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "gallery_bits.json")) as f:
        return json.load(f)


def test_the_recording_holds_exactly_the_cases(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert len(recorded["recorded_on_commit"]) == 40


@pytest.mark.parametrize("case", list(CASES))
def test_output_bytes_are_the_recorded_ones(recorded, case):
    want, got = recorded["cases"][case], run_case(case)
    print("%s:\n  recorded %s\n  got      %s" % (case, want, got))
    if got != want:
        now = versions()
        pytest.fail("%s differs from the recording in %s\nrecorded on %s under torch %s, %s\nrunning under torch %s, %s"
                    % (case, [k for k in want if got.get(k) != want[k]], recorded["recorded_on_commit"], recorded["torch"],
                       recorded["hipcc"], now["torch"], now["hipcc"]))
