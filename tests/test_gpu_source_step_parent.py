"""The rollout kernels of source models -- rat_policy_evaluate, rat_policy_evaluate_noise and the w_out replay behind it, both
rat_policy_rare_event_* calls under user noise, rat_policy_events_user and a solve -- against what the commit before csrc/source_step.h
computed (tests/golden/source_step_parent.npz, recorded from that commit's build by tests/golden/make_source_step_golden.py; cases:
tests/source_step_cases.py).

The header holds pieces that sit on both sides of the bit-for-bit relations the other tests of these calls hold (rare event at a zero
shift against the events of an evaluation), so this file pins them from outside: every recorded array is compared with array_equal (NaN
equal to NaN) and every text with ==.  No tolerances."""
import os

import numpy as np
import pytest

import source_step_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "source_step_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_recording_covers_every_case_and_call(parent):
    assert {k.split("/")[0] for k in parent} == set(cases.CASES)
    assert not any(k.endswith("/error") for k in parent)
    for ep in cases.ENTRY_POINTS:
        assert any(f"/{ep}/" in k and k.endswith("/values") for k in parent), ep


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_output_is_the_parent_commits(name, parent):
    got = cases.run(name)
    want = {k: v for k, v in parent.items() if k.split("/")[0] == name}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        if isinstance(got[k], str):
            assert got[k] == str(want[k]), k
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
