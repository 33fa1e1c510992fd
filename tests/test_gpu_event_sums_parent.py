"""The event sums -- rat_policy_events / _user (ev_sums, ev_final) and rat_policy_tail_events / _user (tle_sums, tle_final, and ev_sums
on the tail weights under the switch tail_dense) -- against what the commit before their shared bodies computed
(tests/golden/event_sums_parent.npz, recorded from that commit's build by tests/golden/make_event_sums_golden.py; cases:
tests/event_sum_cases.py).

ev_sums_body<TAIL> and ev_final_body<TAIL> of csrc/policy_mc.hip hold what the KL and the tail variants have in common -- the assignment
of rollouts to lanes, the partials' addresses, the trees, the first-or-add stores, the counts and the largest margin, the slot reduction
and six of the eight output slots -- and the tests that hold each call to its NumPy model do so within a tolerance.  This file pins them
from outside: no sum changed its order and no selection became a product, hence every recorded array is compared with array_equal (NaN
equal to NaN) and every refusal's text with ==.  No tolerances."""
import os

import numpy as np
import pytest

import event_sum_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "event_sums_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_recording_covers_every_case_and_entry_point(parent):
    assert {k.split("/")[0] for k in parent} == set(cases.CASES)
    for ep in cases.ENTRY_POINTS:
        assert any(f"/{ep}/" in k and k.endswith("/values") for k in parent), ep
        assert any(f"/{ep}/" in k and k.endswith("/error") for k in parent), ep
    for ep in cases.TAIL_ENTRY_POINTS:
        assert any(f"/{ep}/" in k and k.endswith("_dense/values") for k in parent), ep


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
