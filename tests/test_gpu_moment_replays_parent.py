"""The six moment replays -- rat_policy_worst_case_trajectory / _disturbance / _params and rat_policy_tail_trajectory / _disturbance /
_params -- against what the commit before their shared kernel skeleton and host tail computed (tests/golden/moment_replays_parent.npz,
recorded from that commit's build by tests/golden/make_moment_replays_golden.py; cases: tests/moment_replay_cases.py).

The schedule of csrc/policy_mc.hip's moments_body (groups to wavefronts, the liveness word, the LDS reduction into the partials) and
replay_finish of csrc/driver.cpp sit on both sides of every "bit for bit" relation the other tests of these calls hold -- tail against
dense, alpha = 0 against theta = 0 -- so this file pins them from outside: no floating-point sum changed its order, hence every recorded
array is compared with array_equal (NaN equal to NaN) and every refusal's text with ==.  No tolerances."""
import os

import numpy as np
import pytest

import moment_replay_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "moment_replays_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_recording_covers_every_case_and_entry_point(parent):
    assert {k.split("/")[0] for k in parent} == set(cases.CASES)
    for ep in cases.ENTRY_POINTS:
        assert any(f"/{ep}/" in k and not k.endswith("/error") for k in parent), ep
        assert any(f"/{ep}/" in k and k.endswith("/error") for k in parent), ep


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
