"""The five adjoint replays -- rat_policy_gradient / _tail_gradient, rat_policy_param_gradient / _tail_param_gradient and
rat_policy_margin_gradient -- against what the commit before their shared team skeleton and host tail computed
(tests/golden/adjoint_sweeps_parent.npz, recorded from that commit's build by tests/golden/make_adjoint_sweeps_golden.py; cases:
tests/adjoint_sweep_cases.py).

The team of csrc/source_adjoint_lanes.h (the prologue, the Jacobian stage, the seed and the column, the close of a step, the flag) and
replay_finish of csrc/driver.cpp are what the three kernels and the three host paths have in common, and the tests that hold each call to
its NumPy model do so within a tolerance.  This file pins them from outside: no fused multiply-add moved and no exchange reads another
lane, hence every recorded array is compared with array_equal (NaN equal to NaN) and every refusal's text with ==.  No tolerances."""
import os

import numpy as np
import pytest

import adjoint_sweep_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "adjoint_sweeps_parent.npz")) as z:
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
