"""The policy entry points against what the commit before their shared host path computed (tests/golden/policy_host_parent.npz, recorded
from that commit's build by tests/golden/make_policy_host_golden.py; cases: tests/policy_host_cases.py).

pack_policy, mc_chunk / chunk_seed, the two rollout launch helpers and the shared evaluation tail of csrc/driver.cpp sit on both sides of
every "bit for bit" relation the other policy tests hold, so this file pins them from outside: the kernels are the same binaries and the
JIT sources the same text, hence every recorded array is compared with array_equal (NaN equal to NaN) and every refusal's text with ==.
No tolerances."""
import os

import numpy as np
import pytest

import policy_host_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "policy_host_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_recording_covers_every_case_and_entry_point(parent):
    assert {k.split("/")[0] for k in parent} == set(cases.CASES)
    for ep in cases.ENTRY_POINTS:
        assert any(f"/{ep}/" in k and not k.endswith("/error") for k in parent), ep


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
