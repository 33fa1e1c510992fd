"""Records tests/golden/policy_host_parent.npz: what the policy entry points compute on the cases of tests/policy_host_cases.py BEFORE
they shared one host path for packing the policy, chunking the rollouts and reducing the costs.  It was run on an MI355X against the
library built from the commit before that change (RATILQR_SO pointing at that build), and must only ever be re-run against such a parent
build: the file is what "the shared helpers changed no bit" is tested against, so it may not come from the tree under test.

    RATILQR_SO=<library of the parent commit> python tests/golden/make_policy_host_golden.py [output.npz]

Prints every refusal a case did not expect, and fails unless every entry point has at least one successful recording."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import policy_host_cases as cases  # noqa: E402

rec = {}
for name in cases.CASES:
    rec.update(cases.run(name))
for line in cases.UNEXPECTED:
    print("UNEXPECTED", line)
for ep in cases.ENTRY_POINTS:
    n_ok = sum(1 for k in rec if f"/{ep}/" in k and not k.endswith("/error"))
    n_err = sum(1 for k in rec if f"/{ep}/" in k and k.endswith("/error"))
    print(f"{ep}: {n_ok // 2} calls recorded, {n_err} refusals")
    assert n_ok > 0, f"no successful recording of {ep}"
assert not cases.UNEXPECTED, "the parent refused calls the cases expect to succeed (or the reverse)"
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "policy_host_parent.npz")
np.savez_compressed(out, **rec)
print("recorded", len(rec), "entries,", os.path.getsize(out), "bytes, library", cases.rat.SO_PATH)
