"""Records tests/golden/moment_replays_parent.npz: what the six moment replays compute on the cases of tests/moment_replay_cases.py BEFORE
they shared one kernel skeleton (csrc/policy_mc.hip) and one host tail (csrc/driver.cpp).  It was run on an MI355X against the library
built from the commit before that change (RATILQR_SO pointing at that build), and must only ever be re-run against such a parent build:
the file is what "the skeleton changed no bit" is tested against, so it may not come from the tree under test.

    RATILQR_SO=<library of the parent commit> python tests/golden/make_moment_replays_golden.py [output.npz]

Prints every refusal a case did not expect (and every success where it expected a refusal) as UNEXPECTED, and fails unless there is none
and every entry point has at least one successful recording."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import moment_replay_cases as cases  # noqa: E402

rec = {}
for name in cases.CASES:
    t0 = time.perf_counter()
    rec.update(cases.run(name))
    print(f"{name}: {time.perf_counter() - t0:.2f} s")
for line in cases.UNEXPECTED:
    print("UNEXPECTED", line)
for ep in cases.ENTRY_POINTS:
    n_ok = sum(1 for k in rec if f"/{ep}/" in k and not k.endswith("/error"))
    n_err = sum(1 for k in rec if f"/{ep}/" in k and k.endswith("/error"))
    print(f"{ep}: {n_ok // 2} calls recorded, {n_err} refusals")
    assert n_ok > 0, f"no successful recording of {ep}"
assert not cases.UNEXPECTED, "the parent refused calls the cases expect to succeed (or the reverse)"
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "moment_replays_parent.npz")
np.savez_compressed(out, **rec)
print("recorded", len(rec), "entries,", os.path.getsize(out), "bytes, library", cases.rat.SO_PATH)
