"""Records tests/golden/event_sums_parent.npz: what rat_policy_events / _user and rat_policy_tail_events / _user (the tail calls under the
switch tail_dense too) compute on the cases of tests/event_sum_cases.py BEFORE ev_sums / tle_sums and ev_final / tle_final shared one body
each (csrc/policy_mc.hip: ev_sums_body<TAIL>, ev_final_body<TAIL>) and the 12 + 4 event tile was placed by one helper (csrc/driver.cpp).
It was run on an MI355X against the library built from the commit before that change (RATILQR_SO pointing at that build), and must only
ever be re-run against such a parent build: the file is what "the shared body changed no bit" is tested against, so it may not come from
the tree under test.

    RATILQR_SO=<library of the parent commit> python tests/golden/make_event_sums_golden.py [output.npz]

Prints every refusal a case did not expect (and every success where it expected a refusal) as UNEXPECTED, and fails unless there is none
and every entry point has at least one successful recording and one refusal."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import event_sum_cases as cases  # noqa: E402

rec = {}
for name in cases.CASES:
    t0 = time.perf_counter()
    rec.update(cases.run(name))
    print(f"{name}: {time.perf_counter() - t0:.2f} s", flush=True)
for line in cases.UNEXPECTED:
    print("UNEXPECTED", line)
for ep in cases.ENTRY_POINTS:
    n_ok = sum(1 for k in rec if f"/{ep}/" in k and k.endswith("/values"))
    n_err = sum(1 for k in rec if f"/{ep}/" in k and k.endswith("/error"))
    print(f"{ep}: {n_ok} calls recorded, {n_err} refusals")
    assert n_ok > 0 and n_err > 0, f"no successful recording or no refusal of {ep}"
for ep in cases.TAIL_ENTRY_POINTS:
    assert any(f"/{ep}/" in k and k.endswith("_dense/values") for k in rec), f"no recording of {ep} under tail_dense"
assert not cases.UNEXPECTED, "the parent refused calls the cases expect to succeed (or the reverse)"
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "event_sums_parent.npz")
np.savez_compressed(out, **rec)
print("recorded", len(rec), "entries,", os.path.getsize(out), "bytes, library", cases.rat.SO_PATH)
