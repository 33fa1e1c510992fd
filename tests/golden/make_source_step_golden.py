"""Records tests/golden/source_step_parent.npz: what the rollout kernels of source models compute on the cases of
tests/source_step_cases.py BEFORE they took their shared pieces from csrc/source_step.h.  It was run on an MI355X against the library
built from the commit before that change (RATILQR_SO pointing at that build), and must only ever be re-run against such a parent build:
the file is what "the header changed no bit" is tested against, so it may not come from the tree under test.

    RATILQR_SO=<library of the parent commit> python tests/golden/make_source_step_golden.py [output.npz]

Prints every refusal a case did not expect as UNEXPECTED, and fails unless there is none and every call has at least one recording."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import source_step_cases as cases  # noqa: E402

assert os.environ.get("RATILQR_SO"), "RATILQR_SO must name the library of the parent commit"
rec = {}
for name in cases.CASES:
    t0 = time.perf_counter()
    rec.update(cases.run(name))
    print(f"{name}: {time.perf_counter() - t0:.2f} s", flush=True)
for line in cases.UNEXPECTED:
    print("UNEXPECTED", line)
for ep in cases.ENTRY_POINTS:
    n_ok = sum(1 for k in rec if (f"/{ep}/" in k or k.endswith(f"/{ep}/values")) and k.endswith("/values"))
    print(f"{ep}: {n_ok} calls recorded")
    assert n_ok > 0, f"no successful recording of {ep}"
assert not cases.UNEXPECTED, "the parent refused calls the cases expect to succeed"
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "source_step_parent.npz")
np.savez_compressed(out, **rec)
print("recorded", len(rec), "entries,", os.path.getsize(out), "bytes, library", cases.rat.SO_PATH)
