"""Records tests/golden/stacked_operands_parent.npz: what the fused one-wavefront-per-sample solve computes on the workloads of
tests/stacked_operands_cases.py WITHOUT the stacked operands.  It was run on an MI355X against the library built from the commit before the
switch lq_replay_stack existed (RATILQR_SO pointing at that build), and must only ever be re-run against such a build:
the file is what "switch off selects the old code" is tested against, so it may not come from the tree under test.

    RATILQR_SO=<library of the parent commit> python tests/golden/make_stacked_operands_golden.py [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import stacked_operands_cases as cases  # noqa: E402

fused = cases.run({}, "fused")
rounds = cases.run({}, "rounds")
full = cases.run({"lq_replay": 0}, "fused")
for k in sorted(fused):
    for other, what in ((rounds, "the round-based path"), (full, "lq_replay = 0")):
        if not k.endswith("/counts") and not np.array_equal(fused[k], other[k], equal_nan=True):
            print("the fused path and", what, "differ on", k)
np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "stacked_operands_parent.npz"), **fused)
print("recorded", len(fused), "arrays;", {k: v.tolist() for k, v in fused.items() if k.endswith("/counts")})
