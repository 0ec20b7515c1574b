"""Generate tests/golden/predict_reject_codes.json: what the latent predictors' entry points return for every bad
argument, pair of bad arguments and workspace-size query of tests/test_predict_reject_cpu.py (which holds the cases;
this script only runs them and writes the answers down).

The recording is of a PARENT build, not of the tree it is checked against: build the commit before the change under
test into a directory of its own and point LVAE_LIB at its liblvae_hip.so.  No GPU is needed (every call is rejected
before any launch); a case the library accepts is an error here, not a recording.

Usage:  LVAE_LIB=/path/to/parent/liblvae_hip.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_predict_reject.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "longitudinal-vae_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import test_predict_reject_cpu as T  # noqa: E402

if __name__ == "__main__":
    if "LVAE_LIB" not in os.environ:
        sys.exit("set LVAE_LIB to the parent build's liblvae_hip.so")
    table = T.record(T.P.load())
    for name, codes in table["codes"].items():
        bad = {cid: c for cid, c in codes.items() if not -24 <= c <= -1}
        assert not bad, (name, bad)
    with open(T.GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in table["codes"].items()}, {k: len(v) for k, v in table["sizes"].items()})
