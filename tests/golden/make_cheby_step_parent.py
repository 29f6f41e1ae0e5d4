"""Writes the fixture of tests/test_gpu_cheby_step_parent.py: per case the digest, the counters of one step and the split getters.
Run on the MI355X against the build of the commit BEFORE the change under test (QPROP_HIP_LIB names that build's
libqprop_hip.so; the cases and the records come from the test file itself):

    QPROP_HIP_LIB=/path/to/parent/libqprop_hip.so python tests/golden/make_cheby_step_parent.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cheby_step_parent.json"))
    args = ap.parse_args()
    import test_gpu_cheby_step_parent as T
    ctx = T.L.Context(0)
    out = {}
    for name, make in T.STEP_CASES.items():
        out[name] = json.loads(json.dumps(make(ctx)))
        print(name, out[name], flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
