"""Writes the fixture of tests/test_gpu_plans_parent.py: the plans of its named operators as the C ABI's getters report them, and the
digest of its panel step.  Run on the MI355X against the build of the commit BEFORE the change under test (QPROP_HIP_LIB names that
build's libqprop_hip.so; the operators and the record come from the test file itself):

    QPROP_HIP_LIB=/path/to/parent/libqprop_hip.so python tests/golden/make_plans_parent.py [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plans_parent.json"))
    args = ap.parse_args()
    import test_gpu_plans_parent as T
    ctx = T.L.Context(0)
    out = {"operators": {name: T.plan_record(ctx, name) for name in T.OPERATORS},
           "panel_step": T.panel_step(ctx)}
    ctx.close()
    assert out["panel_step"]["tiles"] == out["panel_step"]["rows"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
