"""Records tests/golden/engine_lowering.json: the CPU launch trace (tests/lowering_trace.py) of
the engine's conv / linear lowering at the commit that is checked out, with that commit's hash.

    python tests/golden/make_golden_lowering.py

Run it at the commit whose lowering is the reference (the parent of a change that must not move
a launch), with the package unmodified and the library built: the fixture also lists the gemm
calls that fs2_gemm_plan refuses or whose requested split-K slice count it does not keep
(``plan_exceptions``); tests/test_lowering_host.py expects exactly those."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lowering_trace as L  # noqa: E402


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    git = lambda *a: subprocess.check_output(("git", "-C", root) + a, text=True).strip()  # noqa: E731
    if git("status", "--porcelain", "--", L.PKG):
        sys.exit("the package differs from the checked-out commit: record from a clean one")
    gemms = {}
    cases = L.trace(gemms)
    fx = {"recorded_from": git("rev-parse", "--short=7", "HEAD"),
          "plan_exceptions": sorted(L.split_mismatches(gemms)),
          "cases": cases}
    with open(os.path.join(HERE, "engine_lowering.json"), "w") as f:
        # one case a line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in fx.items()
                                    if k != "cases"))
        f.write(',\n"cases": {\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}"
                                               for k, v in cases.items()) + "\n}}\n")
    print(len(cases), "cases,", len(fx["plan_exceptions"]), "plan exceptions")


if __name__ == "__main__":
    main()
