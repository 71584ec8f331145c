"""Generator of tests/golden/conv_stats_rows.json: the statistics rows the C ABI's query-only calls (lbc_conv2d_fwd /
lbc_deconv3x3s2_fwd with a NULL output: nothing is launched) answer for the grid of tests/test_conv_rows.py, under every option set
of that grid, on the CPU-emulated build of the kernel sources (the planner is host code: the gfx950 library answers the same).

The committed table was recorded at the commit BEFORE the convolution call sites moved to the shared descriptor builders and
lbc_igemm_plan; tests/test_conv_rows.py holds every later tree to it.  Regenerate only with a deliberate change of the tile policy:

    python tests/golden/make_conv_rows_fixture.py [--lib path/to/liblbc_emu.so]     # rewrites tests/golden/conv_stats_rows.json

The file holds recorded results only: one list of row counts per option set, in the order of test_conv_rows.cases().
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="an emulated build to record from (default: build and load this tree's tests/emu)")
    args = ap.parse_args()
    from learningbycheating_amd import _lib
    from tests import emu
    from tests import test_conv_rows as T
    lib = _lib._inject_for_tests(ctypes.CDLL(args.lib)) if args.lib else emu.activate()
    assert lib.lbc_backend().decode() == "emu-cpu"
    table = []
    for opts in T.OPTIONS:
        for name, value in opts:
            _lib.config_set(name, value)
        table.append(T.query_rows(lib))
        for name, _ in opts:
            _lib.config_set(name, -1)
    out = {"cases_digest": T.cases_digest(), "cases": len(T.cases()), "options": [[list(o) for o in opts] for opts in T.OPTIONS], "rows": table}
    path = os.path.join(HERE, "conv_stats_rows.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d option sets x %d launches, %d distinct row counts" % (path, len(table), len(table[0]), len({r for t in table for r in t})))


if __name__ == "__main__":
    main()
