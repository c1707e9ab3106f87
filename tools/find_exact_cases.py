"""Smallest conv2d shape per plan form, for the case table of tests/exact_support.py (host only: gz_conv2d_plan needs no
GPU).  Enumerates N, C, H, K over the four layer geometries in all three directions and prints, per (plan form, split /
unsplit), the shape with the fewest multiply-adds; forms that tests/golden/dispatch_plan.json or the current table name
and the enumeration does not reach are listed at the end.

    python tools/find_exact_cases.py [max multiply-adds, default 1.5e10]

After a deliberate threshold change: take the printed row for every case that tests/test_exact_cases.py reports as moved
off its kernel."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import exact_support as S      # noqa: E402


def main(max_macs):
    best = S.enumerate_plans(max_macs)
    have = {(row[2], row[3]) for row in S.CONV_ROWS}
    for (form, split), (macs, shape, op) in sorted(best.items()):
        print("    (%r, %r, %r, %r),        # %.3g multiply-adds%s" % (shape, op, form, split, macs,
                                                                    "" if (form, split) in have else "   <-- no row"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_plan.json")))
    want = {S.plan_form(v) for cfg in golden.values() for v in cfg.values() if "3D" not in v and "igemm2r" not in v}
    want |= {row[2] for row in S.CONV_ROWS}
    for form in sorted(want - {f for f, _ in best}):
        print("not reached:", form)


if __name__ == "__main__":
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 1.5e10)
