"""Smallest conv2d shape per plan form, for the case tables of tests/exact_support.py (host only: gz_conv2d_plan needs no
GPU).  Enumerates N, C, H, K over the four layer geometries in all three directions and prints, per (plan form, split /
unsplit), the shape with the fewest multiply-adds; forms that tests/golden/dispatch_plan.json or the current table name
and the enumeration does not reach are listed at the end.

    python tools/find_exact_cases.py [max multiply-adds, default 1.5e10]
    python tools/find_exact_cases.py --rect [max]     the rows of _RECT_TABLE (rectangular maps, H != W)
    python tools/find_exact_cases.py --box [max]      the rows of _BOX3_TABLE (conv3d on boxes that are no cubes)

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


def rect(max_macs):
    """One row per key: the mid-tile shape where the key has one, else the cheapest rectangle; the orientation alternates
    down the sorted keys (neighbours are the split / unsplit launches and the tiles of one loader family) unless the
    other orientation is more than twice cheaper."""
    both = S.enumerate_rect_plans(max_macs)
    side = {o: S.enumerate_rect_plans(max_macs, o) for o in ("tall", "wide")}
    rows, mids = [], 0
    for i, key in enumerate(sorted(both)):
        which = 1 if both[key][1] is not None else 0
        order = ("tall", "wide") if i % 2 == 0 else ("wide", "tall")
        cands = [side[o][key][which] for o in order if key in side[o] and side[o][key][which] is not None]
        pick = cands[0] if len(cands) == 1 or cands[0][0] <= 2 * cands[1][0] else cands[1]
        mids += which
        rows.append((pick, key, which))
    # every loader family in both orientations, per direction: where one is missing, turn the row that pays least for it
    for fam in S.LOADER_FAMILIES:
        for op in S.OPS:
            idx = [i for i, (pick, key, _) in enumerate(rows) if pick[2] == op and S.loader_family(key[0]) == fam]
            for want in ("tall", "wide"):
                if idx and not any(S.orientation(rows[i][0][1]) == want for i in idx):
                    swaps = [(side[want][rows[i][1]][rows[i][2]][0] / rows[i][0][0], i) for i in idx
                             if rows[i][1] in side[want] and side[want][rows[i][1]][rows[i][2]] is not None]
                    if swaps:
                        _, i = min(swaps)
                        rows[i] = (side[want][rows[i][1]][rows[i][2]], rows[i][1], rows[i][2])
                        continue
                    # no row can turn without losing its mid-tile shape: a second row for the cheapest key that can
                    extra = [(side[want][rows[i][1]][0], rows[i][1], 0) for i in idx if rows[i][1] in side[want]]
                    if extra:
                        rows.append(min(extra))
    for n, ((macs, shape, op), (form, split), which) in enumerate(rows):
        note = "" if which else ("   no mid-tile rectangle" if n < len(both) else
                                 "   second row of its key: the family's other orientation, which has no mid-tile shape")
        if macs > 3e9:
            sq = [S.case_macs(r[0]) for r in S.CONV_ROWS if (r[2], r[3]) == (form, split)]
            if sq and min(sq) < macs:
                note += "   (a square row of this key has %.3g)" % min(sq)
        print("    (%r, %r, %r, %r),        # %.3g multiply-adds%s" % (shape, op, form, split, macs, note))
    tall = sum(1 for (m, sh, op), _, _ in rows if sh[2] > sh[3])
    print("# %d rows for %d keys, %d of the keys mid-tile; %d tall (H > W), %d wide"
          % (len(rows), len(both), mids, tall, len(rows) - tall))
    for key in sorted({(r[2], r[3]) for r in S.CONV_ROWS} - set(both)):
        print("not reached by a rectangle: %r split=%r" % key)


def box(max_macs):
    best = S.enumerate_box_plans(max_macs)
    for form, (cheapest, mid) in sorted(best.items()):
        macs, shape, op = mid or cheapest
        print("    (%r, %r, %r),        # %.3g multiply-adds%s" % (shape, op, form, macs, "" if mid else "   no mid-tile box"))
    print("# %d forms, %d of them mid-tile" % (len(best), sum(1 for v in best.values() if v[1])))
    for form in sorted({r[2] for r in S.CONV3_ROWS} - set(best)):
        print("not reached by a box:", form)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    cap = float(args[0]) if args else 1.5e10
    if "--rect" in sys.argv:
        rect(cap)
    elif "--box" in sys.argv:
        box(cap)
    else:
        main(cap)
