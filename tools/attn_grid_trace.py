#!/usr/bin/env python3
"""Per-kernel times of the v2 attention kernels from a rocprofv3 kernel trace
(rocpd sqlite database), split by workgroup order.

Usage: python tools/attn_grid_trace.py <results.db> [--steps N]

A dispatch with grid_size_y > 1 ran the dim3(n_blk, H, B) grid
(MA_ATTN_GRID=legacy), one with a 1-D grid the linear globally heavy-first
order. For fwd2 / dq2 / dkdv2 prints calls, total and mean time per order,
and for the backward pair the union of the two kernels' time intervals (they
co-run on two streams, so the sum of their durations overstates the wall
time). --steps divides the totals into ms per step.
"""

import argparse
import re
import sqlite3

KERNELS = ("fwd2_kernel", "dq2_kernel", "dkdv2_kernel")


def union_ms(intervals):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(intervals):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        tot += cur_e - cur_s
    return tot / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--steps", type=int, default=1)
    args = ap.parse_args()

    c = sqlite3.connect(args.db)
    tabs = [r[0] for r in c.execute(
        "SELECT name FROM sqlite_master WHERE type='table'")]
    disp = next(t for t in tabs if t.startswith("rocpd_kernel_dispatch"))
    sym = next(t for t in tabs if t.startswith("rocpd_info_kernel_symbol"))
    cols = [r[1] for r in c.execute(f"PRAGMA table_info({disp})")]
    gy = "grid_size_y" if "grid_size_y" in cols else \
        next(x for x in cols if "grid" in x and x.endswith("y"))
    rows = c.execute(
        f"SELECT ks.display_name, k.start, k.end, k.{gy} FROM {disp} k "
        f"JOIN {sym} ks ON k.kernel_id = ks.id").fetchall()

    by = {}
    for name, s, e, y in rows:
        kern = next((kn for kn in KERNELS if kn in name), None)
        if kern is None:
            continue
        order = "legacy" if y > 1 else "linear"
        inst = re.sub(r"\(.*", "", name)
        inst = inst[inst.find(kern):]
        by.setdefault((order, kern, inst), []).append((s, e))
    n = args.steps
    print(f"{'order':<7} {'kernel':<34} {'calls':>6} {'total_ms':>10} "
          f"{'ms/step':>9} {'mean_us':>9}")
    for (order, kern, inst), iv in sorted(by.items()):
        ms = sum(e - s for s, e in iv) / 1e6
        print(f"{order:<7} {inst:<34} {len(iv):>6} {ms:>10.2f} {ms / n:>9.2f} "
              f"{1e3 * ms / len(iv):>9.1f}")
    for order in ("legacy", "linear"):
        iv = [x for (o, kern, _), v in by.items()
              if o == order and kern != "fwd2_kernel" for x in v]
        if iv:
            u = union_ms(iv)
            print(f"{order:<7} {'dq2 | dkdv2 union':<34} {'':>6} {u:>10.2f} "
                  f"{u / n:>9.2f}")


if __name__ == "__main__":
    main()
