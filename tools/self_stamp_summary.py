#!/usr/bin/env python3
"""Developer tool: summary of one self-collision launch of a stamp build (tools/build_variant.py NAME -DVMV_SELF_STAMP;
the launcher writes the file named by VMV_SELF_STAMP_OUT, overwritten per launch).
File: 4 uint64 of header (n, group, workgroups, shared passes 1 / per-wave 0), then 4 uint64 per wave: s_memrealtime at
entry, at the end of the wave's last pass and at exit; passes | XCC_ID << 16 | HW_ID << 32.
usage: tools/self_stamp_summary.py FILE [FILE ...]"""
import sys

import numpy as np

TICK_US = 0.01  # s_memrealtime: 100 MHz


def pct(a, ps=(0, 10, 50, 90, 100)):
    return " ".join(f"p{p}={np.percentile(a, p):.1f}" for p in ps)


def summary(path):
    raw = np.fromfile(path, dtype=np.uint64)
    n, group, blocks, shared = (int(x) for x in raw[:4])
    rec = raw[4:].reshape(-1, 4)
    rec = rec[rec[:, 0] != 0]  # (waves of workgroups that never ran a share: none in a one-generation grid)
    t0 = rec[:, 0].astype(np.int64)
    base = t0.min()
    start = (t0 - base) * TICK_US
    work_end = (rec[:, 1].astype(np.int64) - base) * TICK_US
    end = (rec[:, 2].astype(np.int64) - base) * TICK_US
    meta = rec[:, 3]
    passes = (meta & 0xFFFF).astype(np.int64)
    xcc = ((meta >> 16) & 0xF).astype(np.int64)
    hw = (meta >> 32).astype(np.int64)
    cu, sh, se = (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    span = end.max()
    life = end - start
    work = work_end - start
    out = [f"== {path}: n={n} group={group} workgroups={blocks} kernel={'shared passes' if shared else 'per-wave groups'}",
           f"waves stamped {len(rec)}; launch span (first entry -> last exit) {span:.1f} us",
           f"wave entry  (us after the first): {pct(start)}",
           f"wave life   (entry -> exit, us):  {pct(life)}   mean {life.mean():.1f}",
           f"wave work   (entry -> last pass): {pct(work)}   mean {work.mean():.1f}",
           "passes per wave: " + " ".join(f"{p}:{c}" for p, c in zip(*np.unique(passes, return_counts=True)))]
    # generations: entries later than the earliest exit can only be waves that waited for a slot
    late = start > end.min()
    out.append(f"waves entering after the first exit ({end.min():.1f} us): {int(late.sum())}")
    # workgroups per CU (the CU a workgroup ran on: its waves' XCC, SE, SH, CU)
    cu_key = xcc * 1000 + se * 100 + sh * 16 + cu
    keys = cu_key[::4] if len(rec) % 4 == 0 else cu_key  # records are in global wave order, 4 waves per workgroup
    _, per_cu = np.unique(keys, return_counts=True)
    out.append(f"CUs used {len(per_cu)}; workgroups per CU: " +
               " ".join(f"{k}:{c}" for k, c in zip(*np.unique(per_cu, return_counts=True))))
    # concurrency: resident waves over time
    ev = np.concatenate([np.stack([start, np.ones_like(start)], 1), np.stack([end, -np.ones_like(end)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    live = np.cumsum(ev[:, 1])
    peak = int(live.max())
    out.append(f"peak resident waves {peak}; slot-time used = sum(life) / (peak x span) = {life.sum() / (peak * span):.1%}")
    t = np.linspace(0, span, 11)
    live_at = [int(((start <= x) & (end > x)).sum()) for x in t[:-1]]
    out.append("resident waves at 0 %, 10 %, .. 90 % of the span: " + " ".join(map(str, live_at)))
    if len(rec) % 4 == 0:
        we = work_end.reshape(-1, 4)
        lf = life.reshape(-1, 4)
        out.append(f"within a workgroup, last minus first end of work (us): {pct(we.max(1) - we.min(1))}")
        out.append(f"within a workgroup, longest minus shortest life (us): {pct(lf.max(1) - lf.min(1))}")
        out.append(f"workgroup exit (us): {pct(end.reshape(-1, 4).max(1))}")
    return "\n".join(out)


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print(summary(p))
