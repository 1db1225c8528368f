#!/usr/bin/env python3
"""
Per-chunk timeline of the default bench from a rocprofv3 trace.

    rocprofv3 --kernel-trace --memory-copy-trace --stats -d OUT -o run -f csv -- \
        python bench.py --gpus 1 --steps 20 --warmup 5
    python scripts/scan_gap_summary.py OUT [--skip N]

For consecutive gpuscan_qual_column* dispatches: the scan's duration, the gap
from one scan's end to the next scan's start, and every dispatch or copy that
starts inside such a gap (name, queue id).  --skip drops the first N scans
(the warm-up steps).

Resident scans alternate over two streams, so a scan's dispatch can begin
before the previous one has ended.  Such a boundary has no gap: it counts as an
overlap (previous end - this start; the start stamp is taken when the packet
is processed, not when the first wave gets a CU).  What compares across both
cases is the span per chunk, end(N) - end(N-1): without overlap it is the
duration plus the gap.
"""
import argparse
import collections
import csv
import glob
import os
import statistics


def load(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def short(name):
    return name if len(name) <= 60 else name[:57] + "..."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--skip", type=int, default=50)
    ap.add_argument("--kernel", default="gpuscan_qual_column")
    args = ap.parse_args()

    kpath = sorted(glob.glob(os.path.join(args.outdir, "**", "*kernel_trace.csv"), recursive=True))
    cpath = sorted(glob.glob(os.path.join(args.outdir, "**", "*memory_copy_trace.csv"), recursive=True))
    events = []
    for r in load(kpath[0]):
        events.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                       "q%s" % r["Queue_Id"]))
    for p in cpath[:1]:
        for r in load(p):
            events.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                           "copy " + r.get("Direction", "?"), "dma"))
    events.sort()
    scans = [e for e in events if e[2].startswith(args.kernel)]
    scans = scans[args.skip:]
    if len(scans) < 2:
        print("fewer than two scans after --skip")
        return
    durs = [(e[1] - e[0]) * 1e-3 for e in scans]
    gaps, overlaps, spans = [], [], []
    inside = collections.Counter()
    for a, b in zip(scans, scans[1:]):
        spans.append((b[1] - a[1]) * 1e-3)
        if b[0] < a[1]:
            overlaps.append((min(a[1], b[1]) - b[0]) * 1e-3)
            continue
        gaps.append((b[0] - a[1]) * 1e-3)
        for e in events:
            if a[1] <= e[0] < b[0]:
                inside[(short(e[2]), e[3])] += 1
    queues = collections.Counter(e[3] for e in scans)
    switches = sum(1 for a, b in zip(scans, scans[1:]) if a[3] != b[3])
    print("trace: %s" % os.path.relpath(kpath[0], args.outdir))
    print("scans: %d (after skipping %d), queues %s" % (len(scans), args.skip, dict(queues)))
    print("%s duration us: median %.1f  mean %.1f  min %.1f  max %.1f"
          % (args.kernel, statistics.median(durs), statistics.mean(durs), min(durs), max(durs)))
    print("boundaries: %d, the queue id changes at %d of them" % (len(spans), switches))
    print("span per chunk end->next end us: median %.1f  mean %.1f  min %.1f  max %.1f"
          % (statistics.median(spans), statistics.mean(spans), min(spans), max(spans)))
    print("overlapping boundaries (next start before this end): %d of %d" % (len(overlaps), len(spans)))
    if overlaps:
        print("overlap next start->this end us: median %.1f  mean %.1f  min %.1f  max %.1f"
              % (statistics.median(overlaps), statistics.mean(overlaps), min(overlaps), max(overlaps)))
    if not gaps:
        print("no boundary with a gap")
        return
    print("gap end->next start us: median %.1f  mean %.1f  min %.1f  max %.1f"
          % (statistics.median(gaps), statistics.mean(gaps), min(gaps), max(gaps)))
    q = sorted(gaps)
    print("gap percentiles us: p10 %.1f  p50 %.1f  p90 %.1f"
          % (q[len(q) // 10], q[len(q) // 2], q[(9 * len(q)) // 10]))
    print("starts inside the %d gaps (name, queue: count):" % len(gaps))
    if not inside:
        print("  (none)")
    for (name, queue), n in sorted(inside.items(), key=lambda kv: -kv[1]):
        print("  %-60s %-4s %d" % (name, queue, n))


if __name__ == "__main__":
    main()
