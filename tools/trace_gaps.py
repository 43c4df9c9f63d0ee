#!/usr/bin/env python3
"""GPU idle time inside the bench's steps from a rocprofv3 --kernel-trace CSV: union of the kernels' [start, end) intervals against
the span, and the largest gaps with the kernels on both sides; then how far consecutive steps overlap (option "forward_lanes").
usage: trace_gaps.py <dir with *kernel_trace.csv> [n_gaps]"""
import csv
import glob
import sys

rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"][:60], r.get("Stream_Id") or r.get("Queue_Id")))
rows.sort()
# the timed region: from the first kernel after the longest gap (warm-up / parity passes end there) -- simply take the last 40 %
t_lo = rows[int(len(rows) * 0.6)][0]
rows = [r for r in rows if r[0] >= t_lo]
span = rows[-1][1] - rows[0][0]
busy, cur_s, cur_e, gaps, last_name = 0, rows[0][0], rows[0][1], [], rows[0][2]
for s, e, n, _ in rows[1:]:
    if s > cur_e:
        busy += cur_e - cur_s
        gaps.append((s - cur_e, last_name, n))
        cur_s, cur_e = s, e
    else:
        cur_e = max(cur_e, e)
    if e >= cur_e:
        last_name = n
busy += cur_e - cur_s
print(f"{len(rows)} kernels over {span / 1e6:.2f} ms: GPU busy {busy / 1e6:.2f} ms = {100 * busy / span:.2f} %, idle {100 * (1 - busy / span):.2f} % in {len(gaps)} gaps")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
agg = {}
for g, a, b in gaps:
    k = (a, b)
    agg[k] = (agg.get(k, (0, 0))[0] + g, agg.get(k, (0, 0))[1] + 1)
for (a, b), (g, c) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:n]:
    print(f"  {g / 1e3:9.1f} us in {c:4d} gaps   {a}  ->  {b}")

# Steps: on its stream a forward runs from stem_pack to roi_final, and RoIPool starts its head.  Per step: its span, and
# how many of its kernels before the head (backbone, RPN head, proposals; those on the forward's own stream -- the
# second halves of res3 / res4 run on the shared side stream and are not counted) start before the previous step's
# roi_final has ended.  One stream: the steps follow each other and the count is 0.
steps, open_ = [], {}
for s, e, n, q in rows:
    if "stem_pack" in n:
        open_[q] = {"start": s, "pre": [s], "head": None}
    elif q in open_:
        st = open_[q]
        if "roi_pool" in n and st["head"] is None:
            st["head"] = s
        if st["head"] is None:
            st["pre"].append(s)
        if "roi_final" in n:
            st["end"] = e
            steps.append(open_.pop(q))
steps.sort(key=lambda st: st["start"])
if len(steps) > 1:
    early = [sum(1 for t in b["pre"] if t < a["end"]) for a, b in zip(steps, steps[1:])]
    spans = [(st["end"] - st["start"]) / 1e6 for st in steps]
    period = (steps[-1]["end"] - steps[0]["end"]) / 1e6 / (len(steps) - 1)
    print(f"{len(steps)} whole steps: span {sum(spans) / len(spans):.2f} ms each (sum {sum(spans):.2f} ms), one step ends every {period:.2f} ms; "
          f"kernels of step i+1 before its head that start before step i ends: {sorted(early)[len(early) // 2]} (median), "
          f"{min(early)} .. {max(early)} of {len(steps[1]['pre'])}")
