#!/usr/bin/env python3
"""Per-step kernel timeline from a rocprofv3 --kernel-trace CSV dump, for steps whose kernels run on MORE THAN ONE stream (the split
preprocess: das3r_amd/csrc/forward.hip Join).  tools/timeline.py adds durations and gaps along one in-order stream; here every kernel
of a step is placed by its start and end stamps relative to the step's first kernel, so that a kernel that runs beside others shows as
an interval, and the step's critical path is read off the stamps instead of summed.

    python tools/stream_timeline.py <dir with *_kernel_trace.csv> [--steps N]

Prints, averaged over the last N steady-state steps (default 8): per kernel (in order of start) start, end, duration and the queue it
ran on; then the span of the forward (first kernel start -> compositing forward start and end), of the whole step, and the sum of the
kernel durations (equal to the span when nothing overlaps and nothing idles)."""
import argparse
import csv
import glob
import re
from collections import defaultdict

FIRST = ("preprocess_kernel", "preprocess_geometry_kernel")


def short(name):
    base = name.split("(")[0].replace("void ", "").replace("das3r::", "")
    m = re.match(r"preprocess_kernel<([^>]*)>", base)
    if m and [t.strip() for t in m.group(1).split(",")][4:5] == ["true"]:
        return "preprocess_geometry_kernel"   # (preprocess.hip: the geometry kernel is the fifth-flag instantiation of preprocess_kernel)
    return base.split("<")[0]


def load_steps(directory, last=8):
    """-> (kernel names of the commonest forward + backward step, the last `last` such steps as lists of (start, end, name, queue))."""
    rows = []
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?")))
    rows.sort()
    steps, cur = [], []
    for r in rows:
        if r[2] in FIRST and cur:
            steps.append(cur)
            cur = []
        cur.append(r)
    steps.append(cur)
    steps = [s for s in steps if s[0][2] in FIRST and any(x[2].startswith("render_backward") for x in s)]
    if not steps:
        raise SystemExit("no forward + backward step found in the trace")
    shape = defaultdict(int)
    for s in steps:
        shape[tuple(x[2] for x in s)] += 1
    common = max(shape, key=shape.get)
    return common, [s for s in steps if tuple(x[2] for x in s) == common][-last:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    common, steps = load_steps(args.dir, args.steps)
    n = len(steps)
    print(f"{n} steady-state steps of {len(common)} kernels each (us, relative to the start of the step's first kernel)")
    queues = sorted({x[3] for s in steps for x in s})
    print(f"queues seen: {', '.join(queues)}")
    total_dur = 0.0
    fwd_start = fwd_end = None
    for i, name in enumerate(common):
        a = sum(s[i][0] - s[0][0] for s in steps) / n / 1e3
        b = sum(s[i][1] - s[0][0] for s in steps) / n / 1e3
        d = sum(s[i][1] - s[i][0] for s in steps) / n / 1e3
        q = steps[-1][i][3]
        total_dur += d
        if name.startswith("render_forward"):
            fwd_start, fwd_end = a, b
        print(f"{i:3d} {name[:44]:44s} start {a:8.1f}  end {b:8.1f}  dur {d:7.1f}  queue {q}")
    span = sum(max(x[1] for x in s) - s[0][0] for s in steps) / n / 1e3
    if fwd_start is not None:
        print(f"first kernel start -> compositing forward start {fwd_start:.1f} us, -> its end {fwd_end:.1f} us")
    print(f"step span {span:.1f} us, sum of kernel durations {total_dur:.1f} us")
    if len(steps) > 1:
        period = (steps[-1][0][0] - steps[0][0][0]) / (n - 1) / 1e3
        print(f"step period (start to start) {period:.1f} us")


if __name__ == "__main__":
    main()
