#!/usr/bin/env python3
"""What running the SH colour kernel on a side stream beside the binning kernels costs and hides, from two rocprofv3 --kernel-trace dumps
of the same workload: one with DAS3R_SPLIT_COLOUR=0 (the fused preprocess, everything on one stream) and one with the split on.

    DAS3R_SPLIT_COLOUR=0 rocprofv3 --kernel-trace -d off -o kt --output-format csv -- python bench.py
    DAS3R_SPLIT_COLOUR=1 rocprofv3 --kernel-trace -d on  -o kt --output-format csv -- python bench.py
    python tools/probes/split_colour_overlap.py off on

Prints (a) by how much every kernel of the caller's stream between the per-Gaussian kernel and the compositing forward ran longer beside
the colour kernel, (b) how long the colour kernel took there, (c) what the fork (event record behind the geometry kernel) and the join
(stream wait in front of the compositing kernel) cost on the caller's stream: the idle time in front of the first binning kernel and in
front of the compositing kernel, against the same gaps without the split; and the forward's critical path either way."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stream_timeline import load_steps  # noqa: E402


def mean(steps, fn):
    return sum(fn(s) for s in steps) / len(steps) / 1e3


def main():
    names_off, off = load_steps(sys.argv[1])
    names_on, on = load_steps(sys.argv[2])
    side = [i for i, n in enumerate(names_on) if n == "sh_colour_kernel"]
    if len(side) != 1 or "sh_colour_kernel" in names_off:
        raise SystemExit("expected the first trace without and the second with exactly one sh_colour_kernel per step")
    c = side[0]
    main_on = [i for i in range(len(names_on)) if i != c]
    if [names_on[i] for i in main_on][1:] != list(names_off)[1:]:
        raise SystemExit("the two traces do not launch the same kernels on the caller's stream")
    fwd = next(k for k, i in enumerate(main_on) if names_on[i].startswith("render_forward"))
    print(f"{'kernel':40s} {'fused us':>9s} {'split us':>9s} {'diff':>7s}")
    slow = 0.0
    for k, i in enumerate(main_on):
        a = mean(off, lambda s: s[k][1] - s[k][0])
        b = mean(on, lambda s: s[i][1] - s[i][0])
        print(f"{names_on[i][:40]:40s} {a:9.1f} {b:9.1f} {b - a:+7.1f}")
        if 0 < k < fwd:
            slow += b - a
    print(f"(a) the binning kernels ran {slow:+.1f} us longer beside the colour kernel")
    print(f"(b) sh_colour_kernel took {mean(on, lambda s: s[c][1] - s[c][0]):.1f} us "
          f"(started {mean(on, lambda s: s[c][0] - s[main_on[0]][1]):.1f} us behind the geometry kernel's end)")
    gap = lambda steps, idx, k: mean(steps, lambda s: s[idx[k]][0] - s[idx[k - 1]][1])   # noqa: E731
    all_off = list(range(len(names_off)))
    fork = gap(on, main_on, 1) - gap(off, all_off, 1)
    join = gap(on, main_on, fwd) - gap(off, all_off, fwd)
    print(f"(c) fork: {fork:+.1f} us of idle stream in front of the first binning kernel; join: {join:+.1f} us in front of the compositing kernel")
    path_off = mean(off, lambda s: s[fwd][0] - s[0][0])
    path_on = mean(on, lambda s: s[main_on[fwd]][0] - s[0][0])
    print(f"forward critical path up to the compositing kernel: {path_off:.1f} -> {path_on:.1f} us ({path_on - path_off:+.1f})")


if __name__ == "__main__":
    main()
