#!/usr/bin/env python3
"""Cost of the ray-distortion regulariser (csrc/render_distort.hip: das3r_raster_distortion_forward / das3r_raster_distortion_backward)
beside its yardstick, das3r_raster_aux_backward at C = 1 of the same forward, in one process.

    python tools/distortion_bench.py [--shapes c4,sintel] [--warmup 3] [--repeats 20] [--out profiles/distortion.json]
Shapes: tools/aux_bench.py's — `c4`, 1 M random splats at 1920x1080, SH degree 3 (bench.py's flagship workload); `sintel`, the DAS3R
training shape, 512x208 with one Gaussian per pixel of 22 frames (2.34 M Gaussians, few tiles, ~11 k-entry lists).
Per shape one forward is kept (its saved state is what all three read); then `warmup` rounds of everything and `repeats` rounds in which the
three measurements ALTERNATE (a drift of the clocks hits all of them alike), each bracketed by the library's own HIP events (das3r_profile_*),
every kernel of a call summed:
  (a) distortion_of(state): render_distortion_forward_kernel alone;
  (b) the distortion backward: render_distortion_backward_kernel + distortion_fold_kernel + the per-Gaussian backward (the compositing
      kernel's own time is listed as well);
  (c) das3r_raster_aux_backward at C = 1 without dL_dfeatures: render_aux_backward_kernel + the per-Gaussian backward — the same lists, the
      same reductions, less one reduced value and two running sums.
Medians and min / max over the rounds go to stdout and, with --out, into a JSON file.  Expectation (docs/ledger.md (cq)): the distortion
backward at parity to about 1.5x of (c); a record, not a gate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402


def measure(name, dev, warmup, repeats):
    from aux_bench import shape_inputs
    from das3r_amd import _lib
    from das3r_amd.rasterizer import RasterState, _aux_backward_impl, _distortion_backward_impl, _distortion_forward, _forward_full
    rs, t, _ = shape_inputs(name, dev)
    e = torch.empty(0, device=dev)
    P, H, W = t["means3D"].shape[0], int(rs.image_height), int(rs.image_width)
    g = torch.Generator().manual_seed(2)
    feat = torch.rand(P, 1, generator=g).to(dev)
    G = (torch.randn(1, H, W, generator=g) / (H * W)).to(dev)
    _lib.forget_shapes()

    def forward():
        return _forward_full(rs, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e)

    for _ in range(3):   # the library settles on the shape's binning path and kernels
        forward()
    res = forward()
    state = RasterState.of(res, rs)
    totals = _distortion_forward(state, True)[1]

    calls = {
        "distortion_forward": lambda: _distortion_forward(state, True),
        "distortion_backward": lambda: _distortion_backward_impl(state, rs, G, totals, t["means3D"], t["sh"], e, t["opacities"], t["scales"],
                                                                 t["rotations"], e),
        "aux_backward_c1": lambda: _aux_backward_impl(state, rs, feat, G, None, False, t["means3D"], t["sh"], e, t["opacities"], t["scales"],
                                                      t["rotations"], e),
    }
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()

    def timed(fn):
        _lib.profile_report()
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        return {k: ms for k, (_, ms) in _lib.profile_report().items()}

    rows = {k: [] for k in list(calls) + ["distortion_backward_kernel", "aux_backward_kernel_c1"]}
    for _ in range(repeats):
        for k, fn in calls.items():
            r = timed(fn)
            rows[k].append(sum(r.values()))
            if k == "distortion_backward":
                rows["distortion_backward_kernel"].append(r["render_distortion_backward_kernel"])
            elif k == "aux_backward_c1":
                rows["aux_backward_kernel_c1"].append(r["render_aux_backward_kernel"])
    med = {k: round(statistics.median(v), 5) for k, v in rows.items()}
    spread = {k: [round(min(v), 5), round(max(v), 5)] for k, v in rows.items()}
    ratios = {"distortion_backward_over_aux_backward_c1": round(med["distortion_backward"] / med["aux_backward_c1"], 3),
              "distortion_backward_kernel_over_aux_backward_kernel_c1": round(med["distortion_backward_kernel"] / med["aux_backward_kernel_c1"], 3),
              "distortion_forward_over_aux_backward_kernel_c1": round(med["distortion_forward"] / med["aux_backward_kernel_c1"], 3)}
    return dict(shape=name, P=P, W=W, H=H, num_rendered=int(res[0]), mean_list=round(int(res[0]) / (((W + 15) // 16) * ((H + 15) // 16)), 1),
                warmup=warmup, repeats=repeats, median_ms=med, min_max_ms=spread, ratios=ratios)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,sintel")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev),
           "what": "tools/distortion_bench.py: HIP-event times, every kernel of a call summed, medians over alternating repeats after a warm-up", "shapes": []}
    for name in args.shapes.split(","):
        row = measure(name, dev, args.warmup, args.repeats)
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
