#!/usr/bin/env python3
"""Cost of the median depth and its adjoint (csrc/render_median.hip: das3r_raster_median_forward / das3r_raster_median_adjoint) beside
two calls of the same build over the same lists, in one process.

    python tools/median_bench.py [--shapes c4,sintel] [--warmup 3] [--repeats 20] [--out profiles/median_depth.json]
Shapes: tools/aux_bench.py's — `c4`, 1 M random splats at 1920x1080, SH degree 3 (bench.py's flagship workload); `sintel`, the DAS3R
training shape, 512x208 with one Gaussian per pixel of 22 frames (2.34 M Gaussians, few tiles, ~11 k-entry lists).
Per shape one forward is kept (its saved state is what all four read); then `warmup` rounds of everything and `repeats` rounds in which the
four measurements ALTERNATE (a drift of the clocks hits all of them alike), each bracketed by the library's own HIP events (das3r_profile_*),
every kernel of a call summed:
  (a) the median forward at threshold 0.5: render_median_forward_kernel — the walk a wave leaves once its pixels are behind their hits;
  (b) das3r_raster_distortion_forward with the totals plane: render_distortion_forward_kernel — the same walk to the end of every list;
  (c) the median adjoint: render_median_adjoint_kernel + aux_gather_kernel;
  (d) das3r_raster_aux_adjoint at C = 1: render_aux_adjoint_kernel + aux_gather_kernel — the same rows and the same gather.
Medians and min / max over the rounds go to stdout and, with --out, into a JSON file.  A record, not a gate (docs/ledger.md (ct))."""
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
    from das3r_amd.rasterizer import RasterState, _distortion_forward, _forward_full, _median_forward, feature_adjoint, median_hit_adjoint
    rs, t, _ = shape_inputs(name, dev)
    e = torch.empty(0, device=dev)
    P, H, W = t["means3D"].shape[0], int(rs.image_height), int(rs.image_width)
    G = (torch.randn(1, H, W, generator=torch.Generator().manual_seed(2)) / (H * W)).to(dev)
    _lib.forget_shapes()

    def forward():
        return _forward_full(rs, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e)

    for _ in range(3):   # the library settles on the shape's binning path and kernels
        forward()
    res = forward()
    state = RasterState.of(res, rs)
    _, hit_g, hit_p = _median_forward(state, 0.5, True, True)
    dz, dfeat = torch.empty(P, device=dev), torch.empty(P, 1, device=dev)

    calls = {
        "median_forward": lambda: _median_forward(state, 0.5, True, True),
        "distortion_forward": lambda: _distortion_forward(state, True),
        "median_adjoint": lambda: median_hit_adjoint(state, G[0], hit_p, out=dz),
        "aux_adjoint_c1": lambda: feature_adjoint(state, G, out=dfeat),
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

    rows = {k: [] for k in list(calls) + ["median_adjoint_kernel", "aux_adjoint_kernel_c1"]}
    for _ in range(repeats):
        for k, fn in calls.items():
            r = timed(fn)
            rows[k].append(sum(r.values()))
            if k == "median_adjoint":
                rows["median_adjoint_kernel"].append(r["render_median_adjoint_kernel"])
            elif k == "aux_adjoint_c1":
                rows["aux_adjoint_kernel_c1"].append(sum(ms for kk, ms in r.items() if "render_aux_adjoint_kernel" in kk))
    med = {k: round(statistics.median(v), 5) for k, v in rows.items()}
    spread = {k: [round(min(v), 5), round(max(v), 5)] for k, v in rows.items()}
    ratios = {"median_forward_over_distortion_forward": round(med["median_forward"] / med["distortion_forward"], 3),
              "median_adjoint_over_aux_adjoint_c1": round(med["median_adjoint"] / med["aux_adjoint_c1"], 3)}
    covered = hit_g >= 0
    L = _lib.layout(state.P, int(state.capacity) if int(state.capacity) > 0 else state.num_rendered, W, H)
    n_contrib = state.img[L["n_contrib"]:L["n_contrib"] + 4 * H * W].view(torch.int32)
    return dict(shape=name, P=P, W=W, H=H, num_rendered=int(res[0]), mean_list=round(int(res[0]) / (((W + 15) // 16) * ((H + 15) // 16)), 1),
                covered_pixels=int(covered.sum()), mean_hit_position=round(float(hit_p[covered].float().mean()), 1) if bool(covered.any()) else None,
                mean_n_contrib=round(float(n_contrib.float().mean()), 1), warmup=warmup, repeats=repeats, median_ms=med, min_max_ms=spread, ratios=ratios)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,sintel")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev),
           "what": "tools/median_bench.py: HIP-event times, every kernel of a call summed, medians over alternating repeats after a warm-up", "shapes": []}
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
