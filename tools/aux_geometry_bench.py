#!/usr/bin/env python3
"""Cost of the aux channels' geometry backward (csrc/render_aux_bwd.hip, das3r_raster_aux_backward) beside what the same gradients cost
without it, in one process.

    python tools/aux_geometry_bench.py [--shapes c4,sintel] [--repeats 9] [--out profiles/aux_geometry.json]
Shapes: tools/aux_bench.py's — `c4`, 1 M random splats at 1920x1080, SH degree 3 (bench.py's flagship workload); `sintel`, the DAS3R
training shape, 512x208 with one Gaussian per pixel of 22 frames (few tiles, ~11 k-entry lists).
Per shape one forward is kept (its saved state is what the new entry reads); then, after a warm-up of everything, `repeats` rounds in which
the measurements ALTERNATE (a drift of the clocks hits all of them alike), each bracketed by the library's own HIP events (das3r_profile_*),
every kernel of a call summed:
  (a) das3r_raster_aux_backward at C = 1 and C = 3, with dL_dfeatures: render_aux_backward_kernel + aux_gather_kernel + the per-Gaussian
      backward (the compositing kernel's own time is listed as well);
  (b) the parent's way to the same gradients (render_confidence's): a second complete forward with colors_precomp = the features, plus
      das3r_raster_backward on it.
Medians and min / max over the rounds go to stdout and, with --out, into a JSON file; "tie" = one median inside the other's min..max."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402


def measure(name, dev, repeats):
    from aux_bench import shape_inputs
    from das3r_amd import _lib
    from das3r_amd.rasterizer import RasterState, _aux_backward_impl, _backward_impl, _forward_full
    rs, t, _ = shape_inputs(name, dev)
    e = torch.empty(0, device=dev)
    P, H, W = t["means3D"].shape[0], int(rs.image_height), int(rs.image_width)
    g = torch.Generator().manual_seed(2)
    F = torch.rand(P, 3, generator=g).to(dev)
    feats = {c: F[:, :c].contiguous() for c in (1, 3)}
    G = (torch.randn(3, H, W, generator=g) / (H * W)).to(dev)
    grads = {c: G[:c].contiguous() for c in (1, 3)}
    rs0 = rs._replace(bg=torch.zeros(3, device=dev))
    _lib.forget_shapes()

    def forward():
        return _forward_full(rs, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e)

    def parent_way():
        res = _forward_full(rs0, t["means3D"], e, feats[3], t["opacities"], t["scales"], t["rotations"], e)
        _backward_impl(rs0, res[0], G, t["means3D"], e, feats[3], t["opacities"], t["scales"], t["rotations"], e, res[3], res[4], res[5], res[6])

    def new_entry(state, c):
        _aux_backward_impl(state, rs, feats[c], grads[c], None, True, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e)

    for _ in range(3):   # the library settles on the shape's binning path and kernels
        forward()
        parent_way()
    res = forward()
    state = RasterState.of(res, rs)
    for c in (1, 3):
        new_entry(state, c)
    torch.cuda.synchronize()

    def timed(fn):
        _lib.profile_report()
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        return {k: ms for k, (_, ms) in _lib.profile_report().items()}

    rows = {k: [] for k in ("aux_backward_c1", "aux_backward_c3", "aux_backward_kernel_c1", "aux_backward_kernel_c3", "parent_second_forward_plus_backward")}
    for _ in range(repeats):
        for c in (1, 3):
            r = timed(lambda: new_entry(state, c))
            rows[f"aux_backward_c{c}"].append(sum(r.values()))
            rows[f"aux_backward_kernel_c{c}"].append(r["render_aux_backward_kernel"])
        rows["parent_second_forward_plus_backward"].append(sum(timed(parent_way).values()))
    med = {k: round(statistics.median(v), 5) for k, v in rows.items()}
    spread = {k: [round(min(v), 5), round(max(v), 5)] for k, v in rows.items()}
    b = "parent_second_forward_plus_backward"
    verdict = {}
    for c in (1, 3):
        a = f"aux_backward_c{c}"
        tie = spread[b][0] <= med[a] <= spread[b][1] or spread[a][0] <= med[b] <= spread[a][1]
        verdict[f"c{c}"] = "tie" if tie else ("new entry faster" if med[a] < med[b] else "new entry slower")
    ratios = {f"parent_over_aux_backward_c{c}": round(med[b] / med[f"aux_backward_c{c}"], 3) for c in (1, 3)}
    return dict(shape=name, P=P, W=W, H=H, num_rendered=int(res[0]), mean_list=round(int(res[0]) / (((W + 15) // 16) * ((H + 15) // 16)), 1), repeats=repeats,
                median_ms=med, min_max_ms=spread, ratios=ratios, verdict=verdict)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,sintel")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev),
           "what": "tools/aux_geometry_bench.py: HIP-event times, every kernel of a call summed, medians over alternating repeats after a warm-up", "shapes": []}
    for name in args.shapes.split(","):
        row = measure(name, dev, args.repeats)
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
