#!/usr/bin/env python3
"""Cost of the aux-channel kernels (csrc/render_aux.hip) beside the parent's kernels on the same lists, in one process.

    python tools/aux_bench.py [--shapes sintel,c4] [--repeats 7] [--out profiles/aux_channels.json]
Shapes: `sintel` — the DAS3R training shape, 22 frames of 512x208 with one Gaussian per pixel (2.34 M) on smooth depth maps, one view's
forward as the training step makes it; `c4` — 1 M random splats at 1920x1080, SH degree 3 (bench.py's flagship workload).
Per shape one forward is kept (its saved state is what the aux calls read); then, after a warm-up of everything, `repeats` rounds in which the
measurements ALTERNATE (a drift of the clocks hits all of them alike), each bracketed by the library's own HIP events (das3r_profile_*):
  * the colour compositing forward kernel and the compositing backward kernel of that forward (the parent's kernels, the yardsticks);
  * a second complete forward with colors_precomp — every kernel of it, summed: what a feature image cost before (render_confidence's way);
  * render_aux_forward_kernel at C = 1, 3, 8;  render_aux_adjoint_kernel + aux_gather_kernel at C = 1, 3.
The medians over the rounds and the ratios go to stdout and, with --out, into a JSON file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def shape_inputs(name, dev):
    """-> (settings, dict of the eight tensor arguments of _forward_full, dL_dpix)"""
    from das3r_amd import GaussianRasterizationSettings
    e = torch.empty(0, device=dev)
    if name == "c4":
        from das3r_amd.synth import make_workload
        sc = make_workload("c4").to(dev)
        rs = GaussianRasterizationSettings(**sc.settings_kwargs())
        return rs, dict(means3D=sc.means3D, sh=sc.shs, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations), sc.dL_dpix
    if name == "sintel":
        from types import SimpleNamespace
        from das3r_amd.render import rasterizer_inputs
        from das3r_amd.train import build_from_sequence, synthetic_sequence
        seq = synthetic_sequence(frames=22, W=512, H=208, focal=600.0, n_splats=20000, seed=0, device=str(dev), depth="smooth")
        model, cams = build_from_sequence(seq)
        pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
        with torch.no_grad():
            rs, kw = rasterizer_inputs(cams[3], model, pipe, torch.zeros(3, device=dev), camera_pose=model.get_RT(3))
        t = {k: kw[k].detach().contiguous() for k in ("means3D", "opacities", "scales", "rotations")}
        t["sh"] = kw["shs"].detach().contiguous()
        g = torch.Generator().manual_seed(1)
        return rs, t, (torch.randn(3, 208, 512, generator=g) / (208 * 512)).to(dev)
    raise KeyError(name)


def measure(name, dev, repeats):
    from das3r_amd import _lib
    from das3r_amd.rasterizer import RasterState, _backward_impl, _forward_full, composite_features, feature_adjoint
    rs, t, dL = shape_inputs(name, dev)
    e = torch.empty(0, device=dev)
    P, H, W = t["means3D"].shape[0], int(rs.image_height), int(rs.image_width)
    g = torch.Generator().manual_seed(2)
    F = torch.rand(P, 8, generator=g).to(dev)
    feats = {c: F[:, :c].contiguous() for c in (1, 3, 8)}
    grads = {c: (torch.randn(c, H, W, generator=g) / (H * W)).to(dev) for c in (1, 3)}
    _lib.forget_shapes()

    def forward(colors=None):
        return _forward_full(rs, t["means3D"], e if colors is not None else t["sh"], colors if colors is not None else e, t["opacities"],
                             t["scales"], t["rotations"], e)

    def backward(res):
        _backward_impl(rs, res[0], dL, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e, res[3], res[4], res[5], res[6])

    for _ in range(3):   # the library settles on the shape's binning path and kernels
        res = forward()
        backward(res)
        forward(feats[3])
    res = forward()
    state = RasterState.of(res, rs)
    for c in feats:
        composite_features(state, feats[c])
    for c in grads:
        feature_adjoint(state, grads[c])
    torch.cuda.synchronize()

    def timed(fn):
        """kernel name -> ms of one call of fn (the library's events around each of its launches)"""
        _lib.profile_report()
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        return {k: ms for k, (_, ms) in _lib.profile_report().items()}

    rows = {k: [] for k in ("colour_forward_kernel", "colour_backward_kernel", "second_forward_all_kernels", "aux_forward_c1", "aux_forward_c3",
                            "aux_forward_c8", "aux_adjoint_c1", "aux_adjoint_c3", "aux_gather_c1", "aux_gather_c3")}
    names = {}
    for _ in range(repeats):
        r = timed(lambda: backward(forward()))
        fk = [k for k in r if k.startswith("render_forward")]
        bk = [k for k in r if k.startswith("render_backward")]
        names["colour_forward_kernel"], names["colour_backward_kernel"] = "+".join(fk), "+".join(bk)
        rows["colour_forward_kernel"].append(sum(r[k] for k in fk))
        rows["colour_backward_kernel"].append(sum(r[k] for k in bk))
        rows["second_forward_all_kernels"].append(sum(timed(lambda: forward(feats[3])).values()))
        for c in (1, 3, 8):
            rows[f"aux_forward_c{c}"].append(timed(lambda: composite_features(state, feats[c]))["render_aux_forward_kernel"])
        for c in (1, 3):
            r = timed(lambda: feature_adjoint(state, grads[c]))
            rows[f"aux_adjoint_c{c}"].append(r["render_aux_adjoint_kernel"])
            rows[f"aux_gather_c{c}"].append(r["aux_gather_kernel"])
    med = {k: round(statistics.median(v), 5) for k, v in rows.items()}
    spread = {k: [round(min(v), 5), round(max(v), 5)] for k, v in rows.items()}
    fwd, bwd, second = med["colour_forward_kernel"], med["colour_backward_kernel"], med["second_forward_all_kernels"]
    ratios = {f"aux_forward_c{c}_over_colour_forward": round(med[f"aux_forward_c{c}"] / fwd, 3) for c in (1, 3, 8)}
    ratios.update({f"second_forward_over_aux_forward_c{c}": round(second / med[f"aux_forward_c{c}"], 2) for c in (1, 3, 8)})
    ratios.update({f"aux_adjoint_pair_c{c}_over_colour_backward": round((med[f"aux_adjoint_c{c}"] + med[f"aux_gather_c{c}"]) / bwd, 3) for c in (1, 3)})
    return dict(shape=name, P=P, W=W, H=H, num_rendered=int(res[0]), mean_list=round(int(res[0]) / (((W + 15) // 16) * ((H + 15) // 16)), 1), repeats=repeats,
                parent_kernels=names, median_ms=med, min_max_ms=spread, ratios=ratios)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sintel,c4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "what": "tools/aux_bench.py: HIP-event times of single launches, medians over alternating repeats", "shapes": []}
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
