#!/usr/bin/env python3
"""Cost of the normal-consistency regulariser (csrc/normals.hip and the calls it is built from) in one process.

    python tools/normal_bench.py [--shape sintel] [--gaussians 2340000] [--warmup 3] [--repeats 20] [--out profiles/normal_consistency.json]
Three records, each bracketed by the library's own HIP events (das3r_profile_*), medians over `repeats` rounds after `warmup`:
  (a) the two per-Gaussian kernels at P = 2.34 M random rows (the DAS3R training shape's count), with their achieved bytes/s — 53 B per
      Gaussian forward (rotations, scales, means in; normals and the choice byte out), 45 B backward (rotations, choice, dL/dnormals in;
      dL/drotations out);
  (b) the two image kernels at 512x208 and 1920x1080 on a smooth depth image with holes, with their achieved bytes/s (forward: depth, three
      normal planes, alpha, mask in; the loss out = 28 B per pixel; backward: depth, normal, mask, dL/dloss in; five planes out = 44 B);
  (c) the whole term over the lists of one forward of `shape` (tools/aux_bench.py's: `sintel`, 512x208 with one Gaussian per pixel of 22
      frames) — das3r_render's sequence in the default "median" mode: gaussian_normals, the three-channel blend with the coverage, the median
      depth, the loss image; then its backward — beside the ray-distortion term (distortion_of forward and backward) over the SAME lists, the
      measurements alternating so that a drift of the clocks hits both alike.  Every library kernel of a call is summed; torch's own
      elementwise kernels (the mean, autograd's additions) are not in the figure.
A record, not a gate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402


def _timed(fn):
    from das3r_amd import _lib
    _lib.profile_report()
    _lib.profile_enable(True)
    out = fn()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    return out, {k: ms for k, (_, ms) in _lib.profile_report().items()}


def _summary(rows, bytes_of=None):
    med = {k: round(statistics.median(v), 5) for k, v in rows.items()}
    out = dict(median_ms=med, min_max_ms={k: [round(min(v), 5), round(max(v), 5)] for k, v in rows.items()})
    if bytes_of:
        out["GB_per_s"] = {k: round(bytes_of[k] / (med[k] * 1e-3) / 1e9, 1) for k in bytes_of if med[k] > 0}
    return out


def per_gaussian(P, dev, warmup, repeats):
    from das3r_amd import GaussianRasterizationSettings
    from das3r_amd.rasterizer import _gaussian_normals_backward, _gaussian_normals_forward
    g = torch.Generator().manual_seed(1)
    q, s = torch.randn(P, 4, generator=g).to(dev), (torch.rand(P, 3, generator=g) + 0.05).to(dev)
    mu = (torch.randn(P, 3, generator=g) + torch.tensor([0.0, 0.0, 5.0])).to(dev)
    G = torch.randn(P, 3, generator=g).to(dev)
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3, device=dev), 1.0, torch.eye(4, device=dev), torch.eye(4, device=dev), 0,
                                       torch.zeros(3, device=dev), False, False)
    _, choice = _gaussian_normals_forward(rs, q, s, mu)
    calls = {"gaussian_normals_forward": lambda: _gaussian_normals_forward(rs, q, s, mu),
             "gaussian_normals_backward": lambda: _gaussian_normals_backward(rs, q, choice, G)}
    rows = {k: [] for k in calls}
    for r in range(warmup + repeats):
        for k, fn in calls.items():
            ms = sum(_timed(fn)[1].values())
            if r >= warmup:
                rows[k].append(ms)
    return dict(P=P, bytes_per_gaussian={"gaussian_normals_forward": 53, "gaussian_normals_backward": 45},
                **_summary(rows, {"gaussian_normals_forward": 53 * P, "gaussian_normals_backward": 45 * P}))


def image(H, W, dev, warmup, repeats):
    from das3r_amd import GaussianRasterizationSettings
    from das3r_amd.rasterizer import _image_call
    g = torch.Generator().manual_seed(2)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 3.0 + torch.sin(0.01 * xs) * torch.cos(0.013 * ys) + 0.01 * torch.randn(H, W, generator=g)
    z[torch.rand(H, W, generator=g) < 0.01] = 0.0
    z, normal, alpha = z.to(dev), torch.randn(3, H, W, generator=g).to(dev), torch.rand(H, W, generator=g).to(dev)
    mask, G = torch.rand(H, W, generator=g).to(dev), torch.randn(H, W, generator=g).to(dev)
    loss, gd, gn, ga = torch.empty_like(z), torch.empty_like(z), torch.empty_like(normal), torch.empty_like(z)
    rs = GaussianRasterizationSettings(H, W, 0.5 * W / 600.0, 0.5 * H / 600.0, torch.zeros(3, device=dev), 1.0, torch.eye(4, device=dev),
                                       torch.eye(4, device=dev), 0, torch.zeros(3, device=dev), False, False)
    calls = {"normal_consistency_forward": lambda: _image_call("das3r_normal_consistency_forward", rs, z, normal, alpha, mask, loss, None),
             "normal_consistency_backward": lambda: _image_call("das3r_normal_consistency_backward", rs, z, normal, mask, G, gd, gn, ga)}
    rows = {k: [] for k in calls}
    for r in range(warmup + repeats):
        for k, fn in calls.items():
            ms = sum(_timed(fn)[1].values())
            if r >= warmup:
                rows[k].append(ms)
    return dict(H=H, W=W, bytes_per_pixel={"normal_consistency_forward": 28, "normal_consistency_backward": 44},
                **_summary(rows, {"normal_consistency_forward": 28 * H * W, "normal_consistency_backward": 44 * H * W}))


def whole_term(name, dev, warmup, repeats):
    from aux_bench import shape_inputs
    from das3r_amd import AuxGeometry, _lib, distortion_of, gaussian_normals, median_depth_of, normal_consistency
    from das3r_amd.rasterizer import RasterState, _aux_with_geometry, _forward_full
    rs, t, _ = shape_inputs(name, dev)
    e = torch.empty(0, device=dev)
    P, H, W = t["means3D"].shape[0], int(rs.image_height), int(rs.image_width)
    _lib.forget_shapes()
    for _ in range(3):   # the library settles on the shape's binning path and kernels
        _forward_full(rs, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e)
    res = _forward_full(rs, t["means3D"], t["sh"], e, t["opacities"], t["scales"], t["rotations"], e)
    state = RasterState.of(res, rs)

    def leaves():
        kw = {k: t[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
        kw["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
        return kw, AuxGeometry(rs, shs=t["sh"], **kw)

    def normal_forward():
        kw, geo = leaves()
        n = gaussian_normals(rs, kw["rotations"], kw["scales"], kw["means3D"])
        img, alpha = _aux_with_geometry(state, n, geo, True)
        return normal_consistency(median_depth_of(state, geometry=geo), img, alpha, rs).mean()

    def distortion_forward():
        return distortion_of(state, geometry=leaves()[1]).mean()

    rows = {k: [] for k in ("normal_forward", "normal_backward", "distortion_forward", "distortion_backward")}
    kernels = {}
    for r in range(warmup + repeats):
        for k, fn in (("normal", normal_forward), ("distortion", distortion_forward)):
            loss, fwd = _timed(fn)
            _, bwd = _timed(loss.backward)
            if r >= warmup:
                rows[k + "_forward"].append(sum(fwd.values()))
                rows[k + "_backward"].append(sum(bwd.values()))
                kernels[k + "_forward"], kernels[k + "_backward"] = {a: round(b, 5) for a, b in fwd.items()}, {a: round(b, 5) for a, b in bwd.items()}
    out = _summary(rows)
    med = out["median_ms"]
    out["ratios"] = {"normal_over_distortion_forward": round(med["normal_forward"] / med["distortion_forward"], 3),
                     "normal_over_distortion_backward": round(med["normal_backward"] / med["distortion_backward"], 3)}
    return dict(shape=name, P=P, W=W, H=H, num_rendered=int(res[0]), last_round_kernels_ms=kernels, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="sintel")
    ap.add_argument("--gaussians", type=int, default=2_340_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev),
           "what": "tools/normal_bench.py: HIP-event times, every library kernel of a call summed, medians over alternating repeats after a warm-up"}
    out["per_gaussian"] = per_gaussian(args.gaussians, dev, args.warmup, args.repeats)
    print(json.dumps(out["per_gaussian"]), flush=True)
    out["image"] = [image(H, W, dev, args.warmup, args.repeats) for H, W in ((208, 512), (1080, 1920))]
    print(json.dumps(out["image"]), flush=True)
    out["whole_term"] = whole_term(args.shape, dev, args.warmup, args.repeats)
    print(json.dumps(out["whole_term"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
