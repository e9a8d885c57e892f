#!/usr/bin/env python3
"""What TSDF fusion and mesh extraction (das3r_amd.tsdf) cost, on one GPU.

    python tools/tsdf_bench.py [--out profiles/tsdf_fusion.json] [--small]

das3r_tsdf_integrate against tsdf.integrate_torch on the same device in the same process, at a Sintel-shaped job (256^3 voxels, 22 views of
512x208) and a DAVIS-shaped one (512x512x256 voxels, 50 views of 512x288).  The depth images are a smooth relief seen from slightly shifted
cameras (a static surface seen V times), with a colour image and no weight image; the grid has colour.  The baseline is the torch form, never
the kernel.  Then both extraction passes (das3r_tsdf_extract_count, das3r_tsdf_extract_emit) on the fused Sintel-shaped grid.  Median of the
runs after warm-ups, HIP events around each call; the kernel's result against the torch form's on the grid it timed (both on the device:
the tests hold the kernel to the torch form run on the CPU, bit for bit; on the device the two can differ in the last bit of a quotient,
and a voxel whose projection lies within an ulp of a pixel boundary then reads the neighbouring pixel: the fraction of such voxels is reported).

Bytes per integrate call: the kernel reads and writes the grid once per launch of up to DAS3R_TSDF_MAX_VIEWS views — 5 planes x 4 bytes read,
and written where a view was taken — plus the images it gathers from (counted once: neighbouring voxels share their cache lines).  The HBM
share is those bytes over the call's time over the 8 TB/s peak; the kernel does some 60 flops and four IEEE divisions per (voxel, view), so
at many views it is bound by that arithmetic and the gathers, not by the grid's bytes.  --small: a toy size, to rehearse the script."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = {"sintel": dict(dims=(256, 256, 256), V=22, H=208, W=512), "davis": dict(dims=(512, 512, 256), V=50, H=288, W=512)}
SMALL = {"sintel": dict(dims=(48, 40, 32), V=5, H=26, W=64), "davis": dict(dims=(64, 48, 32), V=18, H=36, W=64)}


def scene(dims, V, H, W, seed=1, device="cuda"):
    """A relief at depth about 4 in front of V cameras shifted along x, and the grid around it -> dict of integrate's arguments."""
    focal = 600.0 * W / 512.0
    tanx, tany = 0.5 * W / focal, 0.5 * H / focal
    g = torch.Generator(device=device).manual_seed(seed)
    vv, uu = torch.meshgrid(torch.linspace(-1, 1, H, device=device), torch.linspace(-1, 1, W, device=device), indexing="ij")
    shift = 0.01 * torch.arange(V, device=device, dtype=torch.float32)
    depth = 4.0 + 0.5 * torch.sin(3.0 * (uu[None] + shift[:, None, None] * focal / 4.0 / (W / 2))) * torch.cos(2.0 * vv[None])
    depth = (depth * (1.0 + 0.002 * torch.randn(V, H, W, device=device, generator=g))).contiguous()
    vm = torch.eye(4, device=device).repeat(V, 1, 1)
    vm[:, 3, 0] = -shift   # row-vector layout: the translation is the last row; camera v stands at x = shift[v]
    colour = torch.rand(V, 3, H, W, device=device, generator=g)
    nx, ny, nz = dims
    # the box the first camera sees between depth 3.3 and 4.7, cut into the grid
    ext = (2 * 4.7 * tanx, 2 * 4.7 * tany, 1.4)
    voxel = max(ext[0] / nx, ext[1] / ny, ext[2] / nz)
    origin = (-0.5 * nx * voxel, -0.5 * ny * voxel, 4.0 - 0.5 * nz * voxel)
    return dict(dims=dims, origin=origin, voxel=voxel, depth=depth, viewmatrix=vm.reshape(V, 16).contiguous(), tanfovx=tanx, tanfovy=tany,
                colour=colour.contiguous(), trunc=4.0 * voxel)


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--torch-runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tsdf_bench.py measures on a GPU; none is visible")
    from das3r_amd import _lib
    from das3r_amd.tsdf import TSDFGrid, extract_kernels, integrate_torch
    rows, fused = [], None
    for name, shp in (SMALL if args.small else SHAPES).items():
        sc = scene(**shp)
        nx, ny, nz = shp["dims"]
        nvox, V, H, W = nx * ny * nz, shp["V"], shp["H"], shp["W"]
        grid = TSDFGrid(sc["origin"], sc["voxel"], sc["dims"], device="cuda")
        call = dict(colour=sc["colour"], trunc=sc["trunc"])

        def reset():
            grid.tsdf.fill_(1.0)
            grid.weight.zero_()
            grid.colour.zero_()

        def kernel():
            reset()
            grid.integrate(sc["depth"], sc["viewmatrix"], sc["tanfovx"], sc["tanfovy"], use_kernels=True, **call)

        reset_ms = statistics.median(timed(reset, 2, args.runs))
        k_ms = [m - reset_ms for m in timed(kernel, 2, args.runs)]
        torch.cuda.synchronize()
        observed = float((grid.weight > 0).float().mean())
        fresh = lambda: (torch.ones_like(grid.tsdf), torch.zeros_like(grid.weight), torch.zeros_like(grid.colour))
        ref = integrate_torch(*fresh(), grid.dims, grid.origin, grid.voxel, sc["depth"], sc["viewmatrix"], sc["tanfovx"], sc["tanfovy"], sc["colour"], None,
                              sc["trunc"])
        same_set = float(((ref[1] > 0) == (grid.weight > 0)).float().mean())
        both = (ref[1] > 0) & (grid.weight > 0) & (ref[1] == grid.weight)
        max_err = float((ref[0] - grid.tsdf)[both].abs().max()) if bool(both.any()) else 0.0
        differs = float(((ref[0] - grid.tsdf).abs() > 1e-5).float().mean())
        identical = bool(torch.equal(ref[0], grid.tsdf) and torch.equal(ref[1], grid.weight) and torch.equal(ref[2], grid.colour))
        del ref
        t_ms = timed(lambda: integrate_torch(*fresh(), grid.dims, grid.origin, grid.voxel, sc["depth"], sc["viewmatrix"], sc["tanfovx"], sc["tanfovy"],
                                             sc["colour"], None, sc["trunc"]), 1, args.torch_runs)
        launches = math.ceil(V / _lib.TSDF_MAX_VIEWS)
        grid_bytes = launches * nvox * 5 * 4 * (1.0 + observed)   # read all, write where a view was taken (an upper bound: per launch, not per call)
        image_bytes = V * H * W * 4 * 4
        k_med = statistics.median(k_ms)
        rows.append(dict(shape=name, dims=[nx, ny, nz], voxels=nvox, views=V, image=[W, H], launches=launches, observed_fraction=round(observed, 4),
                         kernel_ms_median=round(k_med, 3), kernel_ms_min=round(min(k_ms), 3), kernel_ms_max=round(max(k_ms), 3),
                         grid_reset_ms=round(reset_ms, 3), torch_ms_median=round(statistics.median(t_ms), 3), torch_ms_min=round(min(t_ms), 3),
                         speedup=round(statistics.median(t_ms) / k_med, 1), bytes_per_call=int(grid_bytes + image_bytes),
                         hbm_fraction=round((grid_bytes + image_bytes) / (k_med * 1e-3) / HBM_PEAK, 4),
                         voxel_views_per_s=round(nvox * V / (k_med * 1e-3), 0), identical_to_torch_form=identical,
                         same_observation_set_fraction=round(same_set, 6), max_tsdf_difference_where_weights_agree=max_err,
                         tsdf_differs_by_more_than_1e_5_fraction=differs))
        print(json.dumps(rows[-1]), flush=True)
        if name == "sintel":
            fused = (grid, sc)
        else:
            del grid
        del sc
        torch.cuda.empty_cache()
    grid, _ = fused
    lib = _lib.load()
    _lib.profile_report()
    mesh = extract_kernels(grid.tsdf, grid.weight, grid.colour, grid.dims, grid.origin, grid.voxel)
    e_ms = timed(lambda: extract_kernels(grid.tsdf, grid.weight, grid.colour, grid.dims, grid.origin, grid.voxel), 2, args.runs)
    _lib.profile_enable(True)
    for _ in range(args.runs):
        extract_kernels(grid.tsdf, grid.weight, grid.colour, grid.dims, grid.origin, grid.voxel)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    prof = {k: round(ms / n, 4) for k, (n, ms) in _lib.profile_report().items() if k.startswith("tsdf_")}
    nvox = grid.tsdf.numel()
    extraction = dict(shape="sintel", voxels=nvox, vertices=int(mesh["vertices"].shape[0]), triangles=int(mesh["faces"].shape[0]),
                      both_passes_ms_median=round(statistics.median(e_ms), 3), both_passes_ms_min=round(min(e_ms), 3),
                      kernel_ms_mean_by_launch=prof, count_pass_ms=round(sum(prof.get(k, 0.0) for k in ("tsdf_count_kernel", "tsdf_scan_kernel", "tsdf_base_kernel")), 4),
                      emit_pass_ms=prof.get("tsdf_emit_kernel"),
                      workspace_bytes=int(lib.das3r_tsdf_extract_workspace_bytes((__import__("ctypes").c_int32 * 3)(*grid.dims))))
    print(json.dumps(extraction), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(what="das3r_tsdf_integrate vs tsdf.integrate_torch, same device and process, and the two extraction passes on the fused "
                                "Sintel-shaped grid (tools/tsdf_bench.py): medians, HIP events around each call, the grid's reset subtracted from the "
                                "kernel's time; both_passes_ms includes the host read of (Nv, Nf) and the output allocations, the per-launch figures "
                                "are the library's own event timings; bytes_per_call = grid planes read once and written where observed, per launch, "
                                "+ the images once; hbm_fraction = those bytes / time / 8 TB/s",
                           integrate=rows, extraction=extraction), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
