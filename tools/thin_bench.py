#!/usr/bin/env python3
"""What voxel thinning (das3r_amd.thin) costs and buys, on one GPU.

    python tools/thin_bench.py voxels [--out profiles/thin_voxels.json]
    python tools/thin_bench.py train  [--out profiles/thin_train_step.jsonl] [--seeds 0,1,2] [--iterations 600]

voxels: das3r_thin_voxels against thin.voxel_keep_torch on the same device in the same process, at the Sintel training shape (22 frames
512x208: 2.34 M points) and the DAVIS one (50 frames 512x288: 7.37 M points) — the shapes of profiles/prune_compaction.json.  The points are a
smooth relief unprojected from F slightly shifted cameras with 0.5 % of depth noise (a static surface seen F times), the score a random
confidence, the edge one pixel footprint.  Median of 20 runs after 3 warm-ups, HIP events; the kept fraction; the two results compared.

train: train.consistent_sequence at the Sintel shape, self-consistent and with the predictor's errors put back (depth_noise 0.02, pose_noise
0.01), thin_relative in {off, 0.5, 1, 2} with thin_opacity "coverage" and R = 1 also with "reference".  Per row and seed: P, the fused train
step's ms (first seed only; measured apart from the job, whose rate contains the held-out passes: 100 steps after 20 warm-ups on the model
as built), peak HBM of the job, and the held-out static-region PSNR after the job of tests/test_gpu_prune.py's protocol (held-out split,
fused, job seed = sequence seed).  One JSON line per (variant, setting, seed), appended as it is measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = {"sintel": (22, 208, 512), "davis": (50, 288, 512)}
SINTEL = dict(frames=22, W=512, H=208, focal=600.0, n_splats=20000)
VARIANTS = {"consistent": dict(), "noisy": dict(depth_noise=0.02, pose_noise=0.01)}
SETTINGS = [("off", None, "coverage"), ("0.5", 0.5, "coverage"), ("1", 1.0, "coverage"), ("2", 2.0, "coverage"), ("1-reference", 1.0, "reference")]


def surface_points(F, H, W, seed):
    """[F * H * W, 3] world points of one relief seen from F shifted cameras, and the pixel footprint."""
    from das3r_amd.model import depth_to_points
    from das3r_amd.thin import pixel_footprint
    g = torch.Generator(device="cuda").manual_seed(seed)
    focal = 600.0
    vv, uu = torch.meshgrid(torch.linspace(-1, 1, H, device="cuda"), torch.linspace(-1, 1, W, device="cuda"), indexing="ij")
    K = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]], device="cuda").repeat(F, 1, 1)
    c2w = torch.eye(4, device="cuda").repeat(F, 1, 1)
    c2w[:, 0, 3] = 0.01 * torch.arange(F, device="cuda")
    shift = c2w[:, 0, 3][:, None, None] * focal / 4.0 / (W / 2)   # the relief follows the world, not the camera
    depth = 4.0 + 0.5 * torch.sin(3.0 * (uu[None] + shift)) * torch.cos(2.0 * vv[None])
    depth = depth * (1.0 + 0.005 * torch.randn(F, H, W, device="cuda", generator=g))
    pts = depth_to_points(K, c2w, depth).reshape(-1, 3).contiguous()
    return pts, pixel_footprint(depth, K, None)


def timed(fn, warmup=3, runs=20):
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


def voxels(args):
    from das3r_amd import _lib
    from das3r_amd.thin import inv_edge_of, voxel_keep_kernels, voxel_keep_torch
    rows = []
    for name, (F, H, W) in SHAPES.items():
        pts, fp = surface_points(F, H, W, seed=1)
        P = pts.shape[0]
        score = torch.rand(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        inv = inv_edge_of(fp)
        keep, count, info = voxel_keep_kernels(pts, score, inv)
        tk, tc = voxel_keep_torch(pts, score, inv)
        same = bool(torch.equal(keep.view(torch.bool), tk) and torch.equal(count, tc))
        kept, err = info.tolist()
        k_ms = timed(lambda: voxel_keep_kernels(pts, score, inv))
        t_ms = timed(lambda: voxel_keep_torch(pts, score, inv))
        rows.append(dict(shape=name, frames=F, image=[W, H], points=P, edge=fp, kept=kept, kept_fraction=round(kept / P, 4), table_error=err,
                         identical_to_torch=same, workspace_bytes=int(_lib.load().das3r_thin_workspace_bytes(P)),
                         kernels_ms_median=round(statistics.median(k_ms), 3), torch_ms_median=round(statistics.median(t_ms), 3),
                         kernels_ms_min=round(min(k_ms), 3), kernels_ms_max=round(max(k_ms), 3), torch_ms_min=round(min(t_ms), 3), torch_ms_max=round(max(t_ms), 3)))
        print(json.dumps(rows[-1]), flush=True)
        del pts, score, keep, count, tk, tc
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(what="das3r_thin_voxels vs thin.voxel_keep_torch, same device and process (tools/thin_bench.py voxels): median of 20 runs after "
                                "3 warm-ups, HIP events, workspace allocation included; edge = one pixel footprint",
                           rows=rows), f, indent=1)
            f.write("\n")


def step_ms(seq, thin_kw):
    """ms of the fused train step on the model as built: 100 steps after 20 warm-ups, HIP events around the hundred."""
    from types import SimpleNamespace
    from das3r_amd import _lib
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, train_step
    _lib.forget_shapes()
    model, cams, _ = build_from_sequence(seq, heldout=True, **thin_kw)
    opt = OptimParams(iterations=600)
    model.training_setup(opt, fused=True)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device="cuda")
    for it in range(1, 21):
        train_step(model, cams[it % len(cams)], opt, it, pipe, bg, fused=True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for it in range(21, 121):
        train_step(model, cams[it % len(cams)], opt, it, pipe, bg, fused=True)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 100.0, int(model._xyz.shape[0])


def train(args):
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.train import consistent_sequence
    dev = torch.device("cuda:0")
    seeds = [int(s) for s in args.seeds.split(",")]
    out = open(args.out, "a") if args.out else None
    for variant, noise in VARIANTS.items():
        for seed in seeds:
            seq = consistent_sequence(seed=seed, moving=True, **SINTEL, **noise)
            for label, rel, mode in SETTINGS:
                thin_kw = {} if rel is None else dict(thin_relative=rel, thin_opacity=mode)
                ms, P0 = step_ms(seq, thin_kw) if seed == seeds[0] else (None, None)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                keep = {}
                rec = run_sequence_job(seed, args.iterations, dev, fused=True, seq=seq, keep=keep,
                                       **({} if rel is None else dict(thin_init_relative=rel, thin_opacity=mode)))
                peak = torch.cuda.max_memory_allocated()
                row = dict(variant=variant, thin_relative=label, thin_opacity=mode if rel is not None else None, seed=seed, P=rec["n_splats"], P_step=P0,
                           step_ms=None if ms is None else round(ms, 3), job_iters_per_s=round(rec["iters_per_s"], 1), peak_hbm_bytes=int(peak),
                           iterations=args.iterations, heldout_static_psnr=rec["psnr"], ok=rec["ok"])
                print(json.dumps(row), flush=True)
                if out:
                    out.write(json.dumps(row) + "\n")
                    out.flush()
                del keep
            del seq
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("voxels", "train"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--iterations", type=int, default=600)
    args = ap.parse_args()
    (voxels if args.what == "voxels" else train)(args)


if __name__ == "__main__":
    main()
