"""The DAS3R-shaped fused train step (noise and smooth depth maps): ms per step under bench.py's timing protocol and the per-kernel
table of the library's own profiler (HIP events around every launch).   python tools/train_step_kernels.py [--depth-l1 INIT FINAL] [--exposure-lr INIT FINAL]
--exposure-lr: the same for the step with per-frame exposure compensation (OptimParams.exposure_lr_init / _final) beside the step without,
with the library's launches per step and the launches the feature adds (exposure_grad_finish_kernel).
--depth-l1: the same for the depth-supervised step (the inverse-depth L1 term, OptimParams.depth_l1_weight_init / _final), with the
library's launches per step and the launches the term adds."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
ap = argparse.ArgumentParser()
ap.add_argument("--depth-l1", nargs=2, type=float, default=None, metavar=("INIT", "FINAL"))
ap.add_argument("--exposure-lr", nargs=2, type=float, default=None, metavar=("INIT", "FINAL"))
ap.add_argument("--json", default=None, help="also write the rows to this file")
cli = ap.parse_args()
dev = torch.device('cuda:0'); torch.cuda.set_device(0)
rk = bench.Ranks(bench.parse_args(['--gpus', '1']))
from das3r_amd import _lib


def depth_step_timer(depth, w0, w1, exposure=(0.0, 0.0), depth_targets=True):
    """bench.train_step_timer's step with cameras that carry the sequence's depth maps and the term's weights in OptimParams; exposure: the
    learning rates of per-frame exposure compensation."""
    from types import SimpleNamespace
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence, train_step
    seq = synthetic_sequence(frames=20, W=512, H=208, focal=600.0, n_splats=20000, seed=0, device=str(dev), depth=depth)
    model, cams = build_from_sequence(seq, depth_targets=depth_targets)
    opt = OptimParams(iterations=bench.ITERS_PER_SCENE, depth_l1_weight_init=w0, depth_l1_weight_final=w1, exposure_lr_init=exposure[0],
                      exposure_lr_final=exposure[1])
    model.training_setup(opt, fused=True)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    it = [0]

    def step():
        it[0] += 1
        train_step(model, cams[it[0] % len(cams)], opt, it[0], pipe, bg, fused=True)
    return step


rows = []
for depth in ('noise', 'smooth'):
    variants = [("photometric", lambda: bench.train_step_timer(dev, fused=True, depth=depth)[0])]
    if cli.depth_l1 is not None:
        variants += [("depth weights 0", lambda: depth_step_timer(depth, 0.0, 0.0)), ("depth", lambda: depth_step_timer(depth, *cli.depth_l1))]
    if cli.exposure_lr is not None:
        variants += [("exposure off", lambda: depth_step_timer(depth, 0.0, 0.0, depth_targets=False)),
                     ("exposure", lambda: depth_step_timer(depth, 0.0, 0.0, exposure=tuple(cli.exposure_lr), depth_targets=False))]
    for what, make in variants:
        step = make()
        for _ in range(30): step()
        t = rk.timed(step, 100, 10) / 100 * 1e3
        _lib.profile_enable(True)
        for _ in range(20): step()
        torch.cuda.synchronize(); rep = _lib.profile_report(); _lib.profile_enable(False)
        row = dict(depth_maps=depth, step=what, train_step_ms=round(t, 4), library_launches_per_step=sum(v[0] for v in rep.values()) / 20,
                   depth_term_launches_per_step=sum(v[0] for k, v in rep.items() if k.startswith(("depth_l1", "depth_pass_inputs", "depth_fold"))) / 20,
                   exposure_launches_per_step=sum(v[0] for k, v in rep.items() if k.startswith("exposure_grad_finish")) / 20,
                   kernel_ms={k: round(v[1] / 20, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])[:16]})
        rows.append(row)
        print(depth, what, 'train step ms', row["train_step_ms"], 'launches', row["library_launches_per_step"], row["kernel_ms"], flush=True)
        del step
if cli.json:
    os.makedirs(os.path.dirname(os.path.abspath(cli.json)), exist_ok=True)
    with open(cli.json, "w") as f:
        json.dump(rows, f, indent=1)
