#!/usr/bin/env python3
"""Cost of one prune event (das3r_amd.prune.prune_points) at the training shapes: the HIP path (das3r_prune_select + das3r_prune_compact)
against the torch path (boolean indexing of the same tensors: what the reference's _prune_optimizer does), in one process, the two
alternating after a warm-up of each.

    python tools/prune_bench.py [--repeats 5] [--out profiles/prune_compaction.json]
Shapes: Sintel (22 frames 512x208) and DAVIS (50 frames 512x288); drop fractions 2 % and 25 % (conf_static = 0 on that share of the
pixels, at random: the shortest runs of kept rows).  The model is the state of a fused job below iteration 3000: six parameters, FusedAdam
moments (those of f_rest compact: [P, 0, 3] at degree 0), the cached pixel index.  Per point: ms of each path (every repeat), the bytes an
event has to move — P * (4 + 4 + 8) for the decision's inputs + 2 * kept * row bytes —, GB/s, and torch.cuda.max_memory_allocated over
the event above what was allocated before it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch import nn  # noqa: E402

SHAPES = {"sintel": (22, 208, 512), "davis": (50, 288, 512)}
COPY_RATE_TBS = 6.29   # the float4-copy rate measured on this project's MI355X (VERDICT weak item 6)


def make_state(F, H, W, drop, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = F * H * W
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    t = dict(_xyz=r(P, 3), _features_dc=r(P, 1, 3), _features_rest=torch.zeros(P, 15, 3, device="cuda"), _scaling=r(P, 3) - 3, _rotation=r(P, 4),
             _opacity=torch.full((P, 1), -3.0, device="cuda"))
    conf = torch.ones(F, H, W, device="cuda")
    conf.view(-1)[torch.rand(P, device="cuda", generator=g) < drop] = 0.0
    return t, conf


def make_model(t, conf):
    from das3r_amd.model import OptimParams, SplatModel
    m = SplatModel(3)
    for k, v in t.items():
        setattr(m, k, nn.Parameter(v.clone()))
    F = conf.shape[0]
    m._conf_static = nn.Parameter(conf.clone())
    m.aggregated_mask = torch.ones(conf.numel(), dtype=torch.bool, device="cuda")
    m._mask_index = torch.arange(conf.numel(), device="cuda")
    m.Q, m.T = nn.Parameter(torch.zeros(F, 4, device="cuda")), nn.Parameter(torch.zeros(F, 3, device="cuda"))
    m.training_setup(OptimParams(), fused=True)
    for k in t:
        p = getattr(m, k)
        shape = (p.shape[0], 0, 3) if k == "_features_rest" else tuple(p.shape)
        m.optimizer.state[p] = dict(step=100, exp_avg=torch.zeros(shape, device="cuda"), exp_avg_sq=torch.ones(shape, device="cuda"))
    return m


def event(t, conf, kernels):
    from das3r_amd.prune import prune_points
    m = make_model(t, conf)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    info = prune_points(m, min_opacity=0.005, use_kernels=kernels)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - base, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for name, (F, H, W) in SHAPES.items():
        for drop in (0.02, 0.25):
            t, conf = make_state(F, H, W, drop, seed=1)
            for kernels in (True, False):   # a warm-up of each
                event(t, conf, kernels)
            ms = {True: [], False: []}
            peak = {}
            for _ in range(args.repeats):
                for kernels in (True, False):
                    m, pk, info = event(t, conf, kernels)
                    ms[kernels].append(round(m, 3))
                    peak[kernels] = pk
            P, kept = info["before"], info["after"]
            row_bytes = (3 + 3 + 45 + 3 + 4 + 1) * 4 + (3 + 3 + 0 + 3 + 4 + 1) * 8 + 8   # parameters, two moments each (f_rest: none at degree 0), the index
            moved = P * 16 + 2 * kept * row_bytes
            best = {k: min(v) for k, v in ms.items()}
            rows.append(dict(shape=name, frames=F, image=[W, H], splats=P, drop_fraction=drop, kept=kept, bytes_moved=moved,
                             kernels_ms=ms[True], torch_ms=ms[False], kernels_best_ms=best[True], torch_best_ms=best[False],
                             kernels_gb_s=round(moved / best[True] / 1e6, 1), torch_gb_s=round(moved / best[False] / 1e6, 1),
                             float4_copy_gb_s=COPY_RATE_TBS * 1e3, kernels_peak_bytes=peak[True], torch_peak_bytes=peak[False]))
            print(json.dumps(rows[-1]), flush=True)
            del t, conf
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(what="one prune event, HIP path vs torch path (tools/prune_bench.py); ms include the one host read of the kept count",
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
