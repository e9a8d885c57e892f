"""Float64 / int64 restatement of the pose pre-transform (das3r_amd/csrc/pretransform.hip with pretransform_math.h and
pretransform_chain.h: the pose matrices and their chain rule, the per-Gaussian forward and backward, the camera's 28 sums), the inputs it
is tested on and the error budgets it is held to.  Plain module, CPU tensors only: tests/test_pose_reference_host.py proves on the CPU
that the budgets accept an op-by-op fp32 evaluation and reject wrong formulas, tests/test_gpu_pose_edges.py holds the kernels to them.
assert_within / worst_ratio are tests/loss_reference.py's.

Reference.  Every function takes the fp32 VALUES the kernel is handed (the per-Gaussian functions take R, t, Lq as fp32 numbers too — the
28 floats das3r_pose_matrices wrote) and computes in float64.  Each returns three dicts: the value, its MAGNITUDE — the sum of the absolute
values of the terms added into it — and the budget (without K):
    matrices64(q, t)      -> R (9, row-major: rotation of q / |q|), t (3), Lq (16, row-major: left multiplication by the RAW q)
    forward64(...)        -> means = R x + t, rotations = Lq rot, scales = exp(scaling), opacities = sigmoid(raw) conf[idx]
    backward64(...)       -> g_xyz = R^T g, g_rotation = Lq^T g, g_scaling = g exp(scaling), g_opacity_raw = g conf s (1 - s),
                             g_conf = g s (one value per Gaussian: place_conf puts them into the confidence map), sums (28):
                             dL/dR = sum g x^T (9), dL/dt = sum g (3), dL/dLq = sum g_rot rot^T (16)
    pose_chain64(q, g28)  -> g_q (4), g_t (3): dL/dR through R(q / |q|) — entry-wise derivative d, projection d - c (c . d) with c = q / |q|,
                             factor 1 / |q| — plus dL/dLq through the linear Lq(q); g_t = g28[9 .. 12)

Budgets, u = 2^-24, first order, from the roundings the two headers spell out; K = 1.001 covers the second-order terms and nothing else.
A sum of terms each of which passes through at most `depth` roundings is off by at most depth u magnitude, in whatever order it is taken.
    means      fl(fma(c, z, fma(b, y, fl(a x))) + t): a x passes 4 roundings                                   4 u (|a x| + |b y| + |c z| + |t|)
    rotations  fma(d, w, fma(c, z, fma(b, y, fl(a x))))                                                        4 u magnitude
    g_xyz      fma(c, z, fma(b, y, fl(a x)))                                                                   3 u magnitude
    g_rotation as rotations                                                                                    4 u magnitude
    expf       the one number the project's code does not give.  The ROCm install at hand carries no document that states an error bound
               for device expf, so it was measured: over every `scaling` and every `-opacity_raw` (handed to the forward as a `scaling`:
               its `scales` output IS expf of it) of the general-tier inputs of tests/test_gpu_pose_edges.py — all kinds at P = 264 and
               65 537, plain and positive at 262 145; results that are normal fp32 numbers, 4.1 M values — the worst
               |expf(x) - exp(x)| / (u exp(x)) on an MI355X is EXPF_MEASURED_U = 1.372 (1.3720 on positive / 262 145 / scaling, 1.3689 on
               plain / 262 145 / -opacity_raw; 0.568 at +-20; expf(90) = inf and expf(-90) = 8.194e-40, a subnormal: the underflow terms
               below).  Allowed is twice that, EXPF_U = 2.744, as a relative error in units of u.  The GPU test prints the figure of
               its `scaling` again on every run.
    scales     expf alone                                                                                      EXPF_U u exp(x)
    g_scaling  fl(g expf(x))                                                                                   (EXPF_U + 1) u |g exp(x)|
    sigmoid    e = expf(-raw); d = fl(1 + e): dd = EXPF_U u e + u d; s = fl(1 / d): ds = s (dd / d + u) = u s (EXPF_U e / d + 2)
    opacities  fl(s c)                                                                                         c ds + u |s c|
    g_conf     fl(g s)                                                                                         |g| ds + u |g s|
    g_opacity_raw  fl(fl(fl(g c) s) fl(1 - s)): fl(1 - s) is off by ds + u (1 - s) (the subtraction is exact for s >= 1/2, Sterbenz; the
               term is kept for s < 1/2), three rounded products                     |g c| (ds (1 - s) + s (ds + u (1 - s))) + 3 u |g c s (1 - s)|
    Underflow  eta = 2^-126.  Where the float64 value of s, 1 - s or of one of the three outputs is nonzero and below 2 eta — a saturated
               sigmoid: expf(90) is inf and the kernel's s an exact 0; expf(-90) is a subnormal that 1 + e swallows — every rounding may
               lose eta instead of u times the value: opacities += (c + 1) eta, g_conf += (|g| + 1) eta, g_opacity_raw += (|g c| + 2) eta
               (s on its way in times its factor, the products after it).
    sums       read off pretransform_backward_kernel and pose_sums_finish, for P Gaussians on a grid of G workgroups of 256 threads:
               ceil(P / (256 G)) serial fused multiply-adds per thread (the product is exact inside the fma: one rounding each)
               + 6 steps of the wave tree + 3 adds of the four waves
               + ceil(G / 256) row adds per thread of the last workgroup + 6 + 3 of the second tree + 1 for `g_small +=`
               = sums_depth(P, cap): depth u sum |g x|.  G = min(ceil(P / 256), cap), cap = 1024 for das3r_pretransform_backward and
               das3r_pretransform_pose_sums, 2048 for das3r_pretransform_backward_adam, none for the rasterizer's chained backward (one
               Gaussian per thread).  A bound by depth and magnitude holds for any order of summation: it covers all three.
    matrices   n2 = w w + x x + y y + z z: 4 roundings on positive terms, 4 u; n = sqrt: 2 u + 1; inv = 1 / n: 4 u; a component c = q inv:
               5 u; a product of two: 11 u; their sum or difference: 12; the doubling is exact; 1 - ...: one more.  D_MATS = 13:
               13 u magnitude with magnitude = 1 + 2 jj + 2 kk on the diagonal, 2 |i j| + 2 |r k| off it.  t and Lq are copies: budget 0.
               (sqrtf and the division are correctly rounded: the library is built without fast-math.)
    pose chain d_a = sum of 6 or 8 terms +-2 c G or -4 c G: c 5 u, the product 1 (the factor 2 or 4 is exact), at most 7 adds: 13 u mag_d,
               mag_d = sum |coef c G|.  dot = sum c_a d_a: (5 + 13 + 1 + 3) u = 22 u magdot, magdot = sum |c_a| mag_d_a.
               g_q[a] = fl(fl(d_a - fl(c_a dot)) inv) + fl(H + H + H + H): d_a has passed 13 + 1 (the subtraction) + 4 + 1 (inv, the
               product) + 1 (the last add) = 20 roundings, c_a dot 5 + 22 + 1 + 1 + 5 + 1 = 35, the H terms 3 + 1 = 4:
               u (20 mag_d_a / n + 35 |c_a| magdot / n + 4 sum |H|).  g_t is a copy: budget 0.
               A budget on g28 (two summation orders compared with each other) goes through the same map with |.| in every place:
               pose_chain64(q, g28, g28_tol) adds it.

Exact tier.  make_exact(P, seed): pose quaternion (0.5, 0.5, 0.5, 0.5) — |q| = 1, R the permutation matrix [[0,0,1],[1,0,0],[0,1,0]], Lq of
entries +-0.5 — integer t, xyz and rot in +-{1, 2, 3}, upstream gradients of means and rotations in +-{1, 2} (none is zero: a missing or
doubled Gaussian moves every one of the 28 sums), scaling = 0 (exp = 1), opacity_raw = 0 (sigmoid = 0.5), conf in {0.25, 0.5, 1},
g_scales and g_opac in +-{1, 2, 3}.  Every product and every partial sum is a multiple of 1/16 below 2^24 — at most 6 P <= 6.3 M in the
sums — so fp32 arithmetic is exact in any order, and so is the float64 of the reference functions: the kernels' outputs must EQUAL them.
exact_sums restates the 28 sums in int64.

General tier.  make_general(kind, P, seed), deterministic; the mask index is a sorted random subset of a confidence map of
P + P // 3 + 5 entries:
    plain      the distribution of tests/test_gpu_fused.py _inputs: xyz ~ 2 N, rot ~ N, scaling ~ N - 2, opacity_raw ~ N, conf ~ U(0, 1),
               q = (0.9, 0.1, -0.2, 0.3) + 0.05 N (norm about 0.97), t ~ N; upstream gradients ~ N
    offunit    plain with q scaled to norm OFFUNIT_NORMS[seed % 2] = 0.2 or 3
    far        xyz = (600, -800, 500) + 50 N and t = -R (600, -800, 500): |R x| ~ 1e3 and |R x + t| ~ 50
    saturated  opacity_raw from {20, -20, 90, -90}, scaling from {20, -20}
    positive   |.| + 0.1 of plain's xyz, rot and of the upstream gradients of means and rotations: nothing cancels in the sums

Mutants (of the reference, in float64: every difference is the formula's; tests/test_pose_reference_host.py holds each to its bar):
    R_transposed, Lq_right (right multiplication), Lq_normalised (Lq of q / |q|)                            matrices64
    chain_no_projection (d, not d - c (c . d)), chain_no_inv_norm (without 1 / |q|)                          pose_chain64
    sums_drop_last, sums_drop_row256 (Gaussians 65 536 .. 65 791), sums_last_row_twice (the clamped row)     backward64
    gconf_without_mask (g_conf written at i, not at idx[i])                                                  place_conf"""
import functools
import math

import numpy as np
import torch

from tests.loss_reference import assert_within, worst_ratio  # noqa: F401  (the one copy of the assertion)

U = 2.0 ** -24
ETA = 2.0 ** -126
K = 1.001
EXPF_MEASURED_U = 1.372   # worst |expf(x) - exp(x)| / (u exp(x)) of device expf over the general-tier inputs, MI355X
EXPF_U = 2.0 * EXPF_MEASURED_U
D_MATS = 13
KINDS = ("plain", "offunit", "far", "saturated", "positive")
OFFUNIT_NORMS = (0.2, 3.0)
MATRIX_MUTANTS = ("R_transposed", "Lq_right", "Lq_normalised")
CHAIN_MUTANTS = ("chain_no_projection", "chain_no_inv_norm")
SUM_MUTANTS = ("sums_drop_last", "sums_drop_row256", "sums_last_row_twice")
CONF_MUTANTS = ("gconf_without_mask",)
CAP_FORWARD, CAP_BACKWARD, CAP_ADAM = 4096, 1024, 2048   # largest grids of pretransform.hip's launches
EXACT_Q = (0.5, 0.5, 0.5, 0.5)
EXACT_R = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
INPUT_NAMES = ("xyz", "rot", "scaling", "opacity_raw")
UPSTREAM_NAMES = ("g_means", "g_rot", "g_scales", "g_opac")


def _d(x):
    return x.detach().double().cpu() if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float64)


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def grid_of(P, cap=None):
    g = _ceil_div(P, 256)
    return g if cap is None else min(g, cap)


def sums_depth(P, cap=None):
    """The largest number of roundings a term of the 28 sums passes through (module docstring: sums)."""
    G = grid_of(P, cap)
    return _ceil_div(P, 256 * G) + 9 + _ceil_div(G, 256) + 9 + 1


# ---------------------------------------------------------------------------------------------------------------- the pose matrices
def _rotation_terms(c):
    """-> (R [9], magnitude [9]) of the rotation of the unit quaternion c = (r, i, j, k), float64."""
    r, i, j, k = (c[a] for a in range(4))
    one = torch.ones((), dtype=torch.float64)
    pairs = [(None, j * j, k * k), (i * j, -r * k), (i * k, r * j), (i * j, r * k), (None, i * i, k * k), (j * k, -r * i), (i * k, -r * j), (j * k, r * i),
             (None, i * i, j * j)]
    R, mag = [], []
    for p in pairs:
        if p[0] is None:
            R.append(one - 2 * (p[1] + p[2]))
            mag.append(one + 2 * (p[1].abs() + p[2].abs()))
        else:
            R.append(2 * (p[0] + p[1]))
            mag.append(2 * (p[0].abs() + p[1].abs()))
    return torch.stack(R), torch.stack(mag)


def _left(q):
    w, x, y, z = (q[a] for a in range(4))
    return torch.stack([w, -x, -y, -z, x, w, -z, y, y, z, w, -x, z, -y, x, w])


def _right(q):
    w, x, y, z = (q[a] for a in range(4))
    return torch.stack([w, -x, -y, -z, x, w, z, -y, y, -z, w, x, z, y, -x, w])


def matrices64(q, t, mutant=None):
    """-> (ref, mag, tol): dicts of R [9], t [3], Lq [16] — what pose_matrices_kernel writes."""
    q, t = _d(q).reshape(4), _d(t).reshape(3)
    n = q.pow(2).sum().sqrt()
    R, magR = _rotation_terms(q / n)
    if mutant == "R_transposed":
        R = R.reshape(3, 3).t().reshape(9)
    Lq = _right(q) if mutant == "Lq_right" else _left(q / n) if mutant == "Lq_normalised" else _left(q)
    ref = dict(R=R, t=t.clone(), Lq=Lq)
    mag = dict(R=magR, t=t.abs(), Lq=Lq.abs())
    tol = dict(R=D_MATS * U * magR, t=torch.zeros(3, dtype=torch.float64), Lq=torch.zeros(16, dtype=torch.float64))
    return ref, mag, tol


# the entry-wise derivative of R(r, i, j, k): d[a] = sum coef * c[comp] * G[entry]   (pose_chain_kernel's dr, di, dj, dk)
_DR = (((-2, 3, 1), (2, 2, 2), (2, 3, 3), (-2, 1, 5), (-2, 2, 6), (2, 1, 7)),
       ((2, 2, 1), (2, 3, 2), (2, 2, 3), (-4, 1, 4), (-2, 0, 5), (2, 3, 6), (2, 0, 7), (-4, 1, 8)),
       ((-4, 2, 0), (2, 1, 1), (2, 0, 2), (2, 1, 3), (2, 3, 5), (-2, 0, 6), (2, 3, 7), (-4, 2, 8)),
       ((-4, 3, 0), (-2, 0, 1), (2, 1, 2), (2, 0, 3), (-4, 3, 4), (2, 2, 5), (2, 1, 6), (2, 2, 7)))
# dL/dLq -> dL/dq: g_q[a] += sum sign * H[entry]
_DL = (((1, 0), (1, 5), (1, 10), (1, 15)), ((-1, 1), (1, 4), (-1, 11), (1, 14)), ((-1, 2), (1, 7), (1, 8), (-1, 13)), ((-1, 3), (-1, 6), (1, 9), (1, 12)))


def _chain_abs(c, inv, G):
    """The pose chain with |.| in every place: (mag_d [4], magdot, sum |H| [4]) for non-negative G [28]."""
    mag_d = torch.stack([sum(abs(coef) * c[comp].abs() * G[e] for coef, comp, e in terms) for terms in _DR])
    magdot = (c.abs() * mag_d).sum()
    magH = torch.stack([sum(G[12 + e] for _, e in terms) for terms in _DL])
    return mag_d, magdot, magH


def pose_chain64(q, g28, g28_tol=None, mutant=None):
    """-> (ref, mag, tol): dicts of g_q [4], g_t [3].  g28_tol: a budget on g28 itself, carried through (module docstring)."""
    q, G = _d(q).reshape(4), _d(g28).reshape(28)
    n = q.pow(2).sum().sqrt()
    inv, c = 1.0 / n, q / n
    d = torch.stack([sum(coef * c[comp] * G[e] for coef, comp, e in terms) for terms in _DR])
    proj = d if mutant == "chain_no_projection" else d - c * (c * d).sum()
    gq = proj * (1.0 if mutant == "chain_no_inv_norm" else inv)
    gq = gq + torch.stack([sum(sign * G[12 + e] for sign, e in terms) for terms in _DL])
    mag_d, magdot, magH = _chain_abs(c, inv, G.abs())
    mag_q = inv * (mag_d + c.abs() * magdot) + magH
    tol_q = U * (20.0 * inv * mag_d + 35.0 * inv * c.abs() * magdot + 4.0 * magH)
    tol_t = torch.zeros(3, dtype=torch.float64)
    if g28_tol is not None:
        T = _d(g28_tol).reshape(28)
        t_d, t_dot, t_H = _chain_abs(c, inv, T)
        tol_q = tol_q + inv * (t_d + c.abs() * t_dot) + t_H
        tol_t = tol_t + T[9:12]
    return dict(g_q=gq, g_t=G[9:12].clone()), dict(g_q=mag_q, g_t=G[9:12].abs()), dict(g_q=tol_q, g_t=tol_t)


# ---------------------------------------------------------------------------------------------------------------- per Gaussian
def _low(x):
    return (x != 0) & (x.abs() < 2.0 * ETA)


def _sigmoid(raw):
    """-> (s, 1 - s, ds): the sigmoid in float64 without cancellation, and the budget of the kernel's s."""
    e = torch.exp(-raw)
    s = torch.where(raw >= 0, 1.0 / (1.0 + e), torch.exp(raw) / (1.0 + torch.exp(raw)))
    oms = torch.where(raw >= 0, e / (1.0 + e), 1.0 / (1.0 + torch.exp(raw)))
    frac = torch.where(torch.isfinite(e), e / (1.0 + e), torch.ones_like(e))   # e / d
    ds = U * s * (EXPF_U * frac + 2.0)
    return s, oms, ds


def _conf_of(conf_flat, idx, P):
    conf_flat = _d(conf_flat).reshape(-1)
    return conf_flat[:P] if idx is None else conf_flat[idx.cpu().long()]


def forward64(xyz, rot, scaling, opacity_raw, conf_flat, idx, R, t, Lq):
    """-> (ref, mag, tol): dicts of means [P,3], rotations [P,4], scales [P,3], opacities [P,1]."""
    x, r, sc, o = _d(xyz), _d(rot), _d(scaling), _d(opacity_raw).reshape(-1)
    P = x.shape[0]
    Rm, tv, L = _d(R).reshape(3, 3), _d(t).reshape(3), _d(Lq).reshape(4, 4)
    c = _conf_of(conf_flat, idx, P)
    means, mag_means = x @ Rm.t() + tv, x.abs() @ Rm.abs().t() + tv.abs()
    rots, mag_rots = r @ L.t(), r.abs() @ L.abs().t()
    scales = torch.exp(sc)
    s, oms, ds = _sigmoid(o)
    op = s * c
    low = _low(s) | _low(oms) | _low(op)
    tol_op = c.abs() * ds + U * op.abs() + (c.abs() + 1.0) * ETA * low
    ref = dict(means=means, rotations=rots, scales=scales, opacities=op.reshape(P, 1))
    mag = dict(means=mag_means, rotations=mag_rots, scales=scales, opacities=op.abs().reshape(P, 1))
    tol = dict(means=4.0 * U * mag_means, rotations=4.0 * U * mag_rots, scales=EXPF_U * U * scales, opacities=tol_op.reshape(P, 1))
    return ref, mag, tol


def _sum_weights(P, grid, mutant):
    """How often each Gaussian is counted in the 28 sums: 1, or what a mutant makes of it."""
    w = torch.ones(P, dtype=torch.float64)
    if mutant == "sums_drop_last":
        w[P - 1] = 0.0
    elif mutant == "sums_drop_row256":
        assert P > 65536, "row 256 of the combine exists from 65 537 Gaussians on"
        w[65536:min(P, 65792)] = 0.0
    elif mutant == "sums_last_row_twice":
        row = (torch.arange(P) // 256) % grid
        w[row == grid - 1] = 2.0
    return w


def backward64(xyz, rot, scaling, opacity_raw, conf_flat, idx, R, Lq, g_means, g_rot, g_scales, g_opac, depth=None, mutant=None, grid=None):
    """-> (ref, mag, tol): dicts of g_xyz [P,3], g_rotation [P,4], g_scaling [P,3], g_opacity_raw [P,1], g_conf [P] (one value per Gaussian:
    place_conf) and sums [28].  depth: of the 28 sums (sums_depth; default: das3r_pretransform_backward's grid).  scaling .. conf_flat and
    g_scales, g_opac may be None (the pose sums alone).  grid: of the launch, for the row mutant."""
    x, r, gm, gr = _d(xyz), _d(rot), _d(g_means), _d(g_rot)
    P = x.shape[0]
    Rm, L = _d(R).reshape(3, 3), _d(Lq).reshape(4, 4)
    depth = sums_depth(P, CAP_BACKWARD) if depth is None else depth
    w = _sum_weights(P, grid_of(P, CAP_BACKWARD) if grid is None else grid, mutant)
    wm, wr = gm * w[:, None], gr * w[:, None]
    sums = torch.cat([(wm.t() @ x).reshape(9), wm.sum(0), (wr.t() @ r).reshape(16)])
    mag_sums = torch.cat([(gm.abs().t() @ x.abs()).reshape(9), gm.abs().sum(0), (gr.abs().t() @ r.abs()).reshape(16)])
    ref, mag, tol = dict(sums=sums), dict(sums=mag_sums), dict(sums=depth * U * mag_sums)
    ref["g_xyz"], mag["g_xyz"] = gm @ Rm, gm.abs() @ Rm.abs()
    ref["g_rotation"], mag["g_rotation"] = gr @ L, gr.abs() @ L.abs()
    tol["g_xyz"], tol["g_rotation"] = 3.0 * U * mag["g_xyz"], 4.0 * U * mag["g_rotation"]
    if scaling is None:
        return ref, mag, tol
    sc, o, gs, go = _d(scaling), _d(opacity_raw).reshape(-1), _d(g_scales), _d(g_opac).reshape(-1)
    c = _conf_of(conf_flat, idx, P)
    ref["g_scaling"] = gs * torch.exp(sc)
    mag["g_scaling"] = ref["g_scaling"].abs()
    tol["g_scaling"] = (EXPF_U + 1.0) * U * mag["g_scaling"]
    s, oms, ds = _sigmoid(o)
    gc = (go * c).abs()
    ro, gconf = go * c * s * oms, go * s
    low = _low(s) | _low(oms) | _low(ro) | _low(gconf)
    ref["g_opacity_raw"], mag["g_opacity_raw"] = ro.reshape(P, 1), ro.abs().reshape(P, 1)
    tol["g_opacity_raw"] = (gc * (ds * oms + s * (ds + U * oms)) + 3.0 * U * ro.abs() + (gc + 2.0) * ETA * low).reshape(P, 1)
    ref["g_conf"], mag["g_conf"] = gconf, gconf.abs()
    tol["g_conf"] = go.abs() * ds + U * gconf.abs() + (go.abs() + 1.0) * ETA * low
    return ref, mag, tol


def place_conf(values, idx, n_conf, fill, mutant=None):
    """The confidence gradient as the kernel leaves it: `values` at the mask positions of a buffer prefilled with `fill`, float64.
    -> (buffer, written: bool mask of the positions that hold a value)."""
    values = _d(values).reshape(-1)
    P = values.shape[0]
    at = torch.arange(P) if idx is None or mutant == "gconf_without_mask" else idx.cpu().long()
    out = torch.full((n_conf,), float(fill), dtype=torch.float64)
    out[at] = values
    written = torch.zeros(n_conf, dtype=torch.bool)
    written[at] = True
    return out, written


# ---------------------------------------------------------------------------------------------------------------- inputs
def _pick(gen, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(len(values), shape, generator=gen)]


def _mask_index(gen, P, n_conf):
    return torch.sort(torch.randperm(n_conf, generator=gen)[:P]).values.contiguous()


def make_exact(P, seed=0, prefill_max=3):
    """Integer-valued fp32 inputs on which every product and partial sum is exact (module docstring) -> dict of CPU tensors."""
    gen = torch.Generator().manual_seed(7001 * seed + P)
    n_conf = P + P // 3 + 5
    pm = lambda vals, shape: _pick(gen, [s * v for v in vals for s in (1.0, -1.0)], shape)
    d = dict(q=torch.tensor(EXACT_Q), t=torch.tensor([3.0, -2.0, 5.0]), xyz=pm((1.0, 2.0, 3.0), (P, 3)), rot=pm((1.0, 2.0, 3.0), (P, 4)),
             scaling=torch.zeros(P, 3), opacity_raw=torch.zeros(P, 1), conf=_pick(gen, (0.25, 0.5, 1.0), (n_conf,)), idx=_mask_index(gen, P, n_conf),
             g_means=pm((1.0, 2.0), (P, 3)), g_rot=pm((1.0, 2.0), (P, 4)), g_scales=pm((1.0, 2.0, 3.0), (P, 3)), g_opac=pm((1.0, 2.0, 3.0), (P, 1)))
    d["prefill"] = pm((1.0, 2.0, 3.0), (28,))   # what g_small may hold before the launch: the sums are added to it
    assert float(d["prefill"].abs().max()) <= prefill_max
    bound = 6 * P + prefill_max   # |g x| <= 2 x 3 per Gaussian, in whatever order the partial sums are formed
    assert bound < 2 ** 24, f"partial sums up to {bound} are not exact in fp32"
    assert float((d["g_means"].abs().max(0).values[:, None] * d["xyz"].abs().max(0).values[None, :]).max()) <= 6.0
    assert float((d["g_rot"].abs().max(0).values[:, None] * d["rot"].abs().max(0).values[None, :]).max()) <= 6.0
    assert all(bool((d[k] != 0).all()) for k in ("xyz", "rot", "g_means", "g_rot", "g_scales", "g_opac"))
    return d


def exact_sums(d):
    """The 28 sums of a make_exact case in int64."""
    x, r, gm, gr = (d[k].to(torch.int64) for k in ("xyz", "rot", "g_means", "g_rot"))
    assert all(torch.equal(a.float(), d[k]) for a, k in ((x, "xyz"), (r, "rot"), (gm, "g_means"), (gr, "g_rot")))
    return torch.cat([(gm.t() @ x).reshape(9), gm.sum(0), (gr.t() @ r).reshape(16)])


def make_general(kind, P, seed=0):
    """-> dict of CPU fp32 tensors (idx: int64), deterministic (module docstring: general tier)."""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * KINDS.index(kind) + P)
    n_conf = P + P // 3 + 5
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    d = dict(xyz=rn(P, 3) * 2, rot=rn(P, 4), scaling=rn(P, 3) - 2, opacity_raw=rn(P, 1), conf=torch.rand(n_conf, generator=gen),
             q=torch.tensor([0.9, 0.1, -0.2, 0.3]) + 0.05 * rn(4), t=rn(3), g_means=rn(P, 3), g_rot=rn(P, 4), g_scales=rn(P, 3), g_opac=rn(P, 1))
    d["idx"] = _mask_index(gen, P, n_conf)
    if kind == "plain":
        pass
    elif kind == "offunit":
        d["q"] = (d["q"].double() / d["q"].double().norm() * OFFUNIT_NORMS[seed % 2]).float()
    elif kind == "far":
        centre = torch.tensor([600.0, -800.0, 500.0])
        d["xyz"] = centre + 50.0 * rn(P, 3)
        R = matrices64(d["q"], d["t"])[0]["R"].reshape(3, 3)
        d["t"] = (-(R @ centre.double())).float()
    elif kind == "saturated":
        d["opacity_raw"] = _pick(gen, (20.0, -20.0, 90.0, -90.0), (P, 1))
        d["scaling"] = _pick(gen, (20.0, -20.0), (P, 3))
    elif kind == "positive":
        for k in ("xyz", "rot", "g_means", "g_rot"):
            d[k] = d[k].abs() + 0.1
    else:
        raise KeyError(kind)
    d = {k: v.contiguous() for k, v in d.items()}
    assert all(bool(torch.isfinite(v).all()) for k, v in d.items() if k != "idx"), kind
    return d


@functools.lru_cache(maxsize=None)
def general(kind, P, seed=0):
    """make_general, shared by the tests and never modified."""
    return make_general(kind, P, seed)


@functools.lru_cache(maxsize=None)
def exact(P, seed=0):
    """make_exact, shared by the tests and never modified."""
    return make_exact(P, seed)


# ---------------------------------------------------------------------------------------------------------------- fp32, op by op
_F = np.float32


def _np32(x):
    return np.asarray(_d(x).numpy(), dtype=np.float64).astype(_F)


def _fma32(a, b, c):
    """fma in fp32: the float64 product of two fp32 numbers is exact, the sum is rounded to float64 and once more to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_F)


def _expf32(x):
    """A correctly rounded expf (u relative): within EXPF_U by construction — the device's own error is measured on the device."""
    with np.errstate(all="ignore"):
        return np.exp(x.astype(np.float64)).astype(_F)


def matrices32(q, t):
    """pose_matrices_kernel op by op (without contraction: the most roundings) -> fp32 tensor [28]."""
    q, t = _np32(q).reshape(4), _np32(t).reshape(3)
    w, x, y, z = q
    inv = _F(1.0) / np.sqrt(w * w + x * x + y * y + z * z)
    r, i, j, k = w * inv, x * inv, y * inv, z * inv
    one, two = _F(1.0), _F(2.0)
    R = [one - two * (j * j + k * k), two * (i * j - r * k), two * (i * k + r * j), two * (i * j + r * k), one - two * (i * i + k * k),
         two * (j * k - r * i), two * (i * k - r * j), two * (j * k + r * i), one - two * (i * i + j * j)]
    L = [w, -x, -y, -z, x, w, -z, y, y, z, w, -x, z, -y, x, w]
    out = np.array(R + list(t) + L, dtype=_F)
    return torch.from_numpy(out)


def pose_chain32(q, g28):
    """pose_chain_kernel op by op (without contraction) -> (g_q [4], g_t [3]) fp32 tensors."""
    q, G = _np32(q).reshape(4), _np32(g28).reshape(28)
    w, x, y, z = q
    n = np.sqrt(w * w + x * x + y * y + z * z)
    inv = _F(1.0) / n
    c = [w * inv, x * inv, y * inv, z * inv]
    d = []
    for terms in _DR:
        acc = None
        for coef, comp, e in terms:
            term = _F(coef) * c[comp] * G[e]
            acc = term if acc is None else _F(acc + term)
        d.append(acc)
    dot = _F(_F(_F(c[0] * d[0] + c[1] * d[1]) + c[2] * d[2]) + c[3] * d[3])
    gq = []
    for a in range(4):
        h = None
        for sign, e in _DL[a]:
            term = _F(sign) * G[12 + e]
            h = term if h is None else _F(h + term)
        gq.append(_F(_F(_F(d[a] - _F(c[a] * dot)) * inv) + h))
    return torch.from_numpy(np.array(gq, dtype=_F)), torch.from_numpy(G[9:12].copy())


def _sigmoid32(o):
    with np.errstate(all="ignore"):
        return _F(1.0) / (_F(1.0) + _expf32(-o))


def forward32(xyz, rot, scaling, opacity_raw, conf_flat, idx, R, t, Lq):
    """pretransform_math.h op by op in numpy float32 -> dict of fp32 tensors."""
    x, r, sc, o = _np32(xyz), _np32(rot), _np32(scaling), _np32(opacity_raw).reshape(-1)
    Rm, tv, L = _np32(R).reshape(3, 3), _np32(t).reshape(3), _np32(Lq).reshape(4, 4)
    c = _np32(_conf_of(conf_flat, idx, x.shape[0]))
    col = lambda m, a: np.broadcast_to(m[a], (x.shape[0],))
    means = np.stack([_fma32(col(Rm[a], 2), x[:, 2], _fma32(col(Rm[a], 1), x[:, 1], col(Rm[a], 0) * x[:, 0])) + tv[a] for a in range(3)], 1)
    rots = np.stack([_fma32(col(L[a], 3), r[:, 3], _fma32(col(L[a], 2), r[:, 2], _fma32(col(L[a], 1), r[:, 1], col(L[a], 0) * r[:, 0]))) for a in range(4)], 1)
    out = dict(means=means, rotations=rots, scales=_expf32(sc), opacities=(_sigmoid32(o) * c).reshape(-1, 1))
    assert all(v.dtype == _F for v in out.values())
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def _serial32(ga, xa):
    """sum_i ga[i] xa[i] as a chain of fused multiply-adds from 0, columns in parallel -> fp32 [columns]."""
    acc = np.zeros(ga.shape[1], dtype=_F)
    for i in range(ga.shape[0]):
        acc = _fma32(ga[i], xa[i], acc)
    return acc


def _pairwise32(ga, xa):
    """sum_i of the ROUNDED products, added in a balanced binary tree."""
    v = (ga * xa).astype(_F)
    n = 1 << max(0, (v.shape[0] - 1).bit_length())
    v = np.concatenate([v, np.zeros((n - v.shape[0], v.shape[1]), dtype=_F)])
    while v.shape[0] > 1:
        v = (v[0::2] + v[1::2]).astype(_F)
    return v[0]


def sums32_depth(P, order):
    """The depth of backward32's 28 sums: P for the serial chain, 1 (the product) + ceil(log2 P) for the tree."""
    return P if order == "serial" else 1 + max(0, (P - 1).bit_length())


def backward32(xyz, rot, scaling, opacity_raw, conf_flat, idx, R, Lq, g_means, g_rot, g_scales, g_opac, order="serial"):
    """pretransform_chain.h op by op in numpy float32; the 28 sums in the given order ("serial" or "pairwise") -> dict of fp32 tensors."""
    x, r, sc, o = _np32(xyz), _np32(rot), _np32(scaling), _np32(opacity_raw).reshape(-1)
    gm, gr, gs, go = _np32(g_means), _np32(g_rot), _np32(g_scales), _np32(g_opac).reshape(-1)
    P = x.shape[0]
    Rm, L = _np32(R).reshape(3, 3), _np32(Lq).reshape(4, 4)
    c = _np32(_conf_of(conf_flat, idx, P))
    b = lambda v: np.broadcast_to(v, (P,))
    g_xyz = np.stack([_fma32(b(Rm[2, a]), gm[:, 2], _fma32(b(Rm[1, a]), gm[:, 1], b(Rm[0, a]) * gm[:, 0])) for a in range(3)], 1)
    g_rotation = np.stack([_fma32(b(L[3, a]), gr[:, 3], _fma32(b(L[2, a]), gr[:, 2], _fma32(b(L[1, a]), gr[:, 1], b(L[0, a]) * gr[:, 0]))) for a in range(4)], 1)
    s = _sigmoid32(o)
    with np.errstate(all="ignore"):
        out = dict(g_xyz=g_xyz, g_rotation=g_rotation, g_scaling=gs * _expf32(sc), g_opacity_raw=(((go * c) * s) * (_F(1.0) - s)).reshape(-1, 1), g_conf=go * s)
    add = _serial32 if order == "serial" else _pairwise32
    # columns: dR[a][b] = sum g[a] x[b]; dt[a] = sum g[a] (a product with 1 is exact); dLq[a][b] = sum g_rot[a] rot[b]
    ga = np.concatenate([np.repeat(gm, 3, axis=1), gm, np.repeat(gr, 4, axis=1)], 1)
    xa = np.concatenate([np.tile(x, (1, 3)), np.ones((P, 3), dtype=_F), np.tile(r, (1, 4))], 1)
    out["sums"] = add(ga, xa)
    assert all(v.dtype == _F for v in out.values())
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def ratios(got, ref, tol, names):
    return {name: worst_ratio(got[name], ref[name], tol[name])[0] for name in names}
