"""Float64 restatement of the one Adam update every optimizer kernel applies (das3r_amd/csrc/adam_math.h: adam.hip's plain and gated
steps, the step inside das3r_pretransform_backward_adam), the inputs it is tested on and the error budgets it is held to.  Plain module,
CPU tensors only: tests/test_adam_reference_host.py proves on the CPU that the budgets accept an op-by-op fp32 evaluation and reject wrong
formulas, tests/test_gpu_adam_edges.py holds the kernels to them.  assert_within is tests/loss_reference.py's.

Reference.  step64(p, m, v, g, beta1, beta2, eps, step_size, bc2_sqrt): the inputs are the fp32 VALUES the kernel is handed (the fp32
betas and eps, step_size and bc2_sqrt as passed), the arithmetic is float64:
    m' = m + (g - m)(1 - beta1)        v' = beta2 v + (1 - beta2) g^2        d = sqrt(v') / bc2_sqrt + eps        p' = p - step_size m' / d
1 - beta is EXACT in fp32 for 0.5 <= beta <= 1 (Sterbenz: the difference of two floats within a factor two of each other), so the kernel's
`1.0f - beta` and the reference's 1 - beta are the same number; the betas of every test stay in that range.

Budgets, u = 2^-24, from the roundings adam_math.h spells out (first order; K = 1.001 covers the second-order terms and nothing else):
    m' = fma(fl(g - m), 1 - beta1, m): two roundings, u (1 - beta1)|g - m| through the product and u |m'| at the end
        tol_m = u (|m'| + (1 - beta1)|g - m|)
    v' = fma(fl((1 - beta2) g), g, fl(v beta2)): three roundings of non-negative terms that sum to v' (the two inner ones share v'
        between them, so 2 u v' is what they reach; the budget states the plain count)
        tol_v = 3 u v'
    d = fl(fl(sqrt(v') / bc2_sqrt) + eps): sqrt halves the 2 u of v' and adds its own (2 u), the division 3 u, the sum 4 u (eps is exact)
    p' = fma(-step_size, fl(m' / d), p): the quotient carries m's error, the 4 u of d and its own rounding, the product is exact inside
        the fma, the sum rounds once:
        tol_p = u |p'| + u step_size / d (6 |m'| + (1 - beta1)|g - m|)          (6 = 1 of m' + 4 of d + 1 of the quotient)
    Where m' is an exact 0 the update is an exact 0 and fma(-s, 0, p) = p: the term u |p'| is dropped there, and an element with
    g = m = v = 0 has the budget 0 for all three outputs (assert_within then demands p bit-unchanged and m = v = 0).
Underflow.  eta = 2^-126, the smallest normal: a result below it is rounded to a multiple of 2^-149, or flushed to 0 by a build without
fp32 denormals, as is an input below it — an absolute error of at most eta either way.  Where a nonzero input or exact intermediate lies
below 2 eta (and only there: the term vanishes everywhere else, zeros included):
    tol_m += 4 eta                      (m and g on the way in, g - m, the result)
    tol_v += (4 + |g|) eta              (v on the way in, fl((1 - beta2) g) times g, fl(v beta2), the result, v' into sqrt)
    d:  |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(a)), so E_v = (4 + |g|) eta reaches d as
        dd = min(sqrt(E_v), E_v / sqrt(v')) / bc2_sqrt, and p' as step_size |m'| dd / (d (d - dd))   (exact in dd, which need not be small
        beside d: with eps = 1e-15 a flushed v ~ 1e-40 moves d by 3e-4 of itself)
    tol_p += step_size (4 eta / d + eta) + eta       (m's term through the quotient, the quotient's own, the result's)

Gated step.  gated64(...) takes the plain learning rate and the integer step count t, computes bc1 = 1 - beta1^t and bc2 = 1 - beta2^t
in float64 from the fp32 betas, and allows the kernel each correction to 4 u relative: 4 u of bc1 in step_size, 2 u of bc2 through the
square root, u each for the division lr / bc1 and the root — 8 u on the update:
    tol_p(gated) = tol_p + 8 u step_size / d |m'|

Mutants (of the reference, in float64: every difference is the formula's): v_uses_beta1, bc_multiplied (d = sqrt(v') bc2_sqrt + eps),
old_m (the update from m, not m'), step_1e-6 (step_size (1 + 1e-6)), tail_rate_for_head (the tail's rate on the head columns of a
split-rate tensor) — each leaves the p budget on >= 99 % of the `p_zero` elements it applies to (host test) — and eps_inside_sqrt
(d = sqrt(v' + eps) / bc2_sqrt), which eps = 1e-15 makes nearly invisible: it moves d by eps / (2 v') of itself, beyond the budget only
where v' < ~1e-8, i.e. for gradients below 1e-4 (28 % of the log-uniform `p_zero` elements, none of a tensor whose gradients are of
the workload's size).  It is there for completeness and held to no bar.

Inputs.  make_inputs(kind, n, seed) -> dict(p, m, v, g) of fp32 [n] tensors, deterministic:
    general   |g|, |m| log-uniform in 1e-9 .. 1e3 with random signs, v = (|g| r)^2 with r log-uniform in 0.1 .. 10 on the even elements
              and the square of an independent magnitude on the odd ones, p ~ N(0, 1)
    first     general with m = v = 0 (the first step of a tensor)
    p_zero    general with p = 0: the update is observed at full precision, not behind u |p| (the kind that bites)
    g_zero    general with every second gradient exactly 0
    all_zero  general with g = m = v = 0 on every second element
    large     |g|, |m| log-uniform in 1e10 .. 1e17, v up to 1e34: g^2 stays finite in fp32
    tiny      |g| log-uniform in 1e-30 .. 1e-15; m = v = 0 on the even elements, |m| in 1e-30 .. 1e-18 and v in 1e-44 .. 1e-36 on the odd
    decay     g = 0, |m| in 1e-42 .. 1e-30, v in 1e-45 .. 1e-36: a Gaussian unseen for a thousand steps, down into the subnormals"""
import functools
import math

import numpy as np
import torch

from tests.loss_reference import assert_within, worst_ratio  # noqa: F401  (the one copy of the assertion)

U = 2.0 ** -24
ETA = 2.0 ** -126
K = 1.001
KINDS = ("general", "first", "p_zero", "g_zero", "all_zero", "large", "tiny", "decay")
MUTANTS = ("v_uses_beta1", "bc_multiplied", "old_m", "step_1e-6", "tail_rate_for_head")
UNHELD_MUTANTS = ("eps_inside_sqrt",)
f32 = lambda x: float(np.float32(x))
BETA1, BETA2, EPS = f32(0.9), f32(0.999), f32(1e-15)   # the fp32 values the kernels are handed


def _logu(gen, n, lo, hi):
    return torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _sign(gen, n):
    return torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()


def make_inputs(kind, n, seed=0):
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * KINDS.index(kind) + n)
    g = _logu(gen, n, 1e-9, 1e3) * _sign(gen, n)
    m = _logu(gen, n, 1e-9, 1e3) * _sign(gen, n)
    r, w = _logu(gen, n, 0.1, 10.0), _logu(gen, n, 1e-9, 1e3)
    even = torch.arange(n) % 2 == 0
    v = torch.where(even, (g.abs() * r) ** 2, w ** 2)
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    tg, tm, tv = _logu(gen, n, 1e-30, 1e-15) * _sign(gen, n), _logu(gen, n, 1e-30, 1e-18) * _sign(gen, n), _logu(gen, n, 1e-44, 1e-36)
    dm, dv = _logu(gen, n, 1e-42, 1e-30) * _sign(gen, n), _logu(gen, n, 1e-45, 1e-36)
    zero = torch.zeros(n, dtype=torch.float64)
    if kind == "general":
        pass
    elif kind == "first":
        m, v = zero, zero
    elif kind == "p_zero":
        p = zero
    elif kind == "g_zero":
        g = torch.where(even, zero, g)
    elif kind == "all_zero":
        g, m, v = torch.where(even, zero, g), torch.where(even, zero, m), torch.where(even, zero, v)
    elif kind == "large":
        g, m = g.sign() * _logu(gen, n, 1e10, 1e17), m.sign() * _logu(gen, n, 1e10, 1e17)
        v = torch.where(even, (g.abs() * r) ** 2, _logu(gen, n, 1e10, 1e17) ** 2)
    elif kind == "tiny":
        g, m, v = tg, torch.where(even, zero, tm), torch.where(even, zero, tv)
    elif kind == "decay":
        g, m, v = zero, dm, dv
    else:
        raise KeyError(kind)
    out = {k: t.float().contiguous() for k, t in dict(p=p, m=m, v=v, g=g).items()}
    assert all(bool(torch.isfinite(t).all()) for t in out.values()) and bool((out["v"] >= 0).all()), kind
    return out


# ---------------------------------------------------------------------------------------------------------------- the formula, and its mutants
def _d(x):
    return x.detach().double().cpu() if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float64)   # (a Python float is a double)


def step64(p, m, v, g, beta1, beta2, eps, step_size, bc2_sqrt, step_size_tail=None, is_head=None, mutant=None, extra_p=0.0):
    """-> (ref, tol): dicts of p, m, v after the step in float64 and their budgets (without K).  step_size / bc2_sqrt: floats or tensors
    broadcast against p.  step_size_tail, is_head: a split-rate tensor — is_head elements step with step_size, the others with
    step_size_tail.  extra_p: units of u step_size / d |m'| added to tol_p (the gated step's 8)."""
    p, m, v, g = _d(p), _d(m), _d(v), _d(g)
    beta1, beta2, eps = float(beta1), float(beta2), float(eps)
    assert 0.5 <= beta1 <= 1.0 and 0.5 <= beta2 <= 1.0, "1 - beta is exact in fp32 for beta in [0.5, 1] only"
    step, bc2_sqrt = _d(step_size) + torch.zeros_like(p), _d(bc2_sqrt) + torch.zeros_like(p)
    if step_size_tail is not None:
        tail = _d(step_size_tail) + torch.zeros_like(p)
        step = tail if mutant == "tail_rate_for_head" else torch.where(is_head, step, tail)
    if mutant == "step_1e-6":
        step = step * (1.0 + 1e-6)
    omb1, omb2 = 1.0 - beta1, 1.0 - beta2
    m1 = m + (g - m) * omb1
    v1 = (beta1 * v + omb1 * g * g) if mutant == "v_uses_beta1" else (beta2 * v + omb2 * g * g)
    if mutant == "bc_multiplied":
        d = v1.sqrt() * bc2_sqrt + eps
    elif mutant == "eps_inside_sqrt":
        d = (v1 + eps).sqrt() / bc2_sqrt
    else:
        d = v1.sqrt() / bc2_sqrt + eps
    p1 = p - step * (m if mutant == "old_m" else m1) / d
    dgm = omb1 * (g - m).abs()
    tol_m = U * (m1.abs() + dgm)
    tol_v = 3.0 * U * v1
    tol_p = U * p1.abs() * (m1 != 0) + U * step / d * ((6.0 + extra_p) * m1.abs() + dgm)
    # underflow: only where a nonzero input or exact intermediate is below 2 eta
    low = lambda x: (x != 0) & (x.abs() < 2.0 * ETA)
    uf_m = low(m) | low(g) | low(g - m) | low((g - m) * omb1) | low(m1)
    uf_v = low(v) | low(g) | low(omb2 * g) | low(omb2 * g * g) | low(v * beta2) | low(v1)
    E_v = (4.0 + g.abs()) * ETA * uf_v
    tol_m = tol_m + 4.0 * ETA * uf_m
    tol_v = tol_v + E_v
    s1 = v1.sqrt()
    dd = torch.minimum(E_v.sqrt(), torch.where(s1 > 0, E_v / s1.clamp_min(1e-300), E_v.sqrt())) / bc2_sqrt
    assert bool((dd < 0.5 * d).all()), "the underflow term of d must stay below d (eps too small for this budget)"
    q = m1.abs() / d
    tol_p = tol_p + step * m1.abs() * dd / (d * (d - dd)) + (step * (4.0 * ETA / d + ETA)) * uf_m + ETA * (low(q) | low(step * q) | low(p1) | low(p))
    return dict(p=p1, m=m1, v=v1), dict(p=tol_p, m=tol_m, v=tol_v)


def corrections64(beta1, beta2, t):
    """-> (bc1, bc2_sqrt) in float64 from the betas as given and the integer step count."""
    return 1.0 - float(beta1) ** int(t), math.sqrt(1.0 - float(beta2) ** int(t))


def gated64(p, m, v, g, beta1, beta2, eps, lr, t, lr_tail=None, is_head=None, mutant=None):
    """The gated kernel's step number t with the plain learning rate(s): corrections in float64, 8 u more on the update."""
    bc1, bc2_sqrt = corrections64(beta1, beta2, t)
    return step64(p, m, v, g, beta1, beta2, eps, _d(lr) / bc1, bc2_sqrt, None if lr_tail is None else _d(lr_tail) / bc1, is_head, mutant, extra_p=8.0)


def host_corrections(lr, t, beta1=BETA1, beta2=BETA2):
    """-> (step_size, bc2_sqrt) as fp32 values: what a caller that computes them in double hands das3r_adam_step."""
    bc1, bc2_sqrt = corrections64(beta1, beta2, t)
    return f32(lr / bc1), f32(bc2_sqrt)


# ---------------------------------------------------------------------------------------------------------------- fp32, op by op
def _fma32(a, b, c):
    """fma in fp32: the float64 product of two fp32 numbers is exact, the sum is rounded to float64 and once more to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def step32(p, m, v, g, beta1, beta2, eps, step_size, bc2_sqrt):
    """adam_math.h op by op in numpy float32 -> dict(p, m, v) of fp32 tensors."""
    p, m, v, g = (np.asarray(_d(x).numpy(), dtype=np.float64).astype(np.float32) for x in (p, m, v, g))
    one = np.float32(1.0)
    b1, b2, e = np.float32(beta1), np.float32(beta2), np.float32(eps)
    s, bc = (np.broadcast_to(np.asarray(_d(x).numpy()).astype(np.float32), p.shape) for x in (step_size, bc2_sqrt))
    with np.errstate(all="ignore"):
        m1 = _fma32(g - m, np.broadcast_to(one - b1, p.shape), m)
        v1 = _fma32((one - b2) * g, g, v * b2)
        den = np.sqrt(v1) / bc + e
        p1 = _fma32(-s, m1 / den, p)
    assert m1.dtype == v1.dtype == den.dtype == p1.dtype == np.float32
    return dict(p=torch.from_numpy(p1.copy()), m=torch.from_numpy(m1.copy()), v=torch.from_numpy(v1.copy()))


def gated_corrections32(lr, t, beta1=BETA1, beta2=BETA2):
    """The gated kernel's corrections as it computes them: 1 - beta^t in double, rounded to fp32; then fp32 division and root."""
    bc1 = np.float32(1.0 - float(beta1) ** int(t))
    bc2 = np.float32(1.0 - float(beta2) ** int(t))
    return float(np.float32(lr) / bc1), float(np.sqrt(bc2))


# ---------------------------------------------------------------------------------------------------------------- shared, computed once
@functools.lru_cache(maxsize=None)
def inputs(kind, n, seed=0):
    """make_inputs, shared by the tests and never modified."""
    return make_inputs(kind, n, seed)


def ratios(got, ref, tol):
    return {name: worst_ratio(got[name], ref[name], tol[name])[0] for name in ("p", "m", "v")}
