"""The bars of tests/adam_reference.py on the CPU: step64 is torch.optim.Adam's step, an op-by-op fp32 evaluation of adam_math.h stays
within K x budget of it on every kind, and float64 evaluations of WRONG formulas do not.  No kernel runs here: that the budgets bite is
proven by mutating the reference, tests/test_gpu_adam_edges.py then holds the kernels to the same budgets."""
import math

import pytest
import torch

from tests import adam_reference as A

N = 20000
STEPS = (1, 2, 7, 1000, 30000)
LR = 1.6e-4


def test_inputs_are_what_the_kinds_promise():
    for n in (1, 2, 257, 2049):
        for kind in A.KINDS:
            x = A.make_inputs(kind, n)
            assert set(x) == {"p", "m", "v", "g"} and all(t.dtype == torch.float32 and tuple(t.shape) == (n,) for t in x.values())
            assert all(bool(torch.isfinite(t).all()) for t in x.values()) and bool((x["v"] >= 0).all())
            again, other = A.make_inputs(kind, n), A.make_inputs(kind, n, seed=1)
            assert all(torch.equal(x[k], again[k]) for k in x)
            assert n < 257 or any(not torch.equal(x[k], other[k]) for k in x)
    n = 2049
    even = torch.arange(n) % 2 == 0
    x = A.make_inputs("general", n)
    assert 1e-9 * 0.99 <= float(x["g"].abs().min()) and float(x["g"].abs().max()) <= 1e3 * 1.01 and bool((x["g"] < 0).any()) and bool((x["g"] > 0).any())
    assert 1e-9 * 0.99 <= float(x["m"].abs().min()) and float(x["m"].abs().max()) <= 1e3 * 1.01 and float(x["p"].abs().max()) > 1.0
    r = (x["v"].double().sqrt() / x["g"].double().abs())[even]
    assert 0.0999 <= float(r.min()) and float(r.max()) <= 10.01
    x = A.make_inputs("first", n)
    assert not bool(x["m"].any()) and not bool(x["v"].any()) and bool(x["g"].all())
    x = A.make_inputs("p_zero", n)
    assert not bool(x["p"].any()) and bool(x["g"].all()) and bool(x["m"].all()) and bool(x["v"].all())
    x = A.make_inputs("g_zero", n)
    assert not bool(x["g"][even].any()) and bool(x["g"][~even].all()) and bool(x["m"].all())
    x = A.make_inputs("all_zero", n)
    for k in ("g", "m", "v"):
        assert not bool(x[k][even].any()) and bool(x[k][~even].all()), k
    assert bool(x["p"].all())
    x = A.make_inputs("large", n)
    assert float(x["g"].abs().max()) > 1e16 and float(x["g"].abs().max()) <= 1.01e17 and bool(torch.isfinite(x["g"] * x["g"]).all()) and float(x["v"].max()) > 1e30
    x = A.make_inputs("tiny", n)
    assert float(x["g"].abs().min()) < 1e-29 and float(x["g"].abs().max()) <= 1.01e-15 and bool(x["g"].all())
    assert not bool(x["m"][even].any()) and not bool(x["v"][even].any()) and bool(x["m"][~even].all())
    assert bool(((x["v"] > 0) & (x["v"] < A.ETA)).any()), "subnormal second moments"
    x = A.make_inputs("decay", n)
    assert not bool(x["g"].any()) and bool(x["m"].all())
    assert bool(((x["m"] != 0) & (x["m"].abs() < A.ETA)).any()) and bool(((x["v"] > 0) & (x["v"] < A.ETA)).any()), "subnormal moments"


def test_the_betas_are_where_one_minus_beta_is_exact():
    import numpy as np
    for b in (A.BETA1, A.BETA2, 0.5, 1.0):
        assert float(np.float32(1.0) - np.float32(b)) == 1.0 - float(np.float32(b))
    with pytest.raises(AssertionError):
        A.step64(*(torch.zeros(1),) * 4, 0.25, A.BETA2, A.EPS, 1e-3, 1.0)


@pytest.mark.parametrize("t", [1, 2, 50])
def test_step64_is_one_step_of_torch_adam(t):
    """torch.optim.Adam on float64 CPU tensors: its step number t against step64 from the state before it, with step_size and bc2_sqrt
    computed as torch computes them (lr / (1 - beta1^t), sqrt(1 - beta2^t) in double)."""
    gen = torch.Generator().manual_seed(t)
    n, lr, betas, eps = 300, 2.5e-3, (A.BETA1, A.BETA2), 1e-15
    p = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    for k in range(t):
        if k == t - 1:
            st = opt.state.get(p)
            before = (p.detach().clone(), torch.zeros(n, dtype=torch.float64) if not st else st["exp_avg"].clone(),
                      torch.zeros(n, dtype=torch.float64) if not st else st["exp_avg_sq"].clone())
        p.grad = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (k % 5 - 2)
        opt.step()
    ref, _ = A.step64(*before, p.grad, betas[0], betas[1], eps, lr / (1.0 - betas[0] ** t), math.sqrt(1.0 - betas[1] ** t))
    for name, got in (("p", p.detach()), ("m", opt.state[p]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"])):
        assert float(((got - ref[name]).abs() / ref[name].abs().clamp_min(1e-300)).max()) <= 1e-13, name
    assert int(opt.state[p]["step"]) == t


@pytest.mark.parametrize("kind", A.KINDS)
def test_fp32_op_by_op_stays_within_the_budgets(kind):
    """numpy float32, every operation of adam_math.h rounded once: within K x budget for every kind and step count, the plain step with the
    host's corrections and the gated step with the corrections the gated kernel computes."""
    x = A.inputs(kind, N)
    worst = {}
    for t in STEPS:
        step_size, bc2_sqrt = A.host_corrections(LR, t)
        ref, tol = A.step64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, step_size, bc2_sqrt)
        got = A.step32(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, step_size, bc2_sqrt)
        for name in ("p", "m", "v"):
            worst[name] = max(worst.get(name, 0.0), A.assert_within(got[name], ref[name], tol[name], A.K, f"fp32 op-by-op {name} [{kind} t={t}]"))
        ref, tol = A.gated64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, A.f32(LR), t)
        got = A.step32(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, *A.gated_corrections32(LR, t))
        worst["gated p"] = max(worst.get("gated p", 0.0), A.assert_within(got["p"], ref["p"], tol["p"], A.K, f"fp32 op-by-op gated p [{kind} t={t}]"))
    print(f"[{kind}] " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))


def test_all_zero_elements_have_the_budget_zero():
    x = A.inputs("all_zero", N)
    even = torch.arange(N) % 2 == 0
    for t in STEPS:
        ref, tol = A.step64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, *A.host_corrections(LR, t))
        gref, gtol = A.gated64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, A.f32(LR), t)
        for r, b in ((ref, tol), (gref, gtol)):
            for name in ("p", "m", "v"):
                assert float(b[name][even].abs().max()) == 0.0 and float(b[name][~even].min()) > 0.0, name
            assert torch.equal(r["p"][even], x["p"][even].double()) and not bool(r["m"][even].any()) and not bool(r["v"][even].any())
    moved = x["p"].clone()
    moved[0] = torch.nextafter(moved[0], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match="element 0"):
        A.assert_within(moved, ref["p"], tol["p"], A.K, "one ulp on an untouched element")


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_a_wrong_formula_leaves_the_budget_on_p_zero(mutant):
    """Each mutant, in float64, leaves K x the p budget on at least 99 % of the `p_zero` elements it applies to (tail_rate_for_head: the
    head columns of a split-rate tensor; bc_multiplied: t <= 1000, beyond which bc2_sqrt is 1 to within the budget)."""
    x = A.inputs("p_zero", N)
    is_head = torch.arange(N) % 48 < 3
    tail = A.f32(LR / 20.0)
    for t in STEPS:
        step_size, bc2_sqrt = A.host_corrections(LR, t)
        args = (x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, step_size, bc2_sqrt, A.f32(tail / (1 - A.BETA1 ** t)), is_head)
        ref, tol = A.step64(*args)
        bad, _ = A.step64(*args, mutant=mutant)
        out = (bad["p"] - ref["p"]).abs() > A.K * tol["p"]
        applies = is_head if mutant == "tail_rate_for_head" else torch.ones(N, dtype=torch.bool)
        frac = float(out[applies].float().mean())
        print(f"[{mutant} t={t}] {100 * frac:.2f} % of {int(applies.sum())} elements leave the budget")
        if mutant == "bc_multiplied" and t > 1000:
            continue
        assert frac >= 0.99, (mutant, t, frac)
        if mutant == "tail_rate_for_head":
            assert not bool(out[~applies].any())


def test_step_1e_6_hides_behind_a_parameter_of_order_one():
    """Why p_zero: with p ~ N(0, 1) the same mutant is visible on a minority of the elements only."""
    x = A.inputs("general", N)
    args = (x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, *A.host_corrections(LR, 7))
    ref, tol = A.step64(*args)
    bad, _ = A.step64(*args, mutant="step_1e-6")
    assert float(((bad["p"] - ref["p"]).abs() > A.K * tol["p"]).float().mean()) < 0.5


def test_eps_inside_sqrt_is_held_to_no_bar():
    """With eps = 1e-15 the mutant moves d by eps / (2 v') of itself: nothing a test could rely on.  Printed, not asserted."""
    x = A.inputs("p_zero", N)
    args = (x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, *A.host_corrections(LR, 7))
    ref, tol = A.step64(*args)
    bad, _ = A.step64(*args, mutant="eps_inside_sqrt")
    print(f"[eps_inside_sqrt] {100 * float(((bad['p'] - ref['p']).abs() > A.K * tol['p']).float().mean()):.2f} % of the elements leave the budget")
