"""The bars of tests/loss_reference.py on the CPU: fp32 torch ops (das3r_amd.losses in fp32, the behaviour the loss kernels replace) stay
within K x budget of the float64 reference on every kind x shape, and float64 evaluations of WRONG formulas do not.  No kernel runs here:
that the budgets bite is proven by mutating the reference, tests/test_gpu_loss_edges.py then holds the kernels to the same budgets."""
import pytest
import torch

from tests import loss_reference as R

LAM, GRAD = 0.2, 3.0
CASES = [(kind, hw) for kind in R.KINDS for hw in R.HOST_SHAPES]
ids = lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}"


def test_inputs_are_what_the_kinds_promise():
    for H, W in R.HOST_SHAPES:
        for kind in R.KINDS:
            r, t, s = R.make_inputs(kind, H, W)
            assert r.dtype == t.dtype == s.dtype == torch.float32 and r.shape == t.shape == (3, H, W) and s.shape == (H, W)
            assert torch.equal(r * 4096, (r * 4096).round()) and torch.equal(t * 4096, (t * 4096).round()) and torch.equal(s * 64, (s * 64).round())
            assert float(r.min()) >= 0 and float(r.max()) <= 1 and float(s.min()) >= 0 and float(s.max()) <= 1
            a, b = R.make_inputs(kind, H, W)[0], R.make_inputs(kind, H, W, seed=1)[0]
            assert torch.equal(a, r) and (kind in ("black", "step") or H * W < 4 or not torch.equal(a, b))
        eq = lambda kind: torch.equal(*R.make_inputs(kind, H, W)[:2])
        assert eq("equal") and eq("equal_flat") and eq("black") and float(R.make_inputs("black", H, W)[0].abs().max()) == 0
        r, t, s = R.make_inputs("ties", H, W)
        assert bool((r == t).any()), "a `ties` image holds a tie at every shape, 1 x 1 included"
        assert H * W < 16 or (bool((r != t).any()) and not eq("uniform"))
        s = R.make_inputs("masked", H, W)[2]
        assert bool((s == 0).any()) and set(s.unique().tolist()) <= {0.0, 1.0} and (H * W == 1 or bool((s == 1).any()))
        r, t, _ = R.make_inputs("flat_bright", H, W)
        assert float(r.min()) >= 0.979 and float(t.max()) <= 0.973
        r, t, _ = R.make_inputs("step", H, W)
        assert set(r.unique().tolist()) | set(t.unique().tolist()) <= {0.0, 1.0}


def test_the_restated_ssim_is_the_librarys():
    from das3r_amd.losses import ssim
    r, t, s = R.make_inputs("uniform", 17, 33)
    a, b = r.double() * s.double(), t.double() * s.double()
    assert float((R.ssim_restated(a, b) - ssim(a, b, size_average=False)).abs().max()) <= 1e-13
    for mutant in ("replicate", "sigma", "c2", "bias"):
        assert float((R.ssim_restated(a, b, mutant) - ssim(a, b, size_average=False)).abs().max()) > 1e-6, mutant


def test_assert_within_demands_exact_zeros_and_names_the_pixel():
    ref, tol = torch.zeros(3, 20, 40, dtype=torch.float64), torch.full((3, 20, 40), 1e-9, dtype=torch.float64)
    tol[1, 17, 35] = 0.0
    got = ref.clone()
    assert R.assert_within(got, ref, tol, 4.0, "all equal") == 0.0
    got[2, 3, 4] = 4e-9
    assert R.assert_within(got, ref, tol, 4.0, "at the bar") == pytest.approx(4.0)
    got[1, 17, 35] = 1e-30
    with pytest.raises(AssertionError, match=r"channel 1, \(y, x\) = \(17, 35\) of 20 x 40, \(y % 16, x % 16\) = \(1, 3\), 2 from the border"):
        R.assert_within(got, ref, tol, 4.0, "a budget of 0")
    got[1, 17, 35] = float("nan")
    with pytest.raises(AssertionError, match="channel 1"):
        R.assert_within(got, ref, tol, 4.0, "not finite")
    with pytest.raises(AssertionError, match="element 2"):
        R.assert_within(torch.tensor([0.0, 0.0, 1.0]), torch.zeros(3), torch.full((3,), 0.1), 4.0, "vector")
    with pytest.raises(AssertionError, match="scalar"):
        R.assert_within(torch.tensor(1.0), torch.tensor(0.0), torch.tensor(0.1), 4.0, "scalar")


def test_assert_within_reports_to_the_tolerance_report(tmp_path, monkeypatch):
    import json
    path = tmp_path / "tol.jsonl"
    monkeypatch.setenv("DAS3R_TOL_REPORT", str(path))
    R.assert_within(torch.tensor([1.0, 2.5]), torch.tensor([1.0, 2.0]), torch.tensor([0.0, 0.25]), 4.0, "some output")
    (row,) = [json.loads(line) for line in open(path)]
    assert row["kind"] == "budget_ratio" and row["what"] == "some output" and row["value"] == 2.0 and row["tol"] == 4.0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fp32_torch_ops_stay_within_the_budgets(case):
    """The reference alone stays within the bars: both photometric forms and the ssim_map form in fp32 on the CPU, at the committed K."""
    kind, (H, W) = case
    for exposure in (None, R.EXPOSURE_B):
        inputs, ref, tol = R.plain_case(kind, H, W, LAM, GRAD, exposure)
        got = R.photometric(*inputs, LAM, GRAD, exposure, dtype=torch.float32)
        for name, K in R.PLAIN_OUTPUTS:
            if ref[name] is not None:
                R.assert_within(got[name], ref[name], tol[name], K, f"fp32 torch {'exposure' if exposure else 'plain'} {name} [{kind} {H}x{W}]")
        assert bool((got["d_render"][:, inputs[2] == 0] == 0).all())
    inputs, ref, tol = R.map_case(kind, H, W)
    got = R.ssim_map(*inputs, dtype=torch.float32)
    for name, K in R.MAP_OUTPUTS:
        R.assert_within(got[name], ref[name], tol[name], K, f"fp32 torch ssim_map {name} [{kind} {H}x{W}]")


def _rejected(kind, H, W, mutant):
    """Does any output of the float64 mutant leave K x budget?  (Plain form with its map; the ssim_map form for the SSIM mutants.)"""
    inputs, ref, tol = R.plain_case(kind, H, W, LAM, GRAD)
    bad = {n: v for n, v in R.ratios(R.photometric(*inputs, LAM, GRAD, mutant=mutant), ref, tol, R.PLAIN_OUTPUTS).items() if v > dict(R.PLAIN_OUTPUTS)[n]}
    if mutant != "tie":
        inputs, ref, tol = R.map_case(kind, H, W)
        bad.update({"ssim_map " + n: v for n, v in R.ratios(R.ssim_map(*inputs, mutant=mutant), ref, tol, R.MAP_OUTPUTS).items() if v > dict(R.MAP_OUTPUTS)[n]})
    return bad


@pytest.mark.parametrize("hw", R.HOST_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_a_wrong_formula_is_rejected(mutant, hw):
    """Replicate padding, window sigma 1.51, C2 x 1.01, m x (1 + 1e-4), d|x|/dx = +1 at ties — each in float64, so every difference is the
    formula's: rejected by at least one kind at every shape; the bias by EVERY kind; the tie rule by every kind that holds a tie."""
    H, W = hw
    hits = {kind: _rejected(kind, H, W, mutant) for kind in R.KINDS}
    print(f"[{mutant} {H}x{W}] " + "; ".join(f"{k}: {max(v.values()):.3g}x" if v else f"{k}: -" for k, v in hits.items()))
    assert any(hits.values()), (mutant, hw)
    if mutant == "bias":
        assert all(hits.values()), {k: bool(v) for k, v in hits.items()}
    if mutant == "tie":
        for kind in ("ties", "equal", "equal_flat", "black"):
            assert "d_render" in hits[kind], (kind, hits[kind])   # (d static sees no tie where render == gt: its two terms cancel)
        assert not hits["flat_bright"], "no tie, no difference"
    if mutant == "replicate" and H > 11 and W > 11:
        assert hits["uniform"] and hits["flat_bright"]
