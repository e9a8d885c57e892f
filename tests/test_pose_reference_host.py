"""tests/pose_reference.py checked on the CPU against itself: the float64 reference against float64 autograd through das3r_amd/camera.py,
an op-by-op fp32 evaluation against every budget (the budgets are not too tight), every mutant against its bar (they are not too loose),
and the exact tier's claims.  No GPU: tests/test_gpu_pose_edges.py holds the kernels to the same reference and budgets.

Mutants and the kinds they apply to.  The three matrix mutants and the two chain mutants are rejected on every general kind (the pose of
every kind is off unit length by 3 % or more; on the exact tier |q| = 1 and Lq_normalised / chain_no_inv_norm are the true formulas: not
applicable there).  The three sum mutants are rejected on the `positive` kind and on the exact tier at P = 65 537 and 262 145;
sums_drop_row256 needs P > 65 536.  gconf_without_mask is rejected wherever there is a mask index (every kind; without one it IS the
kernel's behaviour)."""
import pytest
import torch

from tests import pose_reference as PR

HOST_P = (264, 2049)
PER_GAUSSIAN = ("means", "rotations", "scales", "opacities")
GRADS = ("g_xyz", "g_rotation", "g_scaling", "g_opacity_raw", "g_conf", "sums")


def _mats(d):
    """The 28 floats the kernel would write, as fp32 values (the op-by-op evaluation), split."""
    m = PR.matrices32(d["q"], d["t"])
    return m[:9], m[9:12], m[12:]


def _fwd_args(d):
    R, t, Lq = _mats(d)
    return [d[k] for k in PR.INPUT_NAMES] + [d["conf"], d["idx"], R, t, Lq]


def _bwd_args(d):
    R, _, Lq = _mats(d)
    return [d[k] for k in PR.INPUT_NAMES] + [d["conf"], d["idx"], R, Lq] + [d[k] for k in PR.UPSTREAM_NAMES]


def _rejected(mut, ref, tol):
    """-> names of the outputs on which the mutant leaves K x the budget."""
    return [k for k in ref if PR.worst_ratio(mut[k], ref[k], tol[k])[0] > PR.K]


@pytest.mark.parametrize("kind", PR.KINDS)
def test_reference_agrees_with_float64_autograd_through_camera_py(kind):
    """R and the rotated quaternion from das3r_amd.camera (quat_to_rotation, quat_multiply) in float64 — camera_from_tensor casts to float at
    its end, so R and t are assembled here as it assembles them — the loss sum(out * upstream) differentiated by autograd: every output of
    forward64 / backward64 and the pose gradient of pose_chain64(sums) to 1e-12 of the output's magnitude."""
    from das3r_amd.camera import quat_multiply, quat_to_rotation
    for seed in (0, 1):
        d = PR.make_general(kind, 264, seed)
        q, t = d["q"].double().requires_grad_(True), d["t"].double().requires_grad_(True)
        leaves = {k: d[k].double().requires_grad_(True) for k in PR.INPUT_NAMES + ("conf",)}
        R = quat_to_rotation(q[None])[0]
        out = dict(means=leaves["xyz"] @ R.t() + t, rotations=quat_multiply(q, leaves["rot"]), scales=torch.exp(leaves["scaling"]),
                   opacities=torch.sigmoid(leaves["opacity_raw"]) * leaves["conf"][d["idx"]][:, None])
        ups = dict(zip(PER_GAUSSIAN, (d[k].double() for k in PR.UPSTREAM_NAMES)))
        sum((out[k] * ups[k]).sum() for k in out).backward()
        m64 = PR.matrices64(d["q"], d["t"])[0]   # (float64 matrices of the fp32 pose: the reference's own, not the rounded ones)
        close = lambda a, b, mag, what, floor=0.0: PR.assert_within(a, b.detach(), 1e-12 * (mag + 1e-300) + floor, 1.0, f"autograd {kind} {what}")
        close(m64["R"].reshape(3, 3), R, 1.0 + 0 * R.detach(), "R")
        ref, mag, _ = PR.forward64(*[d[k] for k in PR.INPUT_NAMES], d["conf"], d["idx"], m64["R"], m64["t"], m64["Lq"])
        for k in PER_GAUSSIAN:
            close(ref[k], out[k], mag[k], k)
        ref, mag, _ = PR.backward64(*[d[k] for k in PR.INPUT_NAMES], d["conf"], d["idx"], m64["R"], m64["Lq"], *[d[k] for k in PR.UPSTREAM_NAMES])
        for k, leaf in (("g_xyz", "xyz"), ("g_rotation", "rot"), ("g_scaling", "scaling")):
            close(ref[k], leaves[leaf].grad, mag[k], k)
        # (autograd forms 1 - s from a rounded s: off by up to 2^-53 absolute, which is all of 1 - s at raw = 90 — the reference's own
        #  1 - s = e / (1 + e) has no such cancellation; the comparison allows autograd that much)
        cancel = 2.0 ** -52 * (d["g_opac"].double() * d["conf"].double()[d["idx"]][:, None]).abs()
        close(ref["g_opacity_raw"], leaves["opacity_raw"].grad, mag["g_opacity_raw"], "g_opacity_raw", cancel)
        placed, _ = PR.place_conf(ref["g_conf"], d["idx"], d["conf"].numel(), 0.0)
        mag_conf, _ = PR.place_conf(mag["g_conf"], d["idx"], d["conf"].numel(), 0.0)
        close(placed, leaves["conf"].grad, mag_conf, "g_conf")
        ch, chmag, _ = PR.pose_chain64(d["q"], ref["sums"])
        close(ch["g_q"], q.grad, chmag["g_q"], "g_q")
        close(ch["g_t"], t.grad, chmag["g_t"], "g_t")


@pytest.mark.parametrize("P", HOST_P)
@pytest.mark.parametrize("kind", PR.KINDS)
def test_fp32_evaluation_stays_within_every_budget(kind, P):
    """pretransform_math.h / pretransform_chain.h / the two pose kernels op by op in numpy float32 (expf correctly rounded), the 28 sums as
    one serial chain of fused multiply-adds and as a balanced tree of rounded products: the worst ratio to the budget is printed, at most 1."""
    worst = {}
    for seed in (0, 1):
        d = PR.make_general(kind, P, seed)
        m32 = PR.matrices32(d["q"], d["t"])
        ref, _, tol = PR.matrices64(d["q"], d["t"])
        for k, got in (("R", m32[:9]), ("t", m32[9:12]), ("Lq", m32[12:])):
            worst[k] = max(worst.get(k, 0.0), PR.assert_within(got, ref[k], tol[k], 1.0, f"fp32 {kind} {k}"))
        ref, _, tol = PR.forward64(*_fwd_args(d))
        got = PR.forward32(*_fwd_args(d))
        for k in PER_GAUSSIAN:
            worst[k] = max(worst.get(k, 0.0), PR.assert_within(got[k], ref[k], tol[k], 1.0, f"fp32 {kind} {k}"))
        for order in ("serial", "pairwise"):
            ref, _, tol = PR.backward64(*_bwd_args(d), depth=PR.sums32_depth(P, order))
            got = PR.backward32(*_bwd_args(d), order=order)
            for k in GRADS:
                name = f"{k} ({order})" if k == "sums" else k
                worst[name] = max(worst.get(name, 0.0), PR.assert_within(got[k], ref[k], tol[k], 1.0, f"fp32 {kind} {name}"))
            g28 = got["sums"]   # (fp32 values, as the chain kernel is handed them)
            ref, _, tol = PR.pose_chain64(d["q"], g28)
            gq, gt = PR.pose_chain32(d["q"], g28)
            for k, g in (("g_q", gq), ("g_t", gt)):
                worst[k] = max(worst.get(k, 0.0), PR.assert_within(g, ref[k], tol[k], 1.0, f"fp32 {kind} {k}"))
    print(f"[fp32 emulation {kind} P={P}] worst ratio to the budget: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("kind", PR.KINDS)
def test_matrix_and_chain_mutants_leave_their_budgets(kind):
    for seed in (0, 1):
        d = PR.make_general(kind, 264, seed)
        ref, _, tol = PR.matrices64(d["q"], d["t"])
        for m in PR.MATRIX_MUTANTS:
            assert _rejected(PR.matrices64(d["q"], d["t"], mutant=m)[0], ref, tol), (kind, seed, m)
        sums = PR.backward64(*_bwd_args(d))[0]["sums"].float()
        ref, _, tol = PR.pose_chain64(d["q"], sums)
        for m in PR.CHAIN_MUTANTS:
            assert "g_q" in _rejected(PR.pose_chain64(d["q"], sums, mutant=m)[0], ref, tol), (kind, seed, m)
        # a wrong matrix shows in what is computed with it, too: the per-Gaussian outputs of a transposed R / a right-multiplying Lq
        fref, _, ftol = PR.forward64(*_fwd_args(d))
        R, t, Lq = _mats(d)
        for m, out in (("R_transposed", "means"), ("Lq_right", "rotations")):
            mm = PR.matrices64(d["q"], d["t"], mutant=m)[0]
            mut = PR.forward64(*[d[k] for k in PR.INPUT_NAMES], d["conf"], d["idx"], mm["R"], t, mm["Lq"])[0]
            assert out in _rejected(mut, fref, ftol), (kind, seed, m)


@pytest.mark.parametrize("P", [65537, 262145])
def test_sum_mutants_leave_the_budget_on_positive_inputs_and_the_exact_tier(P):
    """A Gaussian or a row of the combine lost, or the clamped row counted: beyond the budget of das3r_pretransform_backward's depth on the
    `positive` kind (nothing cancels: a lost row shows at full size), and unequal to the int64 sums on the exact tier."""
    d = PR.general("positive", P)
    ref, _, tol = PR.backward64(*_bwd_args(d))
    e = PR.exact(P)
    want = PR.exact_sums(e)
    R, _, Lq = _mats(e)
    pose_only = lambda x: [x["xyz"], x["rot"], None, None, None, None, R, Lq, x["g_means"], x["g_rot"], None, None]
    assert torch.equal(PR.backward64(*pose_only(e))[0]["sums"], want.double())
    for m in PR.SUM_MUTANTS:
        for grid in (PR.grid_of(P, PR.CAP_BACKWARD), PR.grid_of(P, PR.CAP_ADAM), PR.grid_of(P)):
            mut = PR.backward64(*_bwd_args(d), mutant=m, grid=grid)[0]
            ratio = PR.worst_ratio(mut["sums"], ref["sums"], tol["sums"])[0]
            assert ratio > PR.K, (m, grid, ratio)
            got = PR.backward64(*pose_only(e), mutant=m, grid=grid)[0]["sums"]
            assert not torch.equal(got, want.double()), (m, grid)
            assert bool((got != want.double()).all()), "no input is zero: every one of the 28 sums moves"


@pytest.mark.parametrize("kind", PR.KINDS)
def test_conf_gradient_without_the_mask_index_is_rejected(kind):
    d = PR.general(kind, 264)
    ref, _, tol = PR.backward64(*_bwd_args(d))
    n = d["conf"].numel()
    want, written = PR.place_conf(ref["g_conf"], d["idx"], n, 777.0)
    budget, _ = PR.place_conf(tol["g_conf"], d["idx"], n, 0.0)
    got, written_m = PR.place_conf(ref["g_conf"], d["idx"], n, 777.0, mutant="gconf_without_mask")
    assert not torch.equal(written, written_m)
    assert PR.worst_ratio(got, want, budget)[0] > PR.K
    e = PR.exact(257)
    ev = PR.backward64(*_bwd_args(e))[0]["g_conf"]
    assert not torch.equal(PR.place_conf(ev, e["idx"], e["conf"].numel(), 777.0)[0], PR.place_conf(ev, e["idx"], e["conf"].numel(), 777.0, mutant="gconf_without_mask")[0])


@pytest.mark.parametrize("P", [1, 257, 262145, 1048653])
def test_exact_tier_is_exact(P):
    """make_exact: the op-by-op fp32 matrices are exactly the permutation and +-0.5, the int64 sums stay below 2^24, every reference value is
    a multiple of 1/16 that fp32 holds exactly, and (small P) the fp32 evaluation in either summation order EQUALS the reference."""
    e = PR.make_exact(P)
    m = PR.matrices32(e["q"], e["t"])
    assert torch.equal(m[:9].reshape(3, 3), torch.tensor(PR.EXACT_R)) and torch.equal(m[9:12], e["t"])
    assert bool((m[12:].abs() == 0.5).all())
    m64 = PR.matrices64(e["q"], e["t"])[0]
    assert torch.equal(torch.cat([m64["R"], m64["t"], m64["Lq"]]), m.double())
    sums = PR.exact_sums(e)
    assert int(sums.abs().max()) + int(e["prefill"].abs().max()) < 2 ** 24 and 6 * P + 3 < 2 ** 24
    fref = PR.forward64(*_fwd_args(e))[0]
    bref = PR.backward64(*_bwd_args(e))[0]
    assert torch.equal(bref["sums"], sums.double())
    for k, v in list(fref.items()) + list(bref.items()):
        assert torch.equal(v.float().double(), v) and torch.equal((v * 16).round(), v * 16), k
    assert torch.equal(fref["scales"], torch.ones(P, 3, dtype=torch.float64)) and torch.equal(fref["opacities"][:, 0], 0.5 * e["conf"][e["idx"]].double())
    if P <= 257:
        got = PR.forward32(*_fwd_args(e))
        assert all(torch.equal(got[k].double(), fref[k]) for k in PER_GAUSSIAN)
        for order in ("serial", "pairwise"):
            got = PR.backward32(*_bwd_args(e), order=order)
            assert all(torch.equal(got[k].double(), bref[k]) for k in GRADS), order


def test_sums_depth_reads_the_three_regimes():
    """1 serial term + 9 + rows per thread + 9 + 1: the second `u` slot from 257 rows, the second b0 iteration from 1025, the second
    grid-stride round behind the caps."""
    assert PR.sums_depth(1, PR.CAP_BACKWARD) == PR.sums_depth(65536, PR.CAP_BACKWARD) == 1 + 9 + 1 + 9 + 1
    assert PR.sums_depth(65537, PR.CAP_BACKWARD) == 22 and PR.sums_depth(262144, PR.CAP_BACKWARD) == 24
    assert PR.sums_depth(262145, PR.CAP_BACKWARD) == 1 + 9 + 4 + 9 + 2 and PR.sums_depth(262145, PR.CAP_ADAM) == PR.sums_depth(262145) == 1 + 9 + 5 + 9 + 1
    assert PR.sums_depth(524288, PR.CAP_ADAM) == 28 and PR.sums_depth(524289, PR.CAP_ADAM) == 29 and PR.sums_depth(1048653, PR.CAP_ADAM) == 30
    assert PR.grid_of(266240) == 1040 and PR.sums_depth(266240) == 1 + 9 + 5 + 9 + 1
