"""The pose pre-transform kernels (das3r_amd/csrc/pretransform.hip: das3r_pose_matrices[_qt], das3r_pose_chain[_qt[_rearm]],
das3r_pretransform_forward / _backward / _backward_adam / _pose_sums) at every regime of their grids and of the fixed-order row combine
(pretransform_chain.h pose_sums_finish), called through the C ABI.

Exact tier (tests/pose_reference.py make_exact: integer-valued inputs, every product and partial sum exact in fp32): the outputs EQUAL the
int64 / exact reference — no tolerance.  The sizes are the smallest at which each path exists: 255 / 256 / 257 (one workgroup, two),
65 536 / 65 537 (256 rows of the combine, a thread's second row), 262 144 / 262 145 (1024 rows; behind das3r_pretransform_backward's cap
of 1024 workgroups a second grid-stride round, for the Adam form row 1025 and the combine's second outer iteration), 524 288 / 524 289 /
524 293 (2048 rows, a second round of the Adam form; a third of the plain one), 1 048 576 / 1 048 577 (the forward's cap of 4096),
1 048 653 (a third round for 77 threads of the Adam form).

General tier (make_general: plain, offunit, far, saturated, positive): within K x the budgets derived in tests/pose_reference.py from the
roundings of the two headers, against float64.  Every test prints its worst ratio per output; the device's expf error is printed too.
The kernels' ratios on an MI355X are recorded in profiles/pose_edges_tol_report.txt: 0.2 - 0.9 per Gaussian, and 0.001 - 0.09 on the 28
sums — a bound by depth and magnitude is a worst case that random roundings of mixed signs stay far below, which is why the sums have the
exact tier: there a single Gaussian or row lost, doubled or read stale is an inequality at any size."""
import ctypes as C

import pytest
import torch

from tests import pose_reference as PR

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
PER_GAUSSIAN = ("means", "rotations", "scales", "opacities")
GRAD_NAMES = ("g_xyz", "g_rotation", "g_scaling", "g_opacity_raw")
LRS = (1.6e-4, 1e-3, 5e-3, 0.05)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15


def _lib():
    from das3r_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Dev:
    """A case's tensors on the device, the pose matrices the kernel makes of its pose, and the four entry points."""

    def __init__(self, d, masked=True):
        self.d, self.P = d, d["xyz"].shape[0]
        self.L, self.lib = _lib()
        for k in PR.INPUT_NAMES + PR.UPSTREAM_NAMES + ("conf", "q", "t"):
            setattr(self, k, d[k].cuda().contiguous())
        self.idx_host = d["idx"] if masked else None
        self.idx = d["idx"].cuda() if masked else None
        assert self.idx is None or (self.idx.dtype == torch.int64 and self.conf.numel() > self.P)
        self.mats = torch.full((28,), float("nan"), device="cuda")
        self.L.check(self.lib.das3r_pose_matrices_qt(_p(self.q), _p(self.t), _p(self.mats), None), "das3r_pose_matrices_qt")
        self.R, self.tv, self.Lq = C.c_void_p(self.mats.data_ptr()), C.c_void_p(self.mats.data_ptr() + 36), C.c_void_p(self.mats.data_ptr() + 48)

    def params(self):
        return [getattr(self, k).clone() for k in PR.INPUT_NAMES]

    def host_mats(self):
        m = self.mats.cpu()
        return m[:9], m[9:12], m[12:]

    def forward(self):
        P = self.P
        out = [torch.full((P, c), float("nan"), device="cuda") for c in (3, 4, 3, 1)]
        self.L.check(self.lib.das3r_pretransform_forward(P, _p(self.xyz), _p(self.rot), _p(self.scaling), _p(self.opacity_raw), _p(self.conf), _p(self.idx),
                                                         self.R, self.tv, self.Lq, *(_p(t) for t in out), None), "das3r_pretransform_forward")
        torch.cuda.synchronize()
        return dict(zip(PER_GAUSSIAN, (t.cpu() for t in out)))

    def _conf_and_small(self, prefill):
        g_conf = torch.full_like(self.conf, SENTINEL)
        small = torch.zeros(28, device="cuda") if prefill is None else prefill.cuda().clone()
        return g_conf, small

    def backward(self, prefill=None, params=None):
        """-> dict of the four gradients (device), g_conf, sums.  params: the four tensors to differentiate at (default: the case's)."""
        P = self.P
        pa = params if params is not None else [getattr(self, k) for k in PR.INPUT_NAMES]
        grads = [torch.full_like(t, float("nan")) for t in pa]
        g_conf, small = self._conf_and_small(prefill)
        self.L.check(self.lib.das3r_pretransform_backward(P, *(_p(t) for t in pa), _p(self.conf), _p(self.idx), self.R, self.Lq, _p(self.g_means), _p(self.g_rot),
                                                          _p(self.g_scales), _p(self.g_opac), *(_p(t) for t in grads), _p(g_conf), _p(small), None),
                     "das3r_pretransform_backward")
        torch.cuda.synchronize()
        return dict(zip(GRAD_NAMES, grads), g_conf=g_conf, sums=small)

    def pose_sums(self, prefill=None):
        _, small = self._conf_and_small(prefill)
        self.L.check(self.lib.das3r_pretransform_pose_sums(self.P, _p(self.xyz), _p(self.rot), self.R, self.Lq, _p(self.g_means), _p(self.g_rot), _p(small), None),
                     "das3r_pretransform_pose_sums")
        torch.cuda.synchronize()
        return small

    def backward_adam(self, opt, params, prefill=None):
        g_conf, small = self._conf_and_small(prefill)
        slots, keep = opt.adam_slots(params)
        self.L.check(self.lib.das3r_pretransform_backward_adam(self.P, _p(self.conf), _p(self.idx), self.R, self.Lq, _p(self.g_means), _p(self.g_rot), _p(self.g_scales),
                                                               _p(self.g_opac), _p(g_conf), _p(small), slots, C.c_float(BETA1), C.c_float(BETA2), C.c_float(EPS), None),
                     "das3r_pretransform_backward_adam")
        opt.step()   # (nothing carries a gradient: counts the step of all four)
        torch.cuda.synchronize()
        del keep
        return dict(g_conf=g_conf, sums=small)


def _adam(params):
    from das3r_amd.fused import FusedAdam
    return FusedAdam([dict(params=[t], lr=lr) for t, lr in zip(params, LRS)], lr=0.0, betas=(BETA1, BETA2), eps=EPS)


def _fwd_ref(dev):
    d = dev.d
    return PR.forward64(*[d[k] for k in PR.INPUT_NAMES], d["conf"], dev.idx_host, *dev.host_mats())


def _bwd_ref(dev, depth=None):
    d = dev.d
    R, _, Lq = dev.host_mats()
    return PR.backward64(*[d[k] for k in PR.INPUT_NAMES], d["conf"], dev.idx_host, R, Lq, *[d[k] for k in PR.UPSTREAM_NAMES], depth=depth)


def _exact_mats(dev):
    R, t, Lq = dev.host_mats()
    assert torch.equal(R.reshape(3, 3), torch.tensor(PR.EXACT_R)) and torch.equal(t, dev.d["t"]) and bool((Lq.abs() == 0.5).all())


def _check_conf_exact(got, ref_values, dev, what):
    want, written = PR.place_conf(ref_values, dev.idx_host, dev.conf.numel(), SENTINEL)
    got = got.cpu().double()
    assert torch.equal(got[written], want[written]), f"{what}: g_conf at the mask positions"
    assert torch.equal(got[~written], want[~written]), f"{what}: g_conf outside the mask positions keeps its prefill"


# ---------------------------------------------------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("masked", [True, False], ids=["mask-index", "no-mask"])
@pytest.mark.parametrize("P", [1, 255, 257, 1048576, 1048577])
def test_exact_forward_equals_the_reference(P, masked):
    dev = Dev(PR.exact(P), masked)
    _exact_mats(dev)
    got, (ref, _, _) = dev.forward(), _fwd_ref(dev)
    for k in PER_GAUSSIAN:
        assert torch.equal(got[k].double(), ref[k]), (k, P)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 65536, 65537, 262144, 262145, 524293])
def test_exact_backward_and_pose_sums_equal_the_reference(P):
    """das3r_pretransform_backward and das3r_pretransform_pose_sums: per-Gaussian gradients, g_conf (the sentinel untouched off the mask), the
    28 sums = the int64 sums, into a zero g_small and on top of small integers; with and without the mask index."""
    e = PR.exact(P)
    want = PR.exact_sums(e).double()
    for masked in (True, False):
        dev = Dev(e, masked)
        _exact_mats(dev)
        ref = _bwd_ref(dev)[0]
        assert torch.equal(ref["sums"], want)
        for prefill in (None, e["prefill"]):
            total = want if prefill is None else want + prefill.double()
            got = dev.backward(prefill)
            for k in GRAD_NAMES:
                assert torch.equal(got[k].cpu().double(), ref[k]), (k, P, masked)
            _check_conf_exact(got["g_conf"], ref["g_conf"], dev, f"backward P={P}")
            assert torch.equal(got["sums"].cpu().double(), total), ("backward sums", P, masked, (got["sums"].cpu().double() - total).tolist())
            sums = dev.pose_sums(prefill).cpu().double()
            assert torch.equal(sums, total), ("pose_sums", P, (sums - total).tolist())


@pytest.mark.parametrize("P", [257, 262145, 524288, 524289, 1048653])
def test_exact_backward_with_adam_inside_equals_the_reference_and_the_two_kernels(P):
    """das3r_pretransform_backward_adam: 1025 rows (the combine's second outer iteration), 2048 rows, a second and a third grid-stride round.
    The 28 sums and g_conf equal the exact reference; parameters and both moments after the step equal das3r_pretransform_backward +
    FusedAdam.step() on the same inputs."""
    e = PR.exact(P)
    dev = Dev(e)
    _exact_mats(dev)
    want = PR.exact_sums(e).double()
    ref_conf = _bwd_ref(dev)[0]["g_conf"]
    pa, pb = dev.params(), dev.params()
    oa, ob = _adam(pa), _adam(pb)
    two = dev.backward(None, params=pa)
    for t, k in zip(pa, GRAD_NAMES):
        t.grad = two[k]
    oa.step()
    oa.zero_grad(set_to_none=True)
    for prefill in (None, e["prefill"]):
        params = pb if prefill is None else dev.params()
        one = dev.backward_adam(ob if prefill is None else _adam(params), params, prefill)
        total = want if prefill is None else want + prefill.double()
        assert torch.equal(one["sums"].cpu().double(), total), ("sums", P, (one["sums"].cpu().double() - total).tolist())
        _check_conf_exact(one["g_conf"], ref_conf, dev, f"backward_adam P={P}")
    torch.cuda.synchronize()
    for k, ta, tb in zip(PR.INPUT_NAMES, pa, pb):
        assert torch.equal(ta, tb), (k, float((ta - tb).abs().max()))
        assert not torch.equal(ta, getattr(dev, k)), "the step moved the parameter"
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[ta][key], ob.state[tb][key]), (k, key)
        assert oa.state[ta]["step"] == ob.state[tb]["step"] == 1


def test_sums_are_bit_identical_from_call_to_call_at_the_largest_grids():
    """The fixed-order claim of pretransform_chain.h with 1024 rows (backward, pose sums: 524 293 Gaussians) and 2048 rows (the Adam form:
    1 048 653), on inputs whose sums DO depend on the order (general tier, plain)."""
    d = PR.general("plain", 524293)
    dev = Dev(d)
    a, b = dev.backward()["sums"], dev.backward()["sums"]
    assert torch.equal(a, b) and bool(a.abs().min() > 0)
    a, b = dev.pose_sums(), dev.pose_sums()
    assert torch.equal(a, b) and bool(a.abs().min() > 0)
    d = PR.general("plain", 1048653)
    dev = Dev(d)
    runs = []
    for _ in range(2):
        params = dev.params()
        runs.append(dev.backward_adam(_adam(params), params)["sums"])
    assert torch.equal(runs[0], runs[1]) and bool(runs[0].abs().min() > 0)


# ---------------------------------------------------------------------------------------------------------------- general tier
POSE_CASES = [("plain", 0), ("plain", 1), ("offunit", 0), ("offunit", 1)]


def _report(what, ratios):
    print(f"[{what}] worst ratio to the budget: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("kind,seed", POSE_CASES)
def test_pose_matrices_within_the_budget(kind, seed):
    L, lib = _lib()
    d = PR.general(kind, 264, seed)
    ref, _, tol = PR.matrices64(d["q"], d["t"])
    pose = torch.cat([d["q"], d["t"]]).cuda()
    q, t = d["q"].cuda(), d["t"].cuda()
    a, b = torch.full((28,), float("nan"), device="cuda"), torch.full((28,), float("nan"), device="cuda")
    L.check(lib.das3r_pose_matrices(_p(pose), _p(a), None), "das3r_pose_matrices")
    L.check(lib.das3r_pose_matrices_qt(_p(q), _p(t), _p(b), None), "das3r_pose_matrices_qt")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    m = a.cpu()
    r = {k: PR.assert_within(got, ref[k], tol[k], PR.K, f"matrices {kind}/{seed} {k}") for k, got in (("R", m[:9]), ("t", m[9:12]), ("Lq", m[12:]))}
    _report(f"pose matrices {kind}/{seed} |q| = {float(d['q'].double().norm()):.3f}", r)


@pytest.mark.parametrize("kind,seed", POSE_CASES)
def test_pose_chain_within_the_budget(kind, seed):
    """das3r_pose_chain, _qt and _qt_rearm on g28 = the reference's sums of the kind (as fp32 values): g_q, g_t within the budget, the three
    entries equal to each other; _qt and _qt_rearm leave g28 zero, _rearm zeroes the two extra rows — also when they are the rows it writes."""
    L, lib = _lib()
    d = PR.general(kind, 264, seed)
    m = PR.matrices64(d["q"], d["t"])[0]
    g28 = PR.backward64(d["xyz"], d["rot"], None, None, None, None, m["R"].float(), m["Lq"].float(), d["g_means"], d["g_rot"], None, None)[0]["sums"].float()
    ref, _, tol = PR.pose_chain64(d["q"], g28)
    pose, q = torch.cat([d["q"], d["t"]]).cuda(), d["q"].cuda()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g_a, out_a = g28.cuda(), torch.full((7,), float("nan"), device="cuda")
    L.check(lib.das3r_pose_chain(_p(pose), _p(g_a), _p(out_a), s), "das3r_pose_chain")
    g_b, Qb, Tb = g28.cuda(), torch.full((3, 4), 9.0, device="cuda"), torch.full((3, 3), 9.0, device="cuda")
    L.check(lib.das3r_pose_chain_qt(_p(q), _p(g_b), _p(Qb[1]), _p(Tb[1]), s), "das3r_pose_chain_qt")
    g_c, Qc, Tc = g28.cuda(), torch.full((3, 4), 9.0, device="cuda"), torch.full((3, 3), 9.0, device="cuda")
    L.check(lib.das3r_pose_chain_qt_rearm(_p(q), _p(g_c), _p(Qc[1]), _p(Tc[1]), _p(Qc[2]), _p(Tc[2]), s), "das3r_pose_chain_qt_rearm")
    g_e, Qe, Te = g28.cuda(), torch.full((3, 4), 9.0, device="cuda"), torch.full((3, 3), 9.0, device="cuda")
    L.check(lib.das3r_pose_chain_qt_rearm(_p(q), _p(g_e), _p(Qe[1]), _p(Te[1]), _p(Qe[1]), _p(Te[1]), s), "das3r_pose_chain_qt_rearm, same rows")
    torch.cuda.synchronize()
    assert torch.equal(g_a.cpu(), g28), "das3r_pose_chain reads g28"
    for g in (g_b, g_c, g_e):
        assert float(g.abs().max()) == 0.0, "g28 is zero at rest"
    assert float(Qc[2].abs().max()) == 0.0 and float(Tc[2].abs().max()) == 0.0 and float(Qc[0].min()) == 9.0 and float(Tc[0].min()) == 9.0
    assert float(Qb[0].min()) == float(Qb[2].min()) == float(Tb[0].min()) == float(Tb[2].min()) == 9.0
    assert float(Qe[0].min()) == float(Qe[2].min()) == float(Te[0].min()) == float(Te[2].min()) == 9.0
    for Qx, Tx in ((Qb, Tb), (Qc, Tc), (Qe, Te)):
        assert torch.equal(Qx[1], out_a[:4]) and torch.equal(Tx[1], out_a[4:])
    out = out_a.cpu()
    r = dict(g_q=PR.assert_within(out[:4], ref["g_q"], tol["g_q"], PR.K, f"pose chain {kind}/{seed} g_q"),
             g_t=PR.assert_within(out[4:], ref["g_t"], tol["g_t"], PR.K, f"pose chain {kind}/{seed} g_t"))
    _report(f"pose chain {kind}/{seed}", r)


GENERAL_CASES = [(k, P) for P in (264, 65537) for k in PR.KINDS] + [("positive", 262145), ("plain", 262145)]


@pytest.mark.parametrize("kind,P", GENERAL_CASES)
def test_general_forward_backward_pose_sums_and_adam_within_the_budgets(kind, P):
    """Forward, backward, pose sums and the Adam-inside form (sums and g_conf: its parameters are tests/test_gpu_adam_edges.py's) against
    float64.  offunit: |q| = 0.2 at P = 264, 3 at 65 537."""
    seed = 1 if (kind == "offunit" and P == 65537) else 0
    d = PR.general(kind, P, seed)
    dev = Dev(d)
    mref, _, mtol = PR.matrices64(d["q"], d["t"])
    R, t, Lq = dev.host_mats()
    what = f"{kind} P={P}"
    r = {k: PR.assert_within(got, mref[k], mtol[k], PR.K, f"{what} {k}") for k, got in (("R", R), ("t", t), ("Lq", Lq))}
    got, (ref, _, tol) = dev.forward(), _fwd_ref(dev)
    expf_err = float(((got["scales"].double() - ref["scales"]).abs() / (PR.U * ref["scales"])).max())
    print(f"[{what}] device expf: worst |expf(x) - exp(x)| / (u exp(x)) = {expf_err:.4f} over `scaling` (allowed {PR.EXPF_U:g})")
    for k in PER_GAUSSIAN:
        r[k] = PR.assert_within(got[k], ref[k], tol[k], PR.K, f"forward {what} {k}")
    got, (ref, mag, tol) = dev.backward(), _bwd_ref(dev, PR.sums_depth(P, PR.CAP_BACKWARD))
    for k in GRAD_NAMES:
        r[k] = PR.assert_within(got[k].cpu(), ref[k], tol[k], PR.K, f"backward {what} {k}")
    want, written = PR.place_conf(ref["g_conf"], dev.idx_host, dev.conf.numel(), SENTINEL)
    budget, _ = PR.place_conf(tol["g_conf"], dev.idx_host, dev.conf.numel(), 0.0)   # (0 off the mask: the sentinel, exactly)
    assert int(written.sum()) == P
    r["g_conf"] = PR.assert_within(got["g_conf"].cpu(), want, budget, PR.K, f"backward {what} g_conf")
    r["sums"] = PR.assert_within(got["sums"].cpu(), ref["sums"], tol["sums"], PR.K, f"backward {what} sums")
    r["sums (pose_sums)"] = PR.assert_within(dev.pose_sums().cpu(), ref["sums"], tol["sums"], PR.K, f"pose_sums {what} sums")
    params = dev.params()
    one = dev.backward_adam(_adam(params), params)
    tol_adam = PR.sums_depth(P, PR.CAP_ADAM) * PR.U * mag["sums"]   # (its grid is capped at 2048 workgroups, not 1024)
    r["sums (adam)"] = PR.assert_within(one["sums"].cpu(), ref["sums"], tol_adam, PR.K, f"backward_adam {what} sums")
    r["g_conf (adam)"] = PR.assert_within(one["g_conf"].cpu(), want, budget, PR.K, f"backward_adam {what} g_conf")
    _report(what, r)
