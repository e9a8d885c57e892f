"""The optimizer kernels (das3r_amd/csrc/adam.hip: das3r_adam_step, das3r_adam_step_gated; the step inside
das3r_pretransform_backward_adam, which shares adam_math.h) against the float64 reference and the derived budgets of
tests/adam_reference.py: the update itself (p = 0), both moments, every descriptor form at the edges of ADAM_CHUNK = 2048 and of its
256-lane sub-blocks, compacted tables, rejected descriptors, and everything that must stay untouched — columns above the active length,
skipped tensors, 64 floats of sentinel either side of every buffer.  The kernels are called through ctypes with hand-built AdamTensor
descriptors; FusedAdam only where it is the subject (the split at 16 tensors, a 300-step run).  The budgets come from the roundings of
adam_math.h (tests/test_adam_reference_host.py); the kernels' own ratios are recorded in profiles/adam_edges_tol_report.txt.

Betas: the fp32 values A.BETA1, A.BETA2 everywhere, FusedAdam and torch.optim.Adam included, so that every side computes with the same
numbers (FusedAdam hands the kernel fp32 betas and computes the bias corrections of the plain step from the betas it was given)."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import adam_reference as A

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FA51C3D   # a NaN: whatever is computed from it cannot pass for a result
INVALID_ARG = -1
ROWS = (1, 227, 228, 456)
FORM_KINDS = ("general", "p_zero", "all_zero")
LR, LR_TAIL, T = 1.6e-4, 1.25e-4 / 20, 7


def layout(rows, row_len, active_len, grad_row_len=0, grad_off=0, state_row_len=0, head_len=0, mirror_row_len=0, mirror_off=0):
    return SimpleNamespace(rows=rows, row_len=row_len, active_len=active_len, grad_row_len=grad_row_len, grad_off=grad_off, state_row_len=state_row_len,
                           head_len=head_len, mirror_row_len=mirror_row_len, mirror_off=mirror_off)


class Guarded:
    """A device buffer of `size` floats between two guard bands, all sentinel but the elements `idx`, which hold `values`."""

    def __init__(self, size, idx, values, offset=0):
        host = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.int32)
        self.idx = idx + GUARD
        if idx.numel():
            assert int(idx.min()) >= 0 and int(idx.max()) < size, "the active region lies inside the buffer"
            host.view(torch.float32)[self.idx] = values
        self.before, self.dev = host, host.cuda()
        self.ptr = self.dev.data_ptr() + 4 * (GUARD + offset)

    def after(self):
        return self.dev.cpu()

    def active(self, host):
        return host.view(torch.float32)[self.idx]

    def outside_unchanged(self, host):
        keep = torch.ones(host.numel(), dtype=torch.bool)
        keep[self.idx] = False
        return torch.equal(host[keep], self.before[keep])


class Case:
    """One das3r_adam_tensor: guarded buffers laid out as the descriptor says, the descriptor, and the float64 reference of its step."""

    def __init__(self, lay, kind, seed=0, lr=LR, lr_tail=LR_TAIL, t=T, gated=False, null_moments=False):
        from das3r_amd.fused import AdamTensor
        self.lay, self.kind, self.t, self.gated = lay, kind, t, gated
        n = lay.rows * lay.active_len
        x = A.inputs(kind, n, seed) if n else {k: torch.zeros(0) for k in "pmvg"}
        r, c = torch.arange(max(lay.rows, 0))[:, None], torch.arange(lay.active_len)[None, :]
        grl, srl = lay.grad_row_len or lay.row_len, lay.state_row_len or lay.row_len
        at = lambda stride, off=0: (r * stride + c + off).reshape(-1)
        body = max(lay.rows, 1)   # (a tensor with rows = 0 still has memory that must stay as it is)
        self.p = Guarded(body * lay.row_len, at(lay.row_len), x["p"])
        self.g = Guarded(body * grl + lay.grad_off, at(grl, lay.grad_off), x["g"], lay.grad_off)
        self.m = Guarded(body * srl, at(srl), x["m"])
        self.v = Guarded(body * srl, at(srl), x["v"])
        self.mirror = Guarded(body * lay.mirror_row_len + lay.mirror_off, at(lay.mirror_row_len, lay.mirror_off), torch.zeros(n), lay.mirror_off) if lay.mirror_row_len else None
        if self.mirror is not None:   # (all sentinel on the way in: the active elements are written, never read)
            self.mirror.before.fill_(SENTINEL)
            self.mirror.dev.fill_(SENTINEL)
        split = 0 < lay.head_len < lay.active_len
        self.is_head = (c < lay.head_len).expand(max(lay.rows, 0), lay.active_len).reshape(-1) if split else None
        if gated:
            self.step_size, self.tail, self.bc2_sqrt = A.f32(lr), A.f32(lr_tail), 1.0
            ref = A.gated64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, self.step_size, t, self.tail if split else None, self.is_head)
        else:
            (self.step_size, self.bc2_sqrt), self.tail = A.host_corrections(lr, t), A.host_corrections(lr_tail, t)[0]
            ref = A.step64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, self.step_size, self.bc2_sqrt, self.tail if split else None, self.is_head)
        self.ref, self.tol = ref
        e = AdamTensor()
        e.param, e.grad = self.p.ptr, self.g.ptr
        e.exp_avg, e.exp_avg_sq = (None, None) if null_moments else (self.m.ptr, self.v.ptr)
        e.rows, e.row_len, e.active_len = lay.rows, lay.row_len, lay.active_len
        e.step_size, e.bc2_sqrt, e.head_len, e.step_size_tail = self.step_size, self.bc2_sqrt, lay.head_len, self.tail
        e.grad_row_len, e.state_row_len = lay.grad_row_len, lay.state_row_len
        e.mirror, e.mirror_row_len = (self.mirror.ptr, lay.mirror_row_len) if self.mirror is not None else (None, 0)
        self.desc = e

    def buffers(self):
        return [b for b in (self.p, self.g, self.m, self.v, self.mirror) if b is not None]

    def results(self):
        return {name: b.after() for name, b in (("p", self.p), ("g", self.g), ("m", self.m), ("v", self.v), ("mirror", self.mirror)) if b is not None}

    def check_unchanged(self, label):
        for b in self.buffers():
            assert torch.equal(b.after(), b.before), f"{label}: a buffer of a tensor that must not be touched has changed"

    def check(self, form, label):
        """Guards and everything outside the active region bit-unchanged, the gradient whole; p, m, v within K x budget; the mirror = p."""
        out = self.results()
        assert torch.equal(out["g"], self.g.before), f"{label}: the gradient is read-only"
        for name in ("p", "m", "v"):
            assert getattr(self, name).outside_unchanged(out[name]), f"{label}: {name} changed outside the active region (guard bands included)"
        ratios = {}
        for name in ("p", "m", "v"):
            got = getattr(self, name).active(out[name])
            ratios[name] = A.assert_within(got, self.ref[name], self.tol[name], A.K, f"{form} {self.kind} {name} [{label}]") if got.numel() else 0.0
        if self.mirror is not None:
            assert self.mirror.outside_unchanged(out["mirror"]), f"{label}: the mirror keeps its sentinel outside the active columns"
            assert torch.equal(self.mirror.active(out["mirror"]).view(torch.int32), self.p.active(out["p"]).view(torch.int32)), f"{label}: mirror == stepped p"
        return out, ratios


def _lib():
    from das3r_amd import _lib
    return _lib, _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def step(cases):
    """One das3r_adam_step over the descriptors of `cases` -> the status."""
    from das3r_amd.fused import AdamTensor
    _, lib = _lib()
    arr = (AdamTensor * max(len(cases), 1))(*[c.desc for c in cases])
    rc = lib.das3r_adam_step(len(cases), arr, C.c_float(A.BETA1), C.c_float(A.BETA2), C.c_float(A.EPS), _stream())
    torch.cuda.synchronize()
    return rc


def step_gated(cases, gate, threshold, state):
    from das3r_amd.fused import AdamTensor
    _, lib = _lib()
    arr = (AdamTensor * max(len(cases), 1))(*[c.desc for c in cases])
    g = torch.tensor([gate], dtype=torch.float32, device="cuda")
    rc = lib.das3r_adam_step_gated(len(cases), arr, C.c_float(A.BETA1), C.c_float(A.BETA2), C.c_float(A.EPS), C.c_void_p(g.data_ptr()), C.c_float(threshold),
                                   C.c_void_p(state.ptr), _stream())
    torch.cuda.synchronize()
    return rc


def run_twice(form, lay, kind, label, **kw):
    """The case through das3r_adam_step from two fresh sets of buffers: checked, and bit-identical."""
    outs = []
    for _ in range(2):
        case = Case(lay, kind, **kw)
        assert step([case]) == 0, _lib()[0].last_error()
        outs.append(case.check(form, label)[0])
    for name in outs[0]:
        assert torch.equal(outs[0][name], outs[1][name]), f"{label}: {name}: two runs must be bit-identical"


# ---------------------------------------------------------------------------------------------------------------- one tensor per call
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 4097, 6144])
def test_flat_tensor_at_the_chunk_and_sub_block_edges(n):
    for kind in FORM_KINDS:
        run_twice("flat", layout(1, n, n), kind, f"n={n}")


@pytest.mark.parametrize("kind", [k for k in A.KINDS if k not in FORM_KINDS])
def test_flat_tensor_of_the_remaining_kinds(kind):
    """first, g_zero, large, tiny (gradients whose square underflows), decay (subnormal moments) at n = 2049."""
    run_twice("flat", layout(1, 2049, 2049), kind, "n=2049")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("compact_state", [False, True], ids=["state-full", "state-compact"])
@pytest.mark.parametrize("active_len", [9, 24, 45])
def test_row_prefix(active_len, compact_state, rows):
    """Rows of 45 floats of which the first 9, 24 or all step; 9 x 227 = 2043 and 9 x 228 = 2052, so a row straddles the chunk edge."""
    for kind in FORM_KINDS:
        run_twice("row-prefix", layout(rows, 45, active_len, state_row_len=active_len if compact_state else 0), kind,
                  f"rows={rows} active={active_len} {'compact' if compact_state else 'full'} state")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("strided", [False, True], ids=["grad-compact", "grad-strided"])
@pytest.mark.parametrize("active_len", [9, 24, 45])
def test_compact_or_strided_gradient(active_len, strided, rows):
    """The gradient with its own row stride: compact (grad_row_len = active_len), or a block of columns of a wider tensor (rows of 48
    floats, the pointer 3 floats in)."""
    lay = layout(rows, 45, active_len, grad_row_len=48, grad_off=3) if strided else layout(rows, 45, active_len, grad_row_len=active_len)
    for kind in FORM_KINDS:
        run_twice("gradient-stride", lay, kind, f"rows={rows} active={active_len} {'strided' if strided else 'compact'}")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("active_len", [3, 12, 48])
def test_split_rates(active_len, rows):
    """Rows of 48 floats, the first 3 with step_size and the others with step_size_tail (a twentieth of it); active_len = 3 has no tail:
    the head's rate throughout (the reference steps every element with step_size then)."""
    for kind in FORM_KINDS:
        run_twice("split-rates", layout(rows, 48, active_len, head_len=3), kind, f"rows={rows} active={active_len}")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("mirror_off", [0, 3])
@pytest.mark.parametrize("active_len", [9, 24, 45])
def test_mirror(active_len, mirror_off, rows):
    """The stepped values written a second time into rows of 48 floats at column offset 0 or 3: equal to p on the active columns, the
    sentinel everywhere else."""
    for kind in FORM_KINDS:
        run_twice("mirror", layout(rows, 45, active_len, mirror_row_len=48, mirror_off=mirror_off), kind, f"rows={rows} active={active_len} offset={mirror_off}")


# ---------------------------------------------------------------------------------------------------------------- tables
def _table():
    """16 descriptors that mix every form; inactive ones (rows = 0, active_len = 0) first, in the middle and last.  Every tensor has its own
    learning rate and step count, so that a table indexed by the wrong counter steps with a neighbour's step_size / bc2_sqrt."""
    lays = [("inactive", layout(0, 45, 45)), ("flat", layout(1, 2049, 2049)), ("row-prefix", layout(228, 45, 9)), ("inactive", layout(7, 45, 0)),
            ("gradient-stride", layout(227, 45, 24, grad_row_len=48, grad_off=3)), ("split-rates", layout(228, 48, 12, head_len=3)),
            ("inactive", layout(0, 1, 1)), ("inactive", layout(31, 48, 0, head_len=3)), ("mirror", layout(227, 45, 9, mirror_row_len=48, mirror_off=3)),
            ("flat", layout(1, 1, 1)), ("row-prefix", layout(456, 45, 24, state_row_len=24)), ("gradient-stride", layout(1, 45, 45, grad_row_len=45)),
            ("flat", layout(1, 255, 255)), ("split-rates", layout(1, 48, 48, head_len=3)), ("mirror", layout(228, 45, 45, mirror_row_len=48)),
            ("inactive", layout(0, 9, 9))]
    kinds = ("p_zero", "general", "all_zero")
    return [(form, Case(lay, kinds[i % 3], seed=i, lr=LR * (1 + i), lr_tail=LR_TAIL * (1 + i), t=1 + 3 * i)) for i, (form, lay) in enumerate(lays)]


def test_table_of_sixteen_with_inactive_tensors():
    outs = []
    for _ in range(2):
        table = _table()
        assert len(table) == 16
        assert step([c for _, c in table]) == 0, _lib()[0].last_error()
        out = []
        for i, (form, c) in enumerate(table):
            if form == "inactive":
                c.check_unchanged(f"table entry {i}")
            else:
                out.append(c.check("table " + form, f"entry {i}")[0])
        outs.append(out)
    for a, b in zip(*outs):
        assert all(torch.equal(a[name], b[name]) for name in a), "two runs must be bit-identical"


def test_empty_and_oversized_tables():
    from das3r_amd.fused import AdamTensor
    _, lib = _lib()
    assert lib.das3r_adam_step(0, None, C.c_float(A.BETA1), C.c_float(A.BETA2), C.c_float(A.EPS), _stream()) == 0
    assert step([]) == 0
    cases = [Case(layout(1, 5 + i, 5 + i), "general", seed=i) for i in range(17)]
    assert step(cases) == INVALID_ARG and "16" in _lib()[0].last_error()
    for i, c in enumerate(cases):
        c.check_unchanged(f"17 tensors, entry {i}")
    state = Guarded(2, torch.arange(2), torch.zeros(2))
    assert step_gated(cases, 1.0, 0.0, state) == INVALID_ARG
    assert torch.equal(state.after(), state.before)
    assert isinstance(AdamTensor(), C.Structure)


REJECTED = {
    "negative rows": dict(lay=layout(-1, 45, 9)),
    "active_len > row_len": dict(lay=layout(4, 45, 46)),
    "active_len > grad_row_len": dict(lay=layout(4, 45, 24, grad_row_len=9)),
    "active_len > state_row_len": dict(lay=layout(4, 45, 24, state_row_len=9)),
    "null moments with active elements": dict(lay=layout(4, 45, 9), null_moments=True),
    "mirror_row_len < active_len": dict(lay=layout(4, 45, 24, mirror_row_len=48)),
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_rejected_descriptor_names_its_index_and_touches_nothing(what):
    """The bad descriptor sits at index 2 behind an inactive and a good one: DAS3R_ERR_INVALID_ARG, das3r_last_error() names tensor 2, and
    no buffer of any tensor changes — the good ones neither (nothing is launched).  The bad tensor's buffers are sized for the descriptor
    it would have been with its fields in range."""
    spec = REJECTED[what]
    bad_lay = spec["lay"]
    sized = layout(max(bad_lay.rows, 1), 48, min(bad_lay.active_len, 45), 48, 0, 48, 0, 48 if bad_lay.mirror_row_len else 0)
    bad = Case(sized, "general", seed=5)
    d = bad.desc
    d.rows, d.row_len, d.active_len, d.grad_row_len, d.state_row_len = bad_lay.rows, bad_lay.row_len, bad_lay.active_len, bad_lay.grad_row_len, bad_lay.state_row_len
    if bad_lay.mirror_row_len:
        d.mirror_row_len = bad_lay.active_len - 1
    if spec.get("null_moments"):
        d.exp_avg, d.exp_avg_sq = None, None
    cases = [Case(layout(0, 45, 45), "general", seed=1), Case(layout(228, 45, 9), "general", seed=2), bad, Case(layout(1, 2049, 2049), "p_zero", seed=3)]
    state = Guarded(2, torch.arange(2), torch.zeros(2))
    for rc in (step(cases), step_gated(cases, 1.0, 0.0, state)):
        assert rc == INVALID_ARG
        assert "tensor 2" in _lib()[0].last_error(), _lib()[0].last_error()
    for i, c in enumerate(cases):
        c.check_unchanged(f"{what}: entry {i}")
    assert torch.equal(state.after(), state.before)


# ---------------------------------------------------------------------------------------------------------------- gated step
def _state(t_before):
    s = Guarded(2, torch.arange(2), torch.zeros(2))
    s.before[GUARD], s.before[GUARD + 1] = t_before, 0
    s.dev.copy_(s.before)
    return s


@pytest.mark.parametrize("n", [2049, 3 * 2049])
@pytest.mark.parametrize("t", [1, 2, 3, 5, 10, 300, 4000])
def test_gated_step_takes_step_t(t, n):
    """state[0] preloaded with t - 1, the gate open: the step is number t with bias corrections computed on the device — within K x the
    gated budget (8 u more than the plain one on the update: 4 u for each 1 - beta^t), state = [t, 0] afterwards, two runs bit-identical."""
    for kind in ("p_zero", "general"):
        outs = []
        for _ in range(2):
            case, state = Case(layout(1, n, n), kind, lr=3e-5, t=t, gated=True), _state(t - 1)
            assert step_gated([case], 26.5, 26.0, state) == 0, _lib()[0].last_error()
            outs.append(case.check("gated", f"t={t} n={n}")[0])
            after = state.after()
            assert after[GUARD:GUARD + 2].tolist() == [t, 0] and state.outside_unchanged(after)
        assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])


@pytest.mark.parametrize("gate", [26.0, 25.0, float("-inf"), float("nan")], ids=["equal", "below", "-inf", "nan"])
def test_gated_step_with_a_closed_gate_moves_nothing(gate):
    """Strictly greater opens the gate: at the threshold, below it or with a NaN nothing moves and the count stays."""
    cases = [Case(layout(1, 2049, 2049), "general", gated=True, t=4), Case(layout(228, 48, 12, head_len=3), "p_zero", gated=True, t=4)]
    state = _state(3)
    assert step_gated(cases, gate, 26.0, state) == 0
    for i, c in enumerate(cases):
        c.check_unchanged(f"closed gate, entry {i}")
    assert torch.equal(state.after(), state.before)


def test_gated_step_of_a_split_rate_table():
    """The gated kernel divides BOTH learning rates by its bias correction: a split-rate tensor and a row prefix beside a flat one, step 3."""
    cases = [("gated split-rates", Case(layout(228, 48, 12, head_len=3), "p_zero", gated=True, t=3, lr=2.5e-3, lr_tail=1.25e-4)),
             ("gated row-prefix", Case(layout(227, 45, 9, state_row_len=9), "general", gated=True, t=3, lr=1e-3)),
             ("gated", Case(layout(1, 257, 257), "all_zero", gated=True, t=3, lr=3e-5))]
    state = _state(2)
    assert step_gated([c for _, c in cases], 1.0, 0.0, state) == 0
    for i, (form, c) in enumerate(cases):
        c.check(form, f"entry {i}")
    assert state.after()[GUARD:GUARD + 2].tolist() == [3, 0]


# ---------------------------------------------------------------------------------------------------------------- FusedAdam
SEVENTEEN = (5, 300, 17, 64, 255, 6, 128, 33, 299, 7, 256, 100, 9, 211, 65, 31, 150)


def _seventeen_groups():
    from das3r_amd.fused import FusedAdam
    xs = [A.inputs("general" if i % 2 else "p_zero", n, seed=20 + i) for i, n in enumerate(SEVENTEEN)]
    params = [x["p"].cuda() for x in xs]
    lrs = [1e-4 * (1 + i) for i in range(17)]
    opt = FusedAdam([dict(params=[p], lr=lr, name=f"g{i}") for i, (p, lr) in enumerate(zip(params, lrs))], lr=0.0, betas=(A.BETA1, A.BETA2), eps=1e-15)
    for i, (p, x) in enumerate(zip(params, xs)):
        opt.state[p] = dict(step=i, exp_avg=x["m"].cuda(), exp_avg_sq=x["v"].cuda())   # (tensor i is about to take its step i + 1)
        p.grad = x["g"].cuda()
    return opt, params, xs, lrs


def test_fused_adam_splits_seventeen_tensors_into_two_launches():
    opt, params, xs, lrs = _seventeen_groups()
    opt.step()
    torch.cuda.synchronize()
    for i, (p, x, lr) in enumerate(zip(params, xs, lrs)):
        ref, tol = A.step64(x["p"], x["m"], x["v"], x["g"], A.BETA1, A.BETA2, A.EPS, *A.host_corrections(lr, i + 1))
        st = opt.state[p]
        assert st["step"] == i + 1
        for name, got in (("p", p), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            A.assert_within(got.cpu(), ref[name], tol[name], A.K, f"FusedAdam-17 {name} [group {i}, {SEVENTEEN[i]} elements]")


def test_fused_adam_with_a_gate_refuses_seventeen_tensors_before_anything_moves():
    opt, params, xs, _ = _seventeen_groups()
    with pytest.raises(RuntimeError, match="at most 16"):
        opt.step(gate=torch.tensor(30.0, device="cuda"), threshold=26.0)
    torch.cuda.synchronize()
    for i, (p, x) in enumerate(zip(params, xs)):
        st = opt.state[p]
        assert torch.equal(p.cpu(), x["p"]) and torch.equal(st["exp_avg"].cpu(), x["m"]) and torch.equal(st["exp_avg_sq"].cpu(), x["v"]), i
        assert st["step"] == i, "no step was counted"
    assert opt._gate_state is None or opt._gate_state.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- 300 steps
LONG_STEPS = 300


@functools.lru_cache(maxsize=None)
def _long_run_problem():
    gen = torch.Generator().manual_seed(4099)
    shapes = dict(flat=(4099,), sh=(91, 15, 3))
    init = {k: torch.randn(s, generator=gen) for k, s in shapes.items()}
    target = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    noise = [{k: 0.3 * torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()} for _ in range(LONG_STEPS)]
    gates = [26.0 + float(x) for x in (torch.rand(LONG_STEPS, generator=gen) - 0.4)]   # open (> 26) on about 60 % of the steps
    return init, target, noise, gates


def _long_run(make_opt, dtype, device, gated, fused):
    """-> {tensor: (p, exp_avg, exp_avg_sq)} as float64 CPU tensors after LONG_STEPS iterations.  The gradient of every iteration is
    g = (p - p*) + noise_t from THIS run's p, in float64 on the host, rounded to fp32; zero above the active SH degree."""
    init, target, noise, gates = _long_run_problem()
    ps = {k: torch.nn.Parameter(v.clone().to(dtype).to(device)) for k, v in init.items()}   # (clone: .to() of an fp32 CPU tensor is the tensor itself)
    opt = make_opt(ps)
    degree = 0
    for it in range(LONG_STEPS):
        if it in (100, 200):
            degree += 1
        if fused:
            opt.set_active_sh_degree(degree)
        if it == 150:
            for g in opt.param_groups:
                g["lr"] = g["lr"] * 0.3
        active = (degree + 1) ** 2 - 1
        for k, p in ps.items():
            g = (p.detach().double().cpu() - target[k]) + noise[it][k]
            if k == "sh":
                g[:, active:, :] = 0.0
            p.grad = g.float().to(dtype).to(device)
        if not gated:
            opt.step()
        elif fused:
            opt.step(gate=torch.tensor(gates[it], device=device), threshold=26.0)
        elif gates[it] > 26.0:
            opt.step()
    out = {}
    for k, p in ps.items():
        st = opt.state[p]
        m, v = (opt._full_moment(st[key], p) for key in ("exp_avg", "exp_avg_sq")) if fused else (st["exp_avg"], st["exp_avg_sq"])
        out[k] = tuple(t.detach().double().cpu() for t in (p, m, v))
    return out, opt


@pytest.mark.parametrize("gated", [False, True], ids=["every-step", "gated"])
def test_three_hundred_steps_stay_as_close_to_float64_as_fp32_torch(gated):
    """FusedAdam against torch.optim.Adam in float64 on the CPU over 300 steps of a run that feeds back on itself (the SH degree goes up at
    steps 100 and 200, lr changes at 150; with a gate: open on about 60 % of the steps, torch stepped on those only).  The bar on
    max|x - x64| for the parameter and both moments of each tensor is 4 x the deviation of torch.optim.Adam in fp32 on the CPU from the
    same float64 run (4: another rounding order over 300 steps); a bias correction or count that is off by one is far outside."""
    from das3r_amd.fused import FusedAdam
    from tests.util import _report
    groups = lambda ps, extra: [dict(params=[ps["flat"]], lr=1e-3, name="flat"), dict(params=[ps["sh"]], lr=2.5e-3, name="f_rest", **extra)]
    torch_opt = lambda ps: torch.optim.Adam(groups(ps, {}), lr=0.0, betas=(A.BETA1, A.BETA2), eps=1e-15, foreach=False)
    ref, _ = _long_run(torch_opt, torch.float64, "cpu", gated, False)
    f32, _ = _long_run(torch_opt, torch.float32, "cpu", gated, False)
    got, opt = _long_run(lambda ps: FusedAdam(groups(ps, dict(sh_rest=True)), lr=0.0, betas=(A.BETA1, A.BETA2), eps=1e-15), torch.float32, "cuda", gated, True)
    _, _, _, gates = _long_run_problem()
    opened = sum(g > 26.0 for g in gates)
    assert 0.5 * LONG_STEPS < opened < 0.7 * LONG_STEPS
    if gated:
        assert opt._gate_state.tolist() == [opened, 0]
    init = _long_run_problem()[0]
    assert torch.equal(got["sh"][0][:, 8:, :], init["sh"][:, 8:, :].double()), "coefficients above degree 2 are never touched"
    assert not bool(got["sh"][1][:, 8:, :].any()) and not bool(got["sh"][2][:, 8:, :].any())
    failures = []
    for k in ("flat", "sh"):
        for name, x, x32, x64 in zip(("p", "exp_avg", "exp_avg_sq"), got[k], f32[k], ref[k]):
            dev32, dev = float((x32 - x64).abs().max()), float((x - x64).abs().max())
            print(f"[{'gated' if gated else 'plain'} {k} {name}] fp32 torch deviates {dev32:.3e}, FusedAdam {dev:.3e} ({dev / dev32:.2f} x), max|x| {float(x64.abs().max()):.3e}; "
                  f"FusedAdam from fp32 torch {float((x - x32).abs().max()):.3e}, {int((x != x32).sum())} of {x.numel()} elements differ")
            _report("budget_ratio", f"long-run {'gated ' if gated else ''}{name} [{k}: fp32 torch {dev32:.3e}, FusedAdam {dev:.3e}]", dev / dev32, 4.0)
            assert dev32 > 0
            if dev > 4.0 * dev32:
                failures.append((k, name, dev, dev32))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- the step inside the pre-transform's backward
def test_pretransform_backward_adam_steps_within_the_budgets():
    """das3r_pretransform_backward_adam at P = 2049 (a ninth workgroup for a single Gaussian), kind p_zero: the four tensors start at 0,
    their moments are the kind's, the step is number 7.  The gradients the pass computes and never writes are those of
    das3r_pretransform_backward on the same inputs (tests/test_gpu_fused.py holds the two passes to the same bits); parameters and both
    moments of all four tensors within K x the step64 budget."""
    from das3r_amd.fused import FusedAdam
    from tests.test_gpu_fused import _inputs
    _l, lib = _lib()
    P = 2049
    a, mask = _inputs(P, frames=3, hw=(30, 30), seed=4)
    idx = torch.nonzero(mask).reshape(-1).contiguous()
    names, cols, lrs = ("xyz", "rot", "scaling", "opacity_raw"), (3, 4, 3, 1), (1.6e-4, 1e-3, 5e-3, 0.05)
    conf = a["conf"].detach().reshape(-1).contiguous()
    xs = [A.inputs("p_zero", P * c, seed=40 + k) for k, c in enumerate(cols)]
    params = [x["p"].reshape(P, c).cuda() for x, c in zip(xs, cols)]
    assert not any(bool(p.any()) for p in params)
    opt = FusedAdam([dict(params=[p], lr=lr) for p, lr in zip(params, lrs)], lr=0.0, betas=(A.BETA1, A.BETA2), eps=1e-15)
    for p, x, c in zip(params, xs, cols):
        opt.state[p] = dict(step=T - 1, exp_avg=x["m"].reshape(P, c).cuda(), exp_avg_sq=x["v"].reshape(P, c).cuda())
    mats = torch.empty(28, device="cuda")
    _l.check(lib.das3r_pose_matrices(C.c_void_p(a["pose"].detach().data_ptr()), C.c_void_p(mats.data_ptr()), None), "das3r_pose_matrices")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    R, Lq = C.c_void_p(mats.data_ptr()), C.c_void_p(mats.data_ptr() + 48)
    gen = torch.Generator().manual_seed(9)
    ups = [torch.randn(P, c, generator=gen).cuda() for c in cols]
    grads = [torch.empty_like(p) for p in params]
    gconf_a, gconf_b, small_a, small_b = torch.zeros_like(conf), torch.zeros_like(conf), torch.zeros(28, device="cuda"), torch.zeros(28, device="cuda")
    _l.check(lib.das3r_pretransform_backward(P, *(ptr(t) for t in params), ptr(conf), ptr(idx), R, Lq, *(ptr(t) for t in ups), *(ptr(t) for t in grads),
                                             ptr(gconf_a), ptr(small_a), None), "das3r_pretransform_backward")
    torch.cuda.synchronize()
    assert all(bool(g.any()) for g in grads)
    slots, keep = opt.adam_slots(params)
    _l.check(lib.das3r_pretransform_backward_adam(P, ptr(conf), ptr(idx), R, Lq, *(ptr(t) for t in ups), ptr(gconf_b), ptr(small_b), slots,
                                                  C.c_float(A.BETA1), C.c_float(A.BETA2), C.c_float(A.EPS), None), "das3r_pretransform_backward_adam")
    torch.cuda.synchronize()
    assert torch.equal(gconf_a, gconf_b)
    for name, p, x, g, lr in zip(names, params, xs, grads, lrs):
        ref, tol = A.step64(x["p"], x["m"], x["v"], g.reshape(-1).cpu(), A.BETA1, A.BETA2, A.EPS, *A.host_corrections(lr, T))
        st = opt.state[p]
        assert st["step"] == T
        for out, got in (("p", p), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            A.assert_within(got.reshape(-1).cpu(), ref[out], tol[out], A.K, f"pretransform-adam p_zero {out} [{name} P={P}]")
