"""The fused loss kernels (das3r_amd/csrc/photometric.hip: masked L1 + SSIM forward / backward, the ssim_map pair, the exposure
instantiations) against the float64 reference and the conditioning-aware budgets of tests/loss_reference.py, on the images the workload
is made of — masked regions, flat and saturated regions, a render that equals its target, black — at extents around the kernel's
constants (tile 16, window radius 5, halo tile 26), plus (208, 512) whose 416 tiles take finish_sums round its strided loop.  The budgets
and their multipliers K come from fp32 torch ops on the CPU (tests/test_loss_reference_host.py); the kernels' own ratios are recorded in
profiles/loss_edges_tol_report.txt.  Last: das3r_depth_l1 at the pixel counts where its float4 and scalar paths part."""
import ctypes as C
import math

import pytest
import torch

from tests import loss_reference as R
from tests.test_gpu_depth_train import _random_maps, _run_kernel

pytestmark = pytest.mark.gpu

LAM, GRAD = 0.2, 3.0
SHAPES = [(1, 1), (1, 40), (11, 1), (5, 7), (10, 27), (15, 31), (16, 16), (17, 33), (21, 26), (32, 48), (37, 53)]
LARGE = [("masked", (208, 512)), ("equal", (208, 512))]
CASES = [(kind, hw) for hw in SHAPES for kind in R.KINDS] + LARGE
PLAIN_CASES = [c + (LAM,) for c in CASES] + [(kind, (17, 33), lam) for lam in (0.0, 1.0) for kind in R.KINDS]
EXPOSURE_B_CASES = [(kind, hw) for hw in SHAPES for kind in ("masked", "ties", "flat_bright", "step")]
ABI_CASES = [(kind, hw) for hw in ((5, 7), (17, 33), (21, 26)) for kind in ("masked", "equal")]
ids = lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}" + (f"-lambda{c[2]:g}" if len(c) > 2 else "")


def _photometric(inputs, lam, exposure=None):
    from das3r_amd.fused import masked_photometric_loss
    render, gt, static = (t.cuda() for t in inputs)
    r, s = render.requires_grad_(True), static.requires_grad_(True)
    e = None if exposure is None else exposure.cuda().requires_grad_(True)
    loss, mse = masked_photometric_loss(r, gt, s, lam, exposure=e)
    (GRAD * loss).backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach().cpu(), mse=mse.detach().cpu(), d_render=r.grad.cpu(), d_static=s.grad.cpu(), dE=None if e is None else e.grad.cpu())


def _check_photometric(form, got, ref, tol, inputs, label):
    assert tuple(got["d_render"].shape) == tuple(inputs[0].shape) and tuple(got["d_static"].shape) == tuple(inputs[2].shape)
    for name, K in R.PLAIN_OUTPUTS:
        if name != "map" and ref[name] is not None:
            R.assert_within(got[name], ref[name], tol[name], K, f"{form} {name} [{label}]")
    assert bool((got["d_render"][:, inputs[2] == 0] == 0).all()), "d render is an exact 0 behind static == 0"


# ---------------------------------------------------------------------------------------------------------------- plain form
@pytest.mark.parametrize("case", PLAIN_CASES, ids=ids)
def test_masked_photometric_loss_within_the_budgets(case):
    """Plain form, upstream gradient 3: loss, MSE, d render and d static within K x budget of float64; d render exactly 0 behind
    static == 0; two runs bit-identical.  lambda 0.2 at every kind x shape, 0 (L1 alone) and 1 (SSIM alone) at (17, 33)."""
    kind, (H, W), lam = case
    inputs, ref, tol = R.plain_case(kind, H, W, lam, GRAD)
    got, again = _photometric(inputs, lam), _photometric(inputs, lam)
    for name in ("loss", "mse", "d_render", "d_static"):
        assert torch.equal(got[name], again[name]), f"{name}: two runs must be bit-identical"
    _check_photometric("plain", got, ref, tol, inputs, f"{kind} {H}x{W} lambda {lam:g}")


# ---------------------------------------------------------------------------------------------------------------- ssim_map
def _ssim_map(img1, img2, upstream):
    from das3r_amd.fused import ssim_map
    a, b = img1.requires_grad_(True), img2.requires_grad_(True)
    m = ssim_map(a, b)
    (m * upstream).sum().backward()
    torch.cuda.synchronize()
    return dict(map=m.detach().cpu(), d_img1=a.grad.cpu(), d_img2=b.grad.cpu())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_ssim_map_within_the_budgets(case):
    """fused.ssim_map on the MASKED images (render * static, gt * static: what integrate.patch() hands it) with a random upstream gradient
    per pixel: the map and both image gradients within K x budget of float64."""
    kind, (H, W) = case
    inputs, ref, tol = R.map_case(kind, H, W)
    got = _ssim_map(*(t.cuda() for t in inputs))
    for name, K in R.MAP_OUTPUTS:
        assert tuple(got[name].shape) == (3, H, W)
        R.assert_within(got[name], ref[name], tol[name], K, f"ssim_map {name} [{kind} {H}x{W}]")


@pytest.mark.parametrize("kind", ["uniform", "masked"])
def test_ssim_map_takes_permuted_images(kind):
    """[H, W, 3] tensors permuted to [3, H, W] (an image as it is loaded), the upstream gradient too: the same bits as from contiguous
    copies, within the budgets, and gradients of the inputs' shape."""
    H, W = 17, 33
    inputs, ref, tol = R.map_case(kind, H, W)
    dense = _ssim_map(*(t.cuda() for t in inputs))
    hwc = [t.permute(1, 2, 0).contiguous().cuda().permute(2, 0, 1) for t in inputs]
    assert not any(t.is_contiguous() for t in hwc) and all(tuple(t.shape) == (3, H, W) for t in hwc)
    got = _ssim_map(*hwc)
    for name, K in R.MAP_OUTPUTS:
        assert tuple(got[name].shape) == (3, H, W) and torch.equal(got[name], dense[name]), name
        R.assert_within(got[name], ref[name], tol[name], K, f"ssim_map permuted {name} [{kind} {H}x{W}]")


# ---------------------------------------------------------------------------------------------------------------- exposure form
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_identity_exposure_gives_the_plain_forms_bits_on_every_kind(case):
    """E = [I | 0]: loss, MSE, d render and d static of the exposure kernels are the plain kernels' bit for bit — beyond uniform noise:
    on ties (the sign of an exact 0), behind static == 0, on flat images and on partial tiles; dL/dE comes out finite beside them."""
    kind, (H, W) = case
    inputs = R.make_inputs(kind, H, W)
    plain, expo = _photometric(inputs, LAM), _photometric(inputs, LAM, torch.eye(3, 4))
    for name in ("loss", "mse", "d_render", "d_static"):
        diff = int((plain[name] != expo[name]).sum())
        assert torch.equal(plain[name], expo[name]), f"{name}: {diff} of {plain[name].numel()} elements differ"
    assert tuple(expo["dE"].shape) == (3, 4) and bool(torch.isfinite(expo["dE"]).all())


@pytest.mark.parametrize("case", EXPOSURE_B_CASES, ids=ids)
def test_exposure_kernels_within_the_budgets(case):
    """E = a scaled channel permutation plus offsets, entries multiples of 2^-2: comp = apply_exposure(render, E) and comp * static are
    exact in fp32 (asserted), so the budgets apply unchanged to a = comp * static; d render_i carries sum_c |E[i][c]| t_a,c, each dL/dE
    the sum over the pixels of its terms' budgets."""
    from das3r_amd.losses import apply_exposure
    kind, (H, W) = case
    inputs, ref, tol = R.plain_case(kind, H, W, LAM, GRAD, R.EXPOSURE_B)
    E = torch.tensor(R.EXPOSURE_B)
    assert torch.equal(E * 4, (E * 4).round())
    comp32, comp64 = apply_exposure(inputs[0], E), apply_exposure(inputs[0].double(), E.double())
    assert torch.equal(comp32.double(), comp64) and torch.equal((comp32 * inputs[2]).double(), comp64 * inputs[2].double())
    got, again = _photometric(inputs, LAM, E), _photometric(inputs, LAM, E)
    for name in ("loss", "mse", "d_render", "d_static", "dE"):
        assert torch.equal(got[name], again[name]), f"{name}: two runs must be bit-identical"
    _check_photometric("exposure", got, ref, tol, inputs, f"{kind} {H}x{W}")


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("case", ABI_CASES, ids=ids)
def test_c_abi_writes_every_output_inside_the_image(case):
    """The pattern of test_photometric_backward_finish_is_the_two_launches on partial tiles, every output buffer pre-filled with NaN: the
    tile sums, the derivative maps, the SSIM map, d_render, d_static, d_img2 and out8 come back finite (no element inside the image is
    left unwritten, none is computed from the fill), out8 of das3r_photometric_backward_finish holds loss, MSE and PSNR within the
    budgets (the PSNR's from the MSE's through 20 log10), +inf for a render that equals its target as in das3r_amd.losses.psnr."""
    from das3r_amd import _lib
    lib = _lib.load()
    kind, (H, W) = case
    inputs, ref, tol = R.plain_case(kind, H, W, LAM, GRAD)
    render, gt, static = (t.cuda() for t in inputs)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    nb = int(lib.das3r_photometric_blocks(H, W))
    assert nb == math.ceil(H / 16) * math.ceil(W / 16)
    lam, grad = C.c_float(LAM), torch.full((1,), GRAD, device="cuda")
    partials, dmaps, out8, d_render, d_static = nan(nb, 8), nan(4, 3, H, W), nan(8), nan(3, H, W), nan(H, W)
    _lib.check(lib.das3r_photometric_forward(H, W, p(render), p(gt), p(static), lam, p(partials), p(dmaps), s), "forward")
    _lib.check(lib.das3r_photometric_backward_finish(H, W, p(render), p(gt), p(static), lam, p(dmaps), p(grad), p(d_render), p(d_static), p(partials),
                                                     p(out8), s), "backward_finish")
    a, b = render * static, gt * static
    up = R.make_upstream(H, W).cuda()
    partials2, dmaps2, ssim, d_img1, d_img2 = nan(nb, 8), nan(4, 3, H, W), nan(3, H, W), nan(3, H, W), nan(3, H, W)
    _lib.check(lib.das3r_ssim_map_forward(H, W, p(a), p(b), p(ssim), p(dmaps2), p(partials2), s), "ssim_map_forward")
    _lib.check(lib.das3r_ssim_map_backward(H, W, p(a), p(b), p(dmaps2), p(up), p(d_img1), p(d_img2), s), "ssim_map_backward")
    torch.cuda.synchronize()
    for name, t in (("partials", partials[:, :5]), ("dmaps", dmaps), ("d_render", d_render), ("d_static", d_static), ("partials (ssim_map)", partials2[:, :5]),
                    ("dmaps (ssim_map)", dmaps2), ("map", ssim), ("d_img1", d_img1), ("d_img2", d_img2), ("out8[:4], out8[5:]", torch.cat((out8[:4], out8[5:])))):
        assert bool(torch.isfinite(t).all()), f"{name}: {int((~torch.isfinite(t)).sum())} of {t.numel()} elements are not finite"
    label = f"{kind} {H}x{W}"
    o = out8.cpu()
    R.assert_within(o[0], ref["loss"], tol["loss"], R.K_LOSS, f"c-abi loss [{label}]")
    R.assert_within(o[1:4], ref["mse"], tol["mse"], R.K_LOSS, f"c-abi mse [{label}]")
    assert float(o[5:].abs().max()) == 0.0
    if kind == "equal":
        assert float(ref["mse"].max()) == 0.0 and math.isinf(float(ref["psnr"])) and float(o[4]) == float("inf")
    else:
        R.assert_within(o[4], ref["psnr"], R.psnr_budget(ref["mse"], tol["mse"]), R.K_LOSS, f"c-abi psnr [{label}]")
    R.assert_within(d_render, ref["d_render"], tol["d_render"], R.K_RENDER, f"c-abi d_render [{label}]")
    R.assert_within(d_static, ref["d_static"], tol["d_static"], R.K_STATIC, f"c-abi d_static [{label}]")
    mref, mtol = R.map_case(kind, H, W)[1:]
    for name, t, K in (("map", ssim, R.K_MAP), ("d_img1", d_img1, R.K_RENDER), ("d_img2", d_img2, R.K_RENDER)):
        R.assert_within(t, mref[name], mtol[name], K, f"c-abi ssim_map {name} [{label}]")


# ---------------------------------------------------------------------------------------------------------------- das3r_depth_l1 leftovers
def _depth_maps(H, W, seed):
    """_random_maps with, whatever the size, a live pixel (the last), a tie (the first, from two pixels on) and a masked-out pixel (the
    second, from three on)."""
    D, T, m, s = _random_maps(H, W, seed)
    flat = [t.view(-1) for t in (D, T, m, s)]
    n = H * W

    def put(k, d, t, mask, stat):
        for f, v in zip(flat, (d, t, mask, stat)):
            f[k] = v

    if n >= 2:
        put(0, 0.5, 0.5, 1.0, 0.5)
    if n >= 3:
        put(1, 0.75, 0.25, 0.0, 0.5)
    put(n - 1, 0.75, 0.25, 1.0, 0.5)
    return D, T, m, s


def _check_depth_l1(D, T, m, s, target_on_device=None):
    """The checks of tests/test_gpu_depth_train.py::test_depth_l1_kernel_against_the_formula.  -> (gradient, out8) of the first run."""
    from das3r_amd.losses import depth_l1
    H, W = D.shape
    ms = m if s is None else m * s
    off = ms == 0
    T_nan = T.clone()
    T_nan[off] = float("nan")
    weight, grad_loss = 0.37, 2.5
    ref = float(depth_l1(D.double(), T.double(), m.double(), None if s is None else s.double()))
    cu = lambda t: None if t is None else t.cuda().contiguous()
    target = cu(T_nan) if target_on_device is None else target_on_device(T_nan)
    before = torch.tensor([0.5, 1.0, 2.0, 3.0, 4.0, 9.0, 9.0, 7.0], device="cuda")
    d1, o1 = _run_kernel(cu(D), target, cu(m), cu(s), weight, grad_loss, before)
    d2, o2 = _run_kernel(cu(D), target, cu(m), cu(s), weight, grad_loss, before)
    assert torch.equal(d1, d2) and torch.equal(o1, o2), "two runs must be bit-identical"
    o = o1.cpu()
    assert ref > 0 and abs(float(o[5]) - ref) <= 1e-5 * ref, (float(o[5]), ref)
    assert abs(float(o[6]) - weight * float(o[5])) <= 1e-6 * abs(float(o[6]))
    assert float(o[0]) == float(before[0].cpu() + o[6]), "out8[0] after the call = its value before + out8[6] (one fp32 add)"
    assert torch.equal(o[1:5], before[1:5].cpu()) and float(o[7]) == 7.0
    e = (D - T) * ms
    closed = (torch.tensor(grad_loss * weight, dtype=torch.float32) * ms * torch.sign(e)) / float(H * W)
    got = d1.cpu()
    assert torch.isfinite(got).all(), "every pixel of the gradient is written"
    assert bool((got[off] == 0).all()), "exact zeros where m * s == 0"
    assert bool((got[(D == T) & ~off] == 0).all()), "d|x|/dx at 0 is 0"
    assert torch.allclose(got, closed, rtol=1e-6, atol=0.0)
    return d1, o1


@pytest.mark.parametrize("with_static", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 3), (3, 341), (1, 1025)])
def test_depth_l1_kernel_at_fewer_than_four_pixels_and_either_side_of_a_block(H, W, with_static):
    """One pixel and three (less than one thread's four), 1023 (one short of a workgroup's 1024) and 1025 (one past: a second workgroup
    for a single pixel); none a multiple of four, so all on the scalar path."""
    assert (H * W) % 4 != 0
    D, T, m, s = _depth_maps(H, W, 23 + W)
    _check_depth_l1(D, T, m, s if with_static else None)


def test_depth_l1_kernel_scalar_path_for_a_target_that_starts_four_bytes_into_its_storage():
    """H * W % 4 == 0 takes the float4 path — unless a pointer is not 16-byte aligned: `target` as a view one float into its storage takes
    the scalar path at such a size, and gives the float4 path's bits."""
    H, W = 4, 257   # 1028 pixels: two workgroups
    D, T, m, s = _depth_maps(H, W, 31)
    views = []

    def shifted(t):
        buf = torch.empty(H * W + 1, device="cuda")
        view = buf[1:].view(H, W)
        view.copy_(t)
        views.append(view)
        return view

    d_vec, o_vec = _check_depth_l1(D, T, m, s)
    d_sca, o_sca = _check_depth_l1(D, T, m, s, target_on_device=shifted)
    assert views[0].data_ptr() % 16 == 4 and views[0].is_contiguous()
    assert torch.equal(d_vec, d_sca) and torch.equal(o_vec, o_sca)
