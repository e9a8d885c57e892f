"""Float64 restatement of the fused loss kernels (das3r_amd/csrc/photometric.hip), the images they are tested on and the error
budgets they are held to.  Plain module, CPU tensors only: tests/test_loss_reference_host.py proves on the CPU that the budgets accept
fp32 torch ops and reject wrong formulas, tests/test_gpu_loss_edges.py holds the kernels to them.

Inputs.  make_inputs(kind, H, W, seed) -> render, gt [3, H, W], static [H, W], fp32.  Images are multiples of 2^-12, static of 2^-6, so
a = render * static and b = gt * static are exact in fp32: a tie in fp32 is a tie in float64, and the kernel's inputs to the window sums
are the reference's to the last bit.

Reference.  The loss of das3r_amd.losses (l1_loss, ssim, optionally apply_exposure) in float64.

Budgets.  u = 2^-24; W* the zero-padded 11 x 11 window; mu1, mu2, e1, e2, e12 the five window means; A, B, C, D as in the kernel;
m = A B / (C D).  An fp32 evaluation rounds every mean by ~u of the sum of its |terms|, and D = e1 - mu1^2 + e2 - mu2^2 + C2 cancels:
    kappa  = 1 + (e1 + e2 + mu1^2 + mu2^2) / D          (relative error of 1/D in units of u)
    beta   = 2 (|e12| + |mu1 mu2|)                      (absolute error of B in units of u)
    kappa2 = kappa (1 + beta / D)                       (relative error of a derivative of m)
    tol_m  = u (|A| / (C D) beta + |m| kappa)
The gradient budgets carry the derivatives' budgets through the backward's window sums:
    g   = |grad_loss| / (3 H W)
    t_a = g [(1 - lambda) + lambda (W*(kappa2 M1) + 2 |a| W*(kappa2 |dm/de1|) + |b| W*(kappa2 |dm/de12|))]           (t_b: 1 <-> 2, a <-> b)
    M1  = 2 |mu2| (|A| + |B|) / (C D) + 2 |m| |mu1| (1 / C + 1 / D) >= |dm/dmu1|        (the sum of its |terms|: see _map_budget)
    tol_render = u t_a |s|,    tol_static = u sum_c (t_a |r| + t_b |t|)
(ssim_map: the derivative maps weighted by |G| inside W*, no L1 term, no s, no g).  A budget is 0 where the result is an exact 0 (d render
behind static == 0), and assert_within then demands the exact 0."""
import functools
import math

import torch
import torch.nn.functional as F

from das3r_amd.losses import _gauss_window, apply_exposure, l1_loss, psnr, ssim

U = 2.0 ** -24
C1, C2 = 0.01 ** 2, 0.03 ** 2
KINDS = ("uniform", "flat_bright", "equal_flat", "equal", "black", "masked", "step", "ties")
MUTANTS = ("replicate", "sigma", "c2", "bias", "tie")

# The multipliers of the budgets: the smallest power of two >= 4 x the worst ratio |fp32 - float64| / budget that fp32 torch ops ON THE CPU
# (das3r_amd.losses in fp32: what the kernels replace) reach over every kind x shape of tests/test_loss_reference_host.py, both forms
# (`python -m tests.loss_reference` prints the table).  The 4 is for the kernel's other summation order (two 11-term FMA passes against
# one 121-term sum).  The kernels play no part in these numbers; theirs are in profiles/loss_edges_tol_report.txt.
# Measured worst fp32-torch ratios (kind, shape):
#   map 10.11 (black 37x53)     d render 3.49 (step 37x53)      d img1 2.61, d img2 2.82 (step 37x53)
#   d static 3.61 (step 1x40)   dE 1.81 (black 1x40)            loss 0.97 (black 17x33)      MSE 0.46 (masked 17x33)
# (Beyond the host test's shapes, for information: at 208x512 fp32 torch reaches 11.4 on the map of `masked`, 1.3 on its image gradients.)
K_MAP = 64.0       # 4 x 10.11 = 40.4
K_RENDER = 16.0    # 4 x  3.49 = 13.9    (d render, d img1, d img2)
K_STATIC = 16.0    # 4 x  3.61 = 14.4    (d static; dE, which is the same kind of sum: gradient x image over the pixels)
K_LOSS = 4.0       # 4 x  0.97 =  3.9    (loss, MSE, PSNR)

HOST_SHAPES = ((1, 1), (1, 40), (11, 1), (5, 7), (16, 16), (17, 33), (37, 53))
# one of part (b) of the exposure tests: a scaled channel permutation plus offsets, entries multiples of 2^-2
EXPOSURE_B = ((0.0, 0.0, 1.25, 0.25), (0.75, 0.0, 0.0, 0.0), (0.0, 0.5, 0.0, -0.25))


def _quant(x, bits):
    return torch.round(x * 2.0 ** bits) / 2.0 ** bits


def make_inputs(kind, H, W, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * KINDS.index(kind) + 131 * H + W)
    rnd = lambda *shape: torch.rand(*shape, generator=g)
    render, gt = _quant(rnd(3, H, W), 12), _quant(rnd(3, H, W), 12)
    static = _quant(0.2 + 0.8 * rnd(H, W), 6)
    extra, extra2 = rnd(3, H, W), rnd(3, H, W)
    if kind == "uniform":
        pass
    elif kind == "flat_bright":
        render, gt = _quant(0.98 + 0.002 * extra, 12), _quant(0.97 + 0.002 * extra2, 12)
    elif kind == "equal_flat":
        gt = _quant(0.9 + 0.001 * extra, 12)
        render = gt.clone()
    elif kind == "equal":
        render = gt.clone()
    elif kind == "black":
        render, gt = torch.zeros(3, H, W), torch.zeros(3, H, W)
    elif kind == "masked":   # the moving object: a centred block of exact zeros in a map of ones
        static = torch.ones(H, W)
        static[H // 4:H - H // 4, W // 4:W - W // 4] = 0.0
    elif kind == "step":     # 0/1 edges through the centre: vertical in the render, horizontal in the ground truth
        render = (torch.arange(W) >= W // 2).float()[None, None, :].expand(3, H, W).clone()
        gt = (torch.arange(H) >= H // 2).float()[None, :, None].expand(3, H, W).clone()
    elif kind == "ties":     # render == gt on a random half of the elements, the first one always
        tie = extra < 0.5
        tie[0, 0, 0] = True
        render = torch.where(tie, gt, render)
    else:
        raise KeyError(kind)
    for img in (render, gt):   # the products are exact in fp32
        assert torch.equal((img * static).double(), img.double() * static.double()), kind
    return render.contiguous(), gt.contiguous(), static.contiguous()


def make_upstream(H, W, seed=0):
    """dL/d(SSIM map) for the ssim_map tests: N(0, 1) quantised like the images."""
    g = torch.Generator().manual_seed(77 + 1000003 * seed + 131 * H + W)
    return _quant(torch.randn(3, H, W, generator=g), 12)


# ---------------------------------------------------------------------------------------------------------------- the formula, and its mutants
def _window(like, sigma=1.5):
    return _gauss_window(11, sigma, 3, like)


def _conv(x, w, pad="zeros"):
    if pad == "zeros":
        return F.conv2d(x[None], w, padding=5, groups=3)[0]
    return F.conv2d(F.pad(x[None], (5, 5, 5, 5), mode=pad), w, groups=3)[0]


def _m_of(mu1, mu2, e1, e2, e12, c2=C2):
    A, B = 2 * mu1 * mu2 + C1, 2 * (e12 - mu1 * mu2) + c2
    C, D = mu1 * mu1 + mu2 * mu2 + C1, (e1 - mu1 * mu1) + (e2 - mu2 * mu2) + c2
    return A, B, C, D, (A * B) / (C * D)


def ssim_restated(a, b, mutant=None):
    """das3r_amd.losses.ssim(a, b, size_average=False) written out (the host test holds the two together), with the mutations."""
    w = _window(a, 1.51 if mutant == "sigma" else 1.5)
    conv = lambda x: _conv(x, w, "replicate" if mutant == "replicate" else "zeros")
    m = _m_of(conv(a), conv(b), conv(a * a), conv(b * b), conv(a * b), C2 * 1.01 if mutant == "c2" else C2)[4]
    return m * (1.0 + 1e-4) if mutant == "bias" else m


def _abs(d, mutant):
    return torch.where(d >= 0, d, -d) if mutant == "tie" else d.abs()   # (where: d|x|/dx = +1 at x == 0)


def photometric(render, gt, static, lam, grad_loss=1.0, exposure=None, dtype=torch.float64, mutant=None):
    """-> dict(loss, mse [3], psnr, map, d_render, d_static, dE or None) of grad_loss * loss.  dtype float64, mutant None: the reference;
    float32: the torch ops the kernels replace; a mutant (float64): a wrong formula the budgets must reject."""
    r, s = render.to(dtype).clone().requires_grad_(True), static.to(dtype).clone().requires_grad_(True)
    E = None if exposure is None else torch.as_tensor(exposure).to(dtype).clone().requires_grad_(True)
    a = (r if E is None else apply_exposure(r, E)) * s
    b = gt.to(dtype) * s
    m = ssim(a, b, size_average=False) if mutant is None else ssim_restated(a, b, mutant)
    l1 = l1_loss(a, b, reduce=False) if mutant is None else _abs(a - b, mutant)
    loss = ((1.0 - lam) * l1 + lam * (1.0 - m)).mean()
    (grad_loss * loss).backward()
    d = lambda t: None if t is None else t.detach().double()
    return dict(loss=d(loss), mse=d(((a - b) ** 2).reshape(3, -1).mean(1)), psnr=d(psnr(a, b).mean()), map=d(m),
                d_render=d(r.grad), d_static=d(s.grad), dE=None if E is None else d(E.grad))


def ssim_map(img1, img2, upstream, dtype=torch.float64, mutant=None):
    """-> dict(map, d_img1, d_img2) of sum(upstream * SSIM map)."""
    a, b = img1.to(dtype).clone().requires_grad_(True), img2.to(dtype).clone().requires_grad_(True)
    m = ssim(a, b, size_average=False) if mutant is None else ssim_restated(a, b, mutant)
    (m * upstream.to(dtype)).sum().backward()
    return dict(map=m.detach().double(), d_img1=a.grad.double(), d_img2=b.grad.double())


# ---------------------------------------------------------------------------------------------------------------- budgets
def _map_budget(a, b):
    """a, b float64 -> tol_m, kappa2, |dm/d(mu1, mu2, e1, e2, e12)|, W*"""
    w = _window(a)
    conv = lambda x: _conv(x, w)
    means = [x.detach().requires_grad_(True) for x in (conv(a), conv(b), conv(a * a), conv(b * b), conv(a * b))]
    A, B, C, D, m = _m_of(*means)
    dm = [x.abs() for x in torch.autograd.grad(m.sum(), means)]
    mu1, mu2, e1, e2, e12 = (x.detach() for x in means)
    A, B, C, D, m = A.detach(), B.detach(), C.detach(), D.detach(), m.detach()
    # dm/dmu1 = 2 mu2 (B - A) / (C D) - 2 m mu1 (1 / C - 1 / D) is a difference, and between equal images an exact 0: a budget relative to
    # it is 0 where no fp32 evaluation is exact (fp32 torch ops miss such a budget by 1e14 x at a pixel with a = b = 0).  The two mu legs
    # carry the sum of the |terms| instead, which is never below |dm/dmu|; the e legs are single products and keep |dm/de|.
    for k, (mu, nu) in enumerate(((mu1, mu2), (mu2, mu1))):
        terms = 2.0 * nu.abs() * (A.abs() + B.abs()) / (C * D) + 2.0 * m.abs() * mu.abs() * (1.0 / C + 1.0 / D)
        assert bool((terms >= dm[k] * (1.0 - 1e-9)).all())
        dm[k] = terms
    kappa = 1.0 + (e1 + e2 + mu1 * mu1 + mu2 * mu2) / D
    beta = 2.0 * (e12.abs() + (mu1 * mu2).abs())
    return U * (A.abs() / (C * D) * beta + m.abs() * kappa), kappa * (1.0 + beta / D), dm, conv


def _grad_budget(a, b, kappa2, dm, conv, weight=None):
    """(t_a, t_b) without L1 term and scale: the derivatives' budgets through the backward's window sums."""
    k = kappa2 if weight is None else kappa2 * weight.abs()
    s_e12 = conv(k * dm[4])
    ta = conv(k * dm[0]) + 2.0 * a.abs() * conv(k * dm[2]) + b.abs() * s_e12
    tb = conv(k * dm[1]) + 2.0 * b.abs() * conv(k * dm[3]) + a.abs() * s_e12
    return ta, tb


def photometric_budgets(render, gt, static, lam, grad_loss=1.0, exposure=None):
    """-> dict(loss, mse, map, d_render, d_static, dE or None): the budgets (without K) of photometric()'s outputs."""
    r, t, s = render.double(), gt.double(), static.double()
    E = None if exposure is None else torch.as_tensor(exposure).double()
    comp = r if E is None else apply_exposure(r, E)
    a, b = comp * s, t * s
    tol_m, kappa2, dm, conv = _map_budget(a, b)
    m = ssim(a, b, size_average=False)
    g = abs(grad_loss) / (3.0 * a.shape[1] * a.shape[2])
    ta, tb = _grad_budget(a, b, kappa2, dm, conv)
    ta, tb = g * ((1.0 - lam) + lam * ta), g * ((1.0 - lam) + lam * tb)
    term = (1.0 - lam) * (a - b).abs() + lam * (1.0 - m)
    out = dict(loss=((1.0 - lam) * U * (a.abs() + b.abs()) + lam * tol_m).mean() + U * term.abs().mean(),
               mse=(2.0 * U * (a.abs() + b.abs()) * (a - b).abs() + 2.0 * U * (a - b) ** 2).reshape(3, -1).mean(1),
               map=tol_m, d_static=U * (ta * comp.abs() + tb * t.abs()).sum(0), dE=None)
    if E is None:
        out["d_render"] = U * ta * s.abs()
    else:   # dL/dr_i = s sum_c E[i][c] g_c;  dL/dE[i][c] = sum_p g_c s r_i,  dL/dE[c][3] = sum_p g_c s
        out["d_render"] = torch.stack([U * s.abs() * sum(abs(float(E[i, c])) * ta[c] for c in range(3)) for i in range(3)], 0)
        dE = torch.zeros(3, 4, dtype=torch.float64)
        for c in range(3):
            for i in range(3):
                dE[i, c] = U * (ta[c] * s.abs() * r[i].abs()).sum()
            dE[c, 3] = U * (ta[c] * s.abs()).sum()
        out["dE"] = dE
    return out


def ssim_map_budgets(img1, img2, upstream):
    a, b = img1.double(), img2.double()
    tol_m, kappa2, dm, conv = _map_budget(a, b)
    ta, tb = _grad_budget(a, b, kappa2, dm, conv, weight=upstream.double())
    return dict(map=tol_m, d_img1=U * ta, d_img2=U * tb)


def psnr_budget(mse, tol_mse):
    """The frame PSNR, mean over the channels of -10 log10(mse_c): the MSE budget through 20 log10(1 / sqrt(mse)), plus u for each of the
    square root, the division, log10f (its own error counted as 2 u of the argument) and the product."""
    k = 10.0 / math.log(10.0)
    per = k * tol_mse / mse + U * (k * 4.0 + (10.0 * torch.log10(mse)).abs())
    return per.mean()


# ---------------------------------------------------------------------------------------------------------------- the assertion
def worst_ratio(got, ref, tol):
    """-> (max |got - ref| / tol, flat index of it); 0 / 0 counts as 0, x / 0 as inf, a non-finite `got` as inf."""
    got, ref, tol = (torch.as_tensor(x).detach().double().cpu() for x in (got, ref, tol))
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).reshape(-1)
    k = int(ratio.argmax()) if ratio.numel() else 0
    return float(ratio[k]), k


def assert_within(got, ref, tol, K, what):
    """|got - ref| <= K tol element-wise (a budget of 0 demands the exact value).  The worst ratio goes to DAS3R_TOL_REPORT."""
    from tests.util import _report
    ratio, k = worst_ratio(got, ref, tol)
    _report("budget_ratio", what, ratio if math.isfinite(ratio) else 1e300, K)
    if ratio <= K:
        return ratio
    got, ref, tol = (torch.as_tensor(x).detach().double().cpu() for x in (got, ref, tol))
    where = ""
    if got.dim() >= 2:
        H, W = got.shape[-2:]
        y, x = (k // W) % H, k % W
        where = (f" at {'channel %d, ' % (k // (H * W)) if got.dim() == 3 else ''}(y, x) = ({y}, {x}) of {H} x {W}, (y % 16, x % 16) = "
                 f"({y % 16}, {x % 16}), {min(y, x, H - 1 - y, W - 1 - x)} from the border")
    elif got.dim() == 1:
        where = f" at element {k}"
    g, r, t = (float(v.reshape(-1)[k]) for v in (got, ref, tol))
    raise AssertionError(f"{what}: |got - ref| = {abs(g - r):.3e} is {ratio:.3g} x the budget {t:.3e} (allowed: {K:g} x){where}; got {g:.9g}, ref {r:.9g}")


# ---------------------------------------------------------------------------------------------------------------- shared, computed once
@functools.lru_cache(maxsize=None)
def plain_case(kind, H, W, lam=0.2, grad_loss=3.0, exposure=None):
    """-> (inputs, reference, budgets) of the photometric form; shared by the tests, never modified."""
    inputs = make_inputs(kind, H, W)
    return inputs, photometric(*inputs, lam, grad_loss, exposure), photometric_budgets(*inputs, lam, grad_loss, exposure)


@functools.lru_cache(maxsize=None)
def map_case(kind, H, W):
    """-> ((img1, img2, upstream), reference, budgets) of the ssim_map form: the masked images, as the patched `ssim` receives them."""
    render, gt, static = make_inputs(kind, H, W)
    inputs = (render * static, gt * static, make_upstream(H, W))
    return inputs, ssim_map(*inputs), ssim_map_budgets(*inputs)


PLAIN_OUTPUTS = (("loss", K_LOSS), ("mse", K_LOSS), ("map", K_MAP), ("d_render", K_RENDER), ("d_static", K_STATIC), ("dE", K_STATIC))
MAP_OUTPUTS = (("map", K_MAP), ("d_img1", K_RENDER), ("d_img2", K_RENDER))


def ratios(got, ref, tol, outputs):
    """{output: worst ratio} over the outputs both sides have."""
    return {name: worst_ratio(got[name], ref[name], tol[name])[0] for name, _ in outputs if got.get(name) is not None and ref.get(name) is not None}


if __name__ == "__main__":   # the table the K constants are read from
    worst = {}
    for kind in KINDS:
        for H, W in HOST_SHAPES:
            forms = [(plain_case(kind, H, W), lambda i: photometric(*i, 0.2, 3.0, dtype=torch.float32), PLAIN_OUTPUTS),
                     (plain_case(kind, H, W, exposure=EXPOSURE_B), lambda i: photometric(*i, 0.2, 3.0, EXPOSURE_B, dtype=torch.float32), PLAIN_OUTPUTS),
                     (map_case(kind, H, W), lambda i: ssim_map(*i, dtype=torch.float32), MAP_OUTPUTS)]
            for (inputs, ref, tol), fn, outputs in forms:
                for name, v in ratios(fn(inputs), ref, tol, outputs).items():
                    if v > worst.get(name, (0.0,))[0]:
                        worst[name] = (v, kind, (H, W))
    for name, (v, kind, hw) in sorted(worst.items()):
        print(f"{name:9s} worst fp32-torch ratio {v:8.3f}  ({kind} {hw})   4 x -> {4 * v:8.2f}   K = {2.0 ** math.ceil(math.log2(4 * v)):g}")
