"""The float64 reference of the normal-consistency regulariser (tests/normal_reference.py) checked against closed forms and finite differences,
on the CPU: the GPU tests compare the kernels with a reference that has itself been checked."""
import math

import pytest
import torch

from tests import normal_reference as nref

TANFOV = (0.7, 0.45)   # unequal on purpose


def _unit(v):
    v = torch.tensor(v, dtype=torch.float64)
    return v / v.norm()


PLANES = {"fronto_parallel": ((0.0, 0.0, -1.0), -3.0),
          "tilted_in_x": ((0.5, 0.0, -1.0), -3.0),
          "tilted_in_both": ((-0.3, 0.4, -1.0), -2.5)}


@pytest.mark.parametrize("name", list(PLANES))
def test_a_plane_gives_its_own_normal_and_a_zero_loss(name):
    n, c = PLANES[name]
    n = _unit(n)
    H, W = 11, 14
    z = nref.plane_depth(H, W, *TANFOV, n, c * 1.0 / torch.tensor(PLANES[name][0], dtype=torch.float64).norm())
    assert bool((z > 0).all())
    N, valid = nref.depth_normals(z, *TANFOV)
    assert bool(valid[1:-1, 1:-1].all()) and not bool(valid[0].any() | valid[-1].any() | valid[:, 0].any() | valid[:, -1].any())
    assert float((N[:, 1:-1, 1:-1] - n[:, None, None]).abs().max()) < 1e-12
    assert float(N[:, 0].abs().max()) == 0.0 and float(N[:, :, -1].abs().max()) == 0.0
    alpha = torch.rand(H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    loss, _, _ = nref.normal_consistency(z, alpha[None] * n[:, None, None], alpha, *TANFOV)
    assert float(loss.abs().max()) < 1e-12
    # and the opposite normal costs 2 alpha
    loss, _, _ = nref.normal_consistency(z, -alpha[None] * n[:, None, None], alpha, *TANFOV)
    assert float((loss[1:-1, 1:-1] - 2 * alpha[1:-1, 1:-1]).abs().max()) < 1e-12


def test_a_fronto_parallel_plane_faces_the_camera():
    N, _ = nref.depth_normals(torch.full((5, 6), 2.0, dtype=torch.float64), *TANFOV)
    assert torch.equal(N[:, 2, 2], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64))


def _smooth_depth(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return 3.0 + torch.sin(0.7 * xs) * torch.cos(0.5 * ys) + 0.05 * torch.randn(H, W, dtype=torch.float64, generator=g)


def _fd(f, x, eps=1e-6):
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + eps
        hi = float(f())
        flat[i] = keep - eps
        lo = float(f())
        flat[i] = keep
        gf[i] = (hi - lo) / (2 * eps)
    return g


def test_autograd_of_the_image_term_agrees_with_central_differences():
    H, W = 6, 7
    gen = torch.Generator().manual_seed(5)
    z = _smooth_depth(H, W, 3)
    normal = torch.randn(3, H, W, dtype=torch.float64, generator=gen)
    alpha = torch.rand(H, W, dtype=torch.float64, generator=gen)
    mask = torch.rand(H, W, dtype=torch.float64, generator=gen)
    G = torch.randn(H, W, dtype=torch.float64, generator=gen)
    leaves = [t.clone().requires_grad_(True) for t in (z, normal, alpha)]
    (nref.normal_consistency(*leaves, *TANFOV, mask)[0] * G).sum().backward()
    for k, t in enumerate((z, normal, alpha)):
        args = [z, normal, alpha]
        fd = _fd(lambda: (nref.normal_consistency(*args, *TANFOV, mask)[0] * G).sum(), t)
        assert float((leaves[k].grad - fd).abs().max()) <= 1e-7 * max(1.0, float(fd.abs().max())), k
    assert float(leaves[0].grad.abs().max()) > 0
    # a pixel's own depth does not enter its own normal: the centre of a 3 x 3 image has no gradient
    z3 = _smooth_depth(3, 3, 4).requires_grad_(True)
    nref.normal_consistency(z3, torch.randn(3, 3, 3, dtype=torch.float64, generator=gen), torch.rand(3, 3, dtype=torch.float64, generator=gen),
                            *TANFOV)[0].sum().backward()
    assert float(z3.grad[1, 1]) == 0.0 and float(z3.grad[1, 0].abs()) > 0 and float(z3.grad[0, 0]) == 0.0


def test_autograd_of_the_gaussian_normals_agrees_with_central_differences():
    gen = torch.Generator().manual_seed(8)
    P = 7
    q = torch.randn(P, 4, dtype=torch.float64, generator=gen) * torch.tensor([0.1, 1.0, 10.0, 1.0, 1.0, 3.0, 0.5], dtype=torch.float64)[:, None]
    s = torch.rand(P, 3, dtype=torch.float64, generator=gen) + 0.1
    mu = torch.randn(P, 3, dtype=torch.float64, generator=gen) + torch.tensor([0.0, 0.0, 4.0], dtype=torch.float64)
    V = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=gen))[0]
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = V
    campos = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    G = torch.randn(P, 3, dtype=torch.float64, generator=gen)
    ql = q.clone().requires_grad_(True)
    out = nref.gaussian_normals(ql, s, mu, view, campos)
    assert float((out["normals"].detach().norm(dim=1) - 1).abs().max()) < 1e-12
    # facing the camera: n_world . d <= 0
    n_world = out["normals"].detach() @ V.t()
    assert bool(((n_world * (mu - campos)).sum(1) <= 0).all())
    (out["normals"] * G).sum().backward()
    fd = _fd(lambda: (nref.gaussian_normals(q, s, mu, view, campos)["normals"] * G).sum(), q, eps=1e-6)
    assert float((ql.grad - fd).abs().max()) <= 1e-6 * float(fd.abs().max())
    # through the normalisation: the gradient is orthogonal to q and scales with 1 / |q|
    assert float((ql.grad * q).sum(1).abs().max()) <= 1e-10 * float(ql.grad.abs().max())


def test_ties_take_the_lowest_axis_and_a_zero_product_keeps_the_axis():
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 4, dtype=torch.float64)
    s = torch.tensor([[0.5, 0.5, 0.5], [0.7, 0.5, 0.5], [0.5, 0.7, 0.5], [0.5, 0.5, 0.7]], dtype=torch.float64)
    mu = torch.tensor([[0.0, 0.0, 1.0]] * 4, dtype=torch.float64)
    out = nref.gaussian_normals(q, s, mu, torch.eye(4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    assert out["k"].tolist() == [0, 1, 0, 0]
    assert out["flip"].tolist() == [False, False, False, False]          # a = e_0 or e_1, d = e_2: the product is exactly 0
    assert torch.equal(out["normals"][0], torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    s2 = torch.tensor([[0.5, 0.5, 0.1]], dtype=torch.float64)
    out = nref.gaussian_normals(q[:1], s2, mu[:1], torch.eye(4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    assert out["choice"].tolist() == [2 | 4] and torch.equal(out["normals"][0], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64))


@pytest.mark.parametrize("bad", [0.0, float("nan"), float("inf"), -1.0])
def test_invalid_pixels_give_exact_zeros_and_do_not_leak(bad):
    H, W = 8, 9
    gen = torch.Generator().manual_seed(11)
    z = _smooth_depth(H, W, 6)
    z[3, 4] = bad
    normal = torch.randn(3, H, W, dtype=torch.float64, generator=gen)
    alpha = torch.rand(H, W, dtype=torch.float64, generator=gen)
    leaves = [t.clone().requires_grad_(True) for t in (z, normal, alpha)]
    loss, N, valid = nref.normal_consistency(*leaves, *TANFOV)
    hole = [(3, 4), (3, 3), (3, 5), (2, 4), (4, 4)]                      # the pixel and the four whose stencils read it
    for y, x in hole:
        assert not bool(valid[y, x]) and float(loss[y, x]) == 0.0 and float(N[:, y, x].abs().max()) == 0.0
    assert int(valid.sum()) == (H - 2) * (W - 2) - len(hole)
    assert float(loss[0].abs().max()) == 0.0 and float(loss[:, 0].abs().max()) == 0.0
    loss.sum().backward()
    for t in leaves:
        assert bool(torch.isfinite(t.grad).all())
    assert float(leaves[0].grad[3, 4]) == 0.0                            # nobody's valid stencil reads the hole
    for y, x in hole:
        assert float(leaves[1].grad[:, y, x].abs().max()) == 0.0 and float(leaves[2].grad[y, x]) == 0.0
    # neighbours of the invalid pixels still get the gradient of THEIR valid readers: (3, 2) is read by (3, 1) alone
    assert float(leaves[0].grad[3, 2].abs()) > 0
    # the same image without the hole, restricted to the pixels whose readers are untouched, has the same gradient
    z_ok = _smooth_depth(H, W, 6).requires_grad_(True)
    nref.normal_consistency(z_ok, normal, alpha, *TANFOV)[0].sum().backward()
    assert float(leaves[0].grad[6, 7]) == float(z_ok.grad[6, 7]) and math.isfinite(float(z_ok.grad[6, 7]))
