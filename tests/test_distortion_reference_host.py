"""The float64 reference of the ray-distortion regulariser (tests/distortion_reference.py) on its own: no device, no library.  The kernels are
held to it in tests/test_gpu_distortion.py; here its two forms, the backward formulas of include/das3r_raster.h and the invariances the
kernels rely on are checked against each other and against autograd."""
import pytest
import torch

from tests import distortion_reference as ref

_CACHE = {}


def _scene():
    """24 x 20 pixels, 40 Gaussians -> (D [H, W], compacted w / m / valid [Npix, K]); computed once, never written to."""
    if "s" not in _CACHE:
        from das3r_amd.synth import make_scene
        sc = make_scene(P=40, W=24, H=20, focal=20.0, sh_degree=0, seed=5, s_px=(0.6, 2.5))
        kw = dict(means3D=sc.means3D.double(), means2D=torch.zeros(sc.P, 3, dtype=torch.float64), shs=sc.shs.double(), scales=sc.scales.double(),
                  rotations=sc.rotations.double())
        skw = {k: v for k, v in sc.settings_kwargs().items() if k not in ("prefiltered", "debug")}
        D, pieces = ref.distortion_reference(sc.opacities.double(), **kw, **skw)
        _CACHE["s"] = (D.detach(), pieces["w"].detach(), pieces["m"].detach(), pieces["valid"])
    return _CACHE["s"]


def test_scene_has_rays_with_several_contributors():
    D, w, m, valid = _scene()
    n = valid.sum(1)
    assert int(n.max()) >= 4 and int((n >= 2).sum()) >= 50 and int((n == 1).sum()) >= 1 and float(D.max()) > 0


def test_pairwise_form_equals_the_prefix_form_in_list_order():
    D, w, m, _ = _scene()
    assert float((ref.pairwise_form(w, m) - ref.prefix_form(w, m)).abs().max()) <= 1e-12
    assert float((D.reshape(-1) - ref.prefix_form(w, m)).abs().max()) <= 1e-12
    assert float(ref.prefix_form(w, m).min()) >= -1e-15, "the list is in depth order: every term is >= 0"


def test_backward_formulas_equal_autograd():
    """q_k = m_k (2 SA_k - A) - (2 SB_k - B) and dD/dm_k = w_k (2 SA_k + w_k - A), SA / SB the sums over the entries behind k."""
    _, w, m, valid = _scene()
    wl, ml = w.clone().requires_grad_(True), m.clone().requires_grad_(True)
    gw, gm = torch.autograd.grad(ref.pairwise_form(wl, ml).sum(), [wl, ml])
    gw, gm = gw * valid, gm * valid   # (a padding entry behind a pixel's list has w = 0 and somebody else's m: no list position, no formula)
    A, B = w.sum(1, keepdim=True), (w * m).sum(1, keepdim=True)
    SA = A - torch.cumsum(w, 1)
    SB = B - torch.cumsum(w * m, 1)
    q = (m * (2 * SA - A) - (2 * SB - B)) * valid
    dm = w * (2 * SA + w - A)
    assert float((q - gw).abs().max()) <= 1e-10 and float((dm - gm).abs().max()) <= 1e-10
    assert float(gw.abs().max()) > 1e-3 and float(gm.abs().max()) > 1e-3


def test_invariant_under_a_shift_and_linear_in_a_scale_of_m():
    D, w, m, _ = _scene()
    scale = float(D.max())
    for c in (-3.0, 0.25, 1e3):
        assert float((ref.pairwise_form(w, m + c).reshape(D.shape) - D).abs().max()) <= 1e-9 * max(1.0, abs(c)) * scale
        assert float((ref.prefix_form(w, m + c).reshape(D.shape) - D).abs().max()) <= 1e-9 * max(1.0, abs(c)) * scale
    for s in (0.5, 7.0):
        assert float((ref.pairwise_form(w, s * m).reshape(D.shape) - s * D).abs().max()) <= 1e-12 * s * scale


def test_a_pixel_with_one_contributor_is_exactly_zero():
    D, w, m, valid = _scene()
    one = valid.sum(1) == 1
    none = valid.sum(1) == 0
    assert bool(one.any())
    assert float(D.reshape(-1)[one].abs().max()) == 0.0
    if bool(none.any()):
        assert float(D.reshape(-1)[none].abs().max()) == 0.0


def test_a_tie_takes_the_fixed_order_derivative():
    """Two entries at one depth: the value is 0 and the derivative is that of w_0 w_1 (m_0 - m_1), entry 0 in front (module docstring)."""
    w = torch.tensor([[0.3, 0.2]], dtype=torch.float64)
    m = torch.tensor([[0.5, 0.5]], dtype=torch.float64, requires_grad=True)
    D = ref.pairwise_form(w, m)
    assert float(D.detach()) == 0.0
    (g,) = torch.autograd.grad(D.sum(), [m])
    assert torch.allclose(g, torch.tensor([[0.06, -0.06]], dtype=torch.float64), atol=1e-15)


def test_the_rebuilt_coverage_is_checked_against_the_oracle():
    """rebuild_weights asserts 1 - prod(1 - alpha) over keep against 1 - T_final: a wrong opacity trips it."""
    from das3r_amd.synth import make_scene
    from oracle.dense_oracle import rasterize_dense
    sc = make_scene(P=12, W=16, H=16, focal=14.0, sh_degree=0, seed=6, s_px=(2.0, 5.0))
    kw = dict(means3D=sc.means3D.double(), means2D=torch.zeros(sc.P, 3, dtype=torch.float64), shs=sc.shs.double(), scales=sc.scales.double(),
              rotations=sc.rotations.double())
    skw = {k: v for k, v in sc.settings_kwargs().items() if k not in ("prefiltered", "debug")}
    aux = rasterize_dense(opacities=sc.opacities.double(), **kw, **skw)[2]
    ref.rebuild_weights(aux, sc.opacities.double(), sc.H, sc.W)
    with pytest.raises(AssertionError, match="rebuilt coverage"):
        ref.rebuild_weights(aux, 0.9 * sc.opacities.double(), sc.H, sc.W)
