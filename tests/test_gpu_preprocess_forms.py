"""GPU test of the per-Gaussian backward's form choice (das3r_amd/csrc/preprocess_choice.h): one backward per instantiated base form of
preprocess_backward_kernel, on tests/test_gpu_sh_jacobian.py's scene.  The raw name das3r_profile_report lists the launch under equals the
name the header gives for the form the header chooses from the same inputs (das3r_debug_choose_preprocess_backward on what the test passed:
SH rows or colours, M, degree, alignment of the SH tensor, the forward's Jacobian bit, cov3D, depth, antialiasing, chain) — and the base form
is the one written here by hand.  What the forms compute is the business of the parity and bit-identity tests."""
import ctypes as C
import math

import pytest
import torch

from tests import util
from tests.test_gpu_sh_jacobian import SHJAC, _dev, _pre, _scene, _sh_on

pytestmark = pytest.mark.gpu

AA = 16   # das3r_raster_saved.flags bit 4


def _chosen(**kw):
    """-> (raw name less its parentheses, base index) of the form the header chooses."""
    from das3r_amd import _lib
    lib = _lib.load()
    v = dict(has_sh=1, has_cov=0, M=16, sh_degree=3, shs_aligned16=1, dL_dshs_aligned16=1, no_sh_stage=0, jac_saved=0, chained=0, quad_rows=0,
             depth=0, aa=0)
    assert set(kw) <= set(v)
    v.update({k: int(x) for k, x in kw.items()})
    form = _lib.PreprocessForm()
    assert lib.das3r_debug_choose_preprocess_backward(C.byref(_lib.PreprocessBackwardInputs(**v)), C.byref(form)) == 0
    return lib.das3r_debug_preprocess_backward_name(C.byref(form)).decode().strip("()"), form.base_index


def _launched(call):
    """The raw names of the preprocess_backward_kernel launches `call` makes."""
    from das3r_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_report()   # drain
    _lib.profile_enable(True)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return {k: n for k, (n, _ms) in _lib.profile_report(raw=True).items() if k.startswith("preprocess_backward_kernel")}


# (degree, M, SH tensor aligned, Jacobian bit kept, colour source / geometry / extras) -> base form in the header's list
#   "sh": SH rows + scales / rotations   "cov": SH rows + cov3D   "rgb": precomputed colours   "rgbcov": both   "pre": raw parameters
CASES = [
    (3, 16, True, True, "cov", 3), (2, 9, True, True, "cov", 4), (3, 16, True, True, "sh", 5), (2, 9, True, True, "sh", 6),
    (3, 16, True, False, "sh", 7), (2, 16, True, False, "sh", 7), (3, 16, False, False, "sh", 8), (0, 16, True, False, "sh", 8),
    (0, 1, True, False, "sh", 9), (0, 9, False, False, "sh", 9), (2, 9, True, False, "sh", 10), (3, 16, True, False, "cov", 11),
    (3, 16, False, False, "cov", 12), (0, 9, True, False, "cov", 13), (2, 9, True, False, "cov", 14), (3, 16, True, False, "rgb", 15),
    (3, 16, True, False, "rgbcov", 16), (3, 16, True, True, "pre", 5), (2, 9, False, False, "pre", 10),
    (3, 16, True, True, "sh depth", 5), (2, 9, True, False, "sh aa", 10), (0, 1, True, False, "sh depth aa", 9),
]


@pytest.mark.parametrize("D,M,aligned,keep_jac,what,base", CASES)
def test_the_launched_form_is_the_one_the_header_chooses(D, M, aligned, keep_jac, what, base):
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    dev = _dev()
    sc = _scene(D, M)
    words = what.split()
    kind, depth, aa = words[0], "depth" in words, "aa" in words
    cov, rgb = kind in ("cov", "rgbcov"), kind in ("rgb", "rgbcov")
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()})
    means3D, opac = sc.means3D.to(dev), sc.opacities.to(dev)
    shs = e if rgb else _sh_on(dev, sc.shs, aligned)
    colors = torch.rand(sc.P, 3, generator=torch.Generator().manual_seed(9)).to(dev) if rgb else e
    scales, rot = (e, e) if cov else (sc.scales.to(dev), sc.rotations.to(dev))
    cov3D = util.cov3d_of(sc).to(dev) if cov else e
    keep = []
    pre = _pre(sc, dev, keep) if kind == "pre" else None
    fw = rasterizer._forward_full(rs, means3D, shs, colors, opac, scales, rot, cov3D, exact=True, pre=pre, invdepth=depth, antialiasing=aa)
    I, _color, _radii, geom, binning, img, cap = fw[:7]
    assert bool(cap.flags & SHJAC) == (not rgb and D >= 2) and bool(cap.flags & AA) == aa
    ticket = rasterizer._Capacity(int(cap))
    ticket.check_word, ticket.check_tag, ticket.flags = cap.check_word, cap.check_tag, cap.flags if keep_jac else cap.flags & ~SHJAC
    dD = torch.ones(1, sc.H, sc.W, device=dev) / (sc.W * sc.H) if depth else None
    ran = _launched(lambda: rasterizer._backward_impl(rs, I, sc.dL_dpix.to(dev), means3D, shs, colors, opac, scales, rot, cov3D, geom, binning, img,
                                                      ticket, pre=pre, grad_invdepth=dD))
    name, index = _chosen(has_sh=not rgb, has_cov=cov, M=0 if rgb else M, sh_degree=D, shs_aligned16=shs.data_ptr() % 16 == 0,
                          jac_saved=bool(ticket.flags & SHJAC), depth=depth, aa=aa)
    print(f"D{D} M{M} {what}: {ran}")
    assert index == base
    assert ran == {name: 1}


def test_chained_jacobian_form():
    """grads->chain at degree 2 with M = 9, the forward's Jacobian bit set: the chained form that reads the planes."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    dev = _dev()
    sc = _scene(2, 9)
    keep = []
    pre = _pre(sc, dev, keep)
    xyz, rot, scaling, logit, conf, _mats = keep
    params = [xyz, rot, scaling, logit]
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()})
    shs = sc.shs.to(dev)
    I, _, _, geom, binning, img, cap = rasterizer._forward_full(rs, xyz, shs, e, logit, scaling, rot, e, exact=True, pre=pre)
    assert cap.flags & SHJAC
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    slots = (_lib.AdamSlot * 4)()
    for k in range(4):
        slots[k].param, slots[k].exp_avg, slots[k].exp_avg_sq = params[k].data_ptr(), m[k].data_ptr(), v[k].data_ptr()
        slots[k].step_size, slots[k].bc2_sqrt = 1e-3, math.sqrt(1.0 - 0.999)
    g_conf, g_small = torch.zeros_like(conf), torch.zeros(28, device=dev)
    chain = _lib.Chain()
    chain.g_conf_flat, chain.g_small, chain.slots = g_conf.data_ptr(), g_small.data_ptr(), slots
    chain.beta1, chain.beta2, chain.eps = 0.9, 0.999, 1e-15
    ran = _launched(lambda: rasterizer._backward_impl(rs, I, sc.dL_dpix.to(dev), xyz, shs, e, logit, scaling, rot, e, geom, binning, img, cap,
                                                      pre=pre, chain=chain))
    name, index = _chosen(M=9, sh_degree=2, jac_saved=1, chained=1)
    assert index == 1 and ran == {name: 1}, ran


@pytest.mark.parametrize("degree,base", [(0, 0), (1, 2)])
def test_chained_forms_of_a_train_step(degree, base):
    """The fused train step with the backward chained through the pose pre-transform (tests/test_gpu_trainstep.py's model): degree 0, and
    SH rows at degree 1 (M = 4)."""
    from das3r_amd import fast_step
    from das3r_amd.train import train_step
    from tests.test_gpu_trainstep import PIPE, _pair
    bg = torch.zeros(3, device="cuda")
    model, cams, _, opt, _dense = _pair(frames=4, W=48, H=32, seed=23, heldout=False, iterations=4000, fused=True, generic=True)
    model.fast_step = True
    model.fuse_backward_chain = True
    if degree:
        model.active_sh_degree = degree
        model.optimizer.set_active_sh_degree(degree)
    assert fast_step.available(model, PIPE)
    ran = _launched(lambda: train_step(model, cams[0], opt, 100, PIPE, bg, fused=True))
    name, index = _chosen(M=(degree + 1) ** 2, sh_degree=degree, chained=1)
    assert index == base and ran == {name: 1}, ran


def test_the_cases_reach_every_base_form():
    assert sorted({c[-1] for c in CASES} | {0, 1, 2}) == list(range(17))
