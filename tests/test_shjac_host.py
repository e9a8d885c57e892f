"""CPU test of the SH-Jacobian planes' host side: the geometry buffer a forward asks for grows by 36 bytes per Gaussian exactly when it
is given SH coefficients at an active degree >= 2 (das3r_raster_saved.flags bit 2), and keeps its size for degrees 0 / 1, for
precomputed colours and for a forward whose caller says no backward will follow (flags bit 3 on the way in).  The allocators record the sizes and return NULL: the forward stops there, before the device is touched."""
import ctypes

import pytest


def _geom_request(hip_lib, P, D, M, sh, flags_in=0):
    from das3r_amd import _lib
    a, i, o, s = _lib.RasterArgs(), _lib.RasterIn(), _lib.RasterOut(), _lib.RasterSaved()
    a.P, a.image_width, a.image_height, a.M, a.sh_degree = P, 64, 48, M, D
    a.tanfovx = a.tanfovy = 1.0
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: nothing is launched once an allocation fails
    a.bg = a.viewmatrix = a.projmatrix = a.campos = fake
    i.means3D = i.opacities = i.scales = i.rotations = fake
    if sh:
        i.shs = fake
    else:
        i.colors_precomp = fake
    o.out_color = o.radii = fake
    s.flags = flags_in
    sizes = []
    cb = _lib.ALLOC_FN(lambda u, n: sizes.append(n) or 0)
    rc = hip_lib.das3r_raster_forward(ctypes.byref(a), ctypes.byref(i), ctypes.byref(o), cb, cb, cb, None, ctypes.byref(s), None)
    assert rc < 0 and b"allocation failed" in hip_lib.das3r_last_error()
    return sizes[0]


@pytest.mark.parametrize("P", [64, 4096, 1000])
def test_geom_grows_by_the_jacobian_planes_only_at_degree_2_and_up(hip_lib, P):
    from das3r_amd import _lib
    base = _lib.layout(P, 0, 64, 48)["geom_bytes"]
    planes = (36 * P + 255) // 256 * 256   # (regions of the buffer are 256-byte aligned)
    for D in range(4):
        for M in sorted({(D + 1) ** 2, 16}):
            want = base + planes if D >= 2 else base
            assert _geom_request(hip_lib, P, D, M, sh=True) == want, (P, D, M)
        assert _geom_request(hip_lib, P, D, 16, sh=False) == base, (P, D, "colors_precomp")
        # flags bit 3 on the way in: no backward will follow, no planes
        assert _geom_request(hip_lib, P, D, 16, sh=True, flags_in=_lib.NO_BACKWARD_IN_FLAG) == base, (P, D, "no backward")
