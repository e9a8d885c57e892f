"""CPU tests of the wiring inside das3r_amd/rasterizer.py: RasterState as the one builder of das3r_raster_saved, the shared helpers, the
tuple interface's signatures (bench.py, the tools and most GPU tests call them), and that per-call state travels as arguments — nothing
but GaussianRasterizer.__call__ and forward touches the module's thread-local.  The calls themselves: tests/test_gpu_rasterizer_calls.py."""
import inspect
import re

import torch


def _state(capacity):
    from das3r_amd.rasterizer import RasterState
    buf = lambda n: torch.zeros(n, dtype=torch.uint8)
    return RasterState(buf(16), buf(32), buf(48), 90, capacity, 10, 32, 16, torch.device("cuda", 0))


def test_raster_state_builds_the_saved_struct_from_a_ticketed_capacity_as_from_a_plain_int():
    from das3r_amd.rasterizer import _Capacity
    cap = _Capacity(100)
    cap.check_word, cap.check_tag, cap.flags = 0x1000, 7, 2 | 16
    ticketed, plain = _state(cap), _state(100)
    a, b = ticketed.saved(), plain.saved()
    for s, st in ((a, ticketed), (b, plain)):
        assert (s.geom, s.binning, s.img) == (st.geom.data_ptr(), st.binning.data_ptr(), st.img.data_ptr())
        assert (s.num_rendered, s.capacity) == (90, 100)
    assert (a.check_word, a.check_tag, a.flags) == (0x1000, 7, 18) and ticketed.flags == 18
    assert (b.check_word, b.check_tag, b.flags) == (None, 0, 0) and plain.flags == 0
    # the self-check reads the ticket alone
    t = ticketed.saved(buffers=False)
    assert (t.check_word, t.check_tag) == (0x1000, 7)
    assert (t.geom, t.binning, t.img, t.num_rendered, t.capacity, t.flags) == (None, None, None, 0, 0, 0)
    # the aux-channel calls: P and the extents, and the same struct
    args, s = ticketed._c_args()
    assert (args.P, args.image_width, args.image_height, args.M, args.sh_degree) == (10, 32, 16, 0, 0)
    assert all(getattr(s, n) == getattr(a, n) for n, _ in type(s)._fields_)
    plain.check()   # (no ticket: returns before the library or a device is touched)


def test_state_of_a_forward_result_is_the_positional_construction():
    from das3r_amd.rasterizer import RasterState
    from types import SimpleNamespace
    res = (90, torch.zeros(3, 16, 32), torch.zeros(10, dtype=torch.int32), torch.zeros(1), torch.zeros(2), torch.zeros(3), 100, torch.zeros(1, 16, 32))
    st = RasterState.of(res, SimpleNamespace(image_width=32, image_height=16))
    assert (st.geom, st.binning, st.img) == (res[3], res[4], res[5])
    assert (st.num_rendered, st.capacity, st.P, st.W, st.H, st.device) == (90, 100, 10, 32, 16, torch.device("cpu"))


def test_chunks_are_eight_channels_at_a_time():
    from das3r_amd.rasterizer import _chunks
    assert _chunks(11) == [(0, 8), (8, 3)]
    for n in range(1, 9):
        assert _chunks(n) == [(0, n)]
    assert _chunks(16) == [(0, 8), (8, 8)] and _chunks(17) == [(0, 8), (8, 8), (16, 1)]
    assert _chunks(0) == [(0, 0)]   # the coverage alone still takes its one call


def test_dense_and_placeholders():
    from das3r_amd.rasterizer import _dense, _empty, _or_empty
    assert _dense(None) is None
    g = torch.zeros(3, 4)
    assert _dense(g) is g
    d = _dense(torch.zeros(4, 3, dtype=torch.float64).t())
    assert d.dtype == torch.float32 and d.is_contiguous() and d.shape == (3, 4)
    cpu = torch.device("cpu")
    assert _or_empty(cpu, None, g, None) == (_empty(cpu), g, _empty(cpu)) and _empty(cpu).numel() == 0


def test_one_rasterising_function_and_the_removed_names_are_gone():
    import diff_gaussian_rasterization
    from das3r_amd import rasterizer
    for name in ("_RasterizeGaussiansInvDepth", "_RasterizeGaussiansFocal", "_apply"):
        assert not hasattr(rasterizer, name), name
    assert diff_gaussian_rasterization._RasterizeGaussians is rasterizer._RasterizeGaussians
    params = list(inspect.signature(rasterizer._RasterizeGaussians.forward).parameters)
    assert params == ["ctx", "means3D", "means2D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3Ds_precomp", "raster_settings",
                      "options", "log_focal"]   # upstream's nine, then the two optional ones
    o = rasterizer._Options()
    assert (o.invdepth, o.antialiasing, o.no_backward, o.want_state, o.state) == (False, False, False, False, None)


def _functions(module):
    """every function the module defines, methods of its classes included -> {qualified name: function}"""
    out = {}
    for name, obj in vars(module).items():
        if inspect.isfunction(obj) and obj.__module__ == module.__name__:
            out[name] = obj
        elif inspect.isclass(obj) and obj.__module__ == module.__name__:
            for k, v in vars(obj).items():
                v = getattr(v, "__func__", v)
                if inspect.isfunction(v) and v.__code__.co_filename == module.__file__:   # (not a NamedTuple's generated methods)
                    out[f"{name}.{k}"] = v
    return out


def test_only_the_module_call_and_forward_touch_the_thread_local():
    from das3r_amd import rasterizer
    fns = _functions(rasterizer)
    assert len(fns) > 40 and "RasterState.saved" in fns and "_RasterizeGaussians.backward" in fns
    touching = sorted(n for n, f in fns.items() if re.search(r"\b_last\b", inspect.getsource(f)))
    assert touching == ["GaussianRasterizer.__call__", "GaussianRasterizer.forward"]
    # ... and only for the two keywords of the call
    assert set(re.findall(r"\b_last\.(\w+)", inspect.getsource(rasterizer))) == {"log_focal", "aux_geometry_grad"}


SIGNATURES = {   # copied from the code before the binding was reorganised: bench.py, the tools and most GPU tests call these
    "_forward_full": "(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, exact=False, pre=None, invdepth=False, "
                     "no_backward=False, antialiasing=False)",
    "_forward_impl": "(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)",
    "_backward_impl": "(rs, num_rendered, grad_out_color, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, geom, binning, "
                      "img, capacity=None, _scratch_misalign=0, pre=None, chain=None, grad_invdepth=None, focal=False, focal_per_splat=False, "
                      "_fill=None)",
    "_aux_backward_impl": "(state, rs, features, grad_image, grad_alpha, want_features, means3D, sh, colors_precomp, opacities, scales, rotations, "
                          "cov3Ds_precomp, _scratch_misalign=0, _fill=None)",
    "check_forward": "(capacity, device)",
    "count_live_pairs": "(rs, P, M, num_rendered, geom, binning, img, capacity)",
    "RasterState": "(geom, binning, img, num_rendered, capacity, P, W, H, device)",
    "RasterState.of": "(res, rs)",
}


def test_the_tuple_interface_keeps_its_signatures():
    from das3r_amd import rasterizer
    for name, want in SIGNATURES.items():
        obj = rasterizer
        for part in name.split("."):
            obj = getattr(obj, part)
        assert str(inspect.signature(obj)) == want, name
    cap = rasterizer._Capacity(5)
    assert isinstance(cap, int) and cap == 5 and (cap.check_word, cap.check_tag, cap.flags) == (None, 0, 0)
    for name in ("_fill_args", "_fill_in", "_on_device", "_stream", "_needs_device", "rasterize_gaussians"):   # host tests patch these
        assert callable(getattr(rasterizer, name)), name
    assert callable(rasterizer._Alloc.get)


def test_count_live_pairs_is_declared_with_the_other_exports(hip_lib):
    import ctypes as C
    from das3r_amd import _lib, rasterizer
    f = hip_lib.das3r_raster_count_live_pairs
    assert f.restype is C.c_int and len(f.argtypes) == 4 and f.argtypes[0] is C.POINTER(_lib.RasterArgs) and f.argtypes[1] is C.POINTER(_lib.RasterSaved)
    assert "argtypes" not in inspect.getsource(rasterizer) and "restype" not in inspect.getsource(rasterizer)
