"""The wiring of das3r_amd/rasterizer.py, pinned as a trace of library calls: which entry is called, with which integer arguments and
flags, and which pointers are NULL — what the parity tests can only report as "gradient differs".  A recording proxy stands around the object
`_lib.load()` returns and forwards every call to the real library.  Pointer values, capacities and learnt hint bits are not recorded (the
capacity a scratch query or a backward is handed is recorded as "the forward's" or not); `_lib.forget_shapes()` comes first.

The expected trace, tests/traces/rasterizer_calls.json, is a recording: `python -m tests.test_gpu_rasterizer_calls` rewrites it from the
code as it stands.  The committed one was made by the binding as it was before it was reorganised around RasterState.  In every configuration the results and every returned gradient must also be the same bit for bit in two runs (a buffer
freed or reused too early shows there).  Scene: 48 random Gaussians in front of the camera, 40 x 24 pixels — 3 x 2 tiles, partial on both axes."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traces", "rasterizer_calls.json")
P, W, H = 48, 40, 24

# the recorded entries' parameters, as include/das3r_raster.h names them
SIGNATURES = {
    "das3r_raster_forward": ("args", "in", "out", "alloc_geom", "alloc_binning", "alloc_img", "user", "saved", "stream"),
    "das3r_raster_backward": ("args", "in", "saved", "dL_dpix", "grads", "stream"),
    "das3r_raster_backward_depth": ("args", "in", "saved", "dL_dpix", "dL_dinvdepth", "grads", "stream"),
    "das3r_raster_backward_focal": ("args", "in", "saved", "dL_dpix", "dL_dinvdepth", "grads", "sums", "per_splat", "workspace", "stream"),
    "das3r_raster_check": ("saved", "stream"),
    "das3r_raster_aux_forward": ("args", "saved", "C", "features", "out", "stream"),
    "das3r_raster_aux_adjoint": ("args", "saved", "C", "dL_dout", "out", "accumulate", "scratch", "stream"),
    "das3r_raster_aux_backward": ("args", "in", "saved", "C", "features", "dL_dout", "dL_dalpha", "dL_dfeatures", "grads", "stream"),
    "das3r_raster_count_live_pairs": ("args", "saved", "out", "stream"),
    "das3r_mark_visible": ("P", "positions", "viewmatrix", "projmatrix", "present", "stream"),
}
INTEGERS = ("P", "C", "accumulate")
QUERIES = ("_scratch_bytes", "_workspace_bytes")
FLAGS_IN, FLAGS_OUT = 8 | 16, 2 | 4 | 16   # das3r_raster_saved.flags: bits 3 and 4 on entry; bits 1, 2 and 4 on exit


def _null_fields(s):
    """the pointer fields of a ctypes structure that are NULL"""
    return [n for n, t in s._fields_ if (t is C.c_void_p or issubclass(t, C._Pointer)) and not getattr(s, n)]


def _is_null(a):
    return a is None or (isinstance(a, int) and a == 0) or (isinstance(a, C.c_void_p) and not a.value)


class _Entry:
    def __init__(self, rec, name, fn):
        self.__dict__.update(rec=rec, name=name, fn=fn)

    def __setattr__(self, k, v):   # (restype / argtypes go to the function itself)
        setattr(self.fn, k, v)

    def __call__(self, *args):
        from das3r_amd import _lib
        rec, name = self.rec, self.name
        if name.endswith(QUERIES):
            vals = [int(getattr(a, "value", a)) for a in args]
            if name.endswith("_scratch_bytes"):   # (capacity, ...): the capacity itself is not recorded, only whose it is
                vals[0] = "the forward's capacity" if rec.capacity is not None and vals[0] == max(rec.capacity, 1) else vals[0]
            rec.calls.append({"entry": name, "args": vals})
            return self.fn(*args)
        e = {"entry": name}
        saved = None
        for label, a in zip(SIGNATURES[name], args):
            s = getattr(a, "_obj", None)
            if label == "stream":
                continue
            if isinstance(s, _lib.RasterArgs):
                e["args"] = {"P": s.P, "M": s.M, "sh_degree": s.sh_degree, "W": s.image_width, "H": s.image_height,
                             "capacity_hint": s.capacity_hint, "prefiltered": s.prefiltered, "debug": s.debug}
            elif isinstance(s, _lib.RasterSaved):
                saved = s
                e["saved"] = {"null": _null_fields(s), "flags_in": int(s.flags) & FLAGS_IN}
                if name != "das3r_raster_forward":
                    e["saved"].update(check_tag=bool(s.check_tag), num_rendered_is_the_forwards=s.num_rendered == rec.num_rendered,
                                      capacity_is_the_forwards=s.capacity == rec.capacity)
            elif isinstance(s, (_lib.RasterIn, _lib.RasterOut, _lib.RasterGrads)):
                e[label] = {"null": _null_fields(s)}
            elif label in INTEGERS:
                e[label] = int(getattr(a, "value", a))
            elif _is_null(a):
                e.setdefault("null_arguments", []).append(label)
        rc = self.fn(*args)
        e["ok"] = rc >= 0
        if saved is not None:
            e["saved"]["flags_out"] = int(saved.flags) & FLAGS_OUT
            if name == "das3r_raster_forward":
                e["saved"]["check_tag"] = bool(saved.check_tag)
                rec.num_rendered, rec.capacity = int(rc), int(saved.capacity)
        rec.calls.append(e)
        return rc


class _Recorder:
    """Stands around the loaded library: every attribute is the library's; calls of the rasterizer's entries are recorded on their way."""

    def __init__(self, lib):
        self.__dict__.update(lib=lib, calls=[], num_rendered=None, capacity=None)

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        return _Entry(self, name, fn) if name in SIGNATURES or name.endswith(QUERIES) else fn


# ---- the scene and the configurations

_HOST = {}


def _host():
    """the scene's tensors on the host, made once and never written to"""
    if not _HOST:
        from das3r_amd.synth import make_scene
        from tests import util
        sc = make_scene(P=P, W=W, H=H, focal=36.0, sh_degree=3, seed=48, s_px=(1.0, 5.0), bg=(0.1, 0.2, 0.3))
        _HOST.update(sc=sc, means3D=sc.means3D, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations, shs=sc.shs,
                     colors_precomp=torch.sigmoid(sc.shs[:, 0, :] * 1.3).contiguous(), cov3D_precomp=util.cov3d_of(sc),
                     features=torch.rand(P, 11, generator=torch.Generator().manual_seed(5)))
    return _HOST


def _settings(dev, **over):
    from das3r_amd import GaussianRasterizationSettings
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _host()["sc"].settings_kwargs().items()}
    kw.update(over)
    return GaussianRasterizationSettings(**kw)


def _leaves(dev, names, grad=True):
    out = {k: _host()[k].to(dev).clone().requires_grad_(grad) for k in names}
    out["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=grad)
    return out


def _weight(t, seed):
    return (torch.randn(t.shape, generator=torch.Generator().manual_seed(seed)) / float(t.numel())).to(t.device)


def _log_focal(dev, grad):
    sc = _host()["sc"]
    return (-torch.log(torch.tensor([sc.tanfovx, sc.tanfovy]))).to(dev).requires_grad_(grad)


GEOMETRY = ("means3D", "opacities", "scales", "rotations")


def _module(dev, names=("colors_precomp",) + GEOMETRY, loss=(0,), settings=None, keep_state=False, **call):
    """One GaussianRasterizer call and the backward of a seeded linear loss on the results `loss` indexes -> results, then gradients."""
    from das3r_amd import GaussianRasterizer
    kw = _leaves(dev, names)
    extra = [v for v in call.values() if torch.is_tensor(v) and v.requires_grad]
    r = GaussianRasterizer(_settings(dev, **(settings or {})), keep_state=keep_state)
    out = r(**kw, **call)
    if loss:
        sum((out[k] * _weight(out[k], 100 + k)).sum() for k in loss).backward()
    return [o.detach() for o in out] + [t.grad for t in list(kw.values()) + extra], r


def _features(dev, n):
    return _host()["features"][:, :n].contiguous().to(dev).requires_grad_(True)


def _no_grad(dev):
    from das3r_amd import GaussianRasterizer
    kw = _leaves(dev, ("colors_precomp",) + GEOMETRY, grad=False)
    with torch.no_grad():
        return list(GaussianRasterizer(_settings(dev))(**kw))


def _keep_state(dev):
    """keep_state=True, then the state's own calls: wider than 8 channels (a call per 8), written and accumulated"""
    from das3r_amd import alpha_of, composite_features, feature_adjoint
    res, r = _module(dev, keep_state=True)
    F = _host()["features"].to(dev)
    image = composite_features(r.state, F)
    rows = feature_adjoint(r.state, _weight(image, 7))
    acc = feature_adjoint(r.state, _weight(image, 8), out=rows.clone(), accumulate=True)
    one = feature_adjoint(r.state, _weight(image[:1], 9))
    return res + [image, rows, acc, one, alpha_of(r.state)]


def _apply_nine(dev):
    """upstream's own call of the autograd function: nine arguments, torch.Tensor([]) for what is not provided"""
    from diff_gaussian_rasterization import _RasterizeGaussians
    kw = _leaves(dev, ("colors_precomp",) + GEOMETRY)
    e = torch.Tensor([])
    color, radii = _RasterizeGaussians.apply(kw["means3D"], kw["means2D"], e, kw["colors_precomp"], kw["opacities"], kw["scales"], kw["rotations"], e,
                                             _settings(dev))
    (color * _weight(color, 100)).sum().backward()
    return [color.detach(), radii] + [t.grad for t in kw.values()]


def _tuples(dev):
    """the tuple interface as bench.py and the tools call it"""
    from das3r_amd.rasterizer import _backward_impl, _forward_full, _forward_impl, check_forward, count_live_pairs
    rs = _settings(dev)
    h = _host()
    m, col, op, sc, rot = (h[k].to(dev) for k in ("means3D", "colors_precomp", "opacities", "scales", "rotations"))
    e = torch.empty(0, device=dev)
    exact = _forward_impl(rs, m, e, col, op, sc, rot, e)
    res = _forward_full(rs, m, e, col, op, sc, rot, e, invdepth=True)
    check_forward(res[6], dev)
    live = count_live_pairs(rs, P, 0, res[0], res[3], res[4], res[5], res[6])
    bwd = _backward_impl(rs, res[0], _weight(res[1], 100), m, e, col, op, sc, rot, e, res[3], res[4], res[5], res[6], _scratch_misalign=4,
                         focal=True, focal_per_splat=True)
    return [exact[1], exact[2], res[1], res[2], res[7], torch.tensor(live)] + list(bwd)


def _empty_cloud(dev):
    from das3r_amd import GaussianRasterizer
    z = lambda n: torch.zeros(0, n, device=dev, requires_grad=True)
    kw = dict(means3D=z(3), means2D=z(3), opacities=z(1), colors_precomp=z(3), scales=z(3), rotations=z(4))
    color, radii = GaussianRasterizer(_settings(dev))(**kw)
    (color * _weight(color, 100)).sum().backward()
    return [color.detach(), radii] + [t.grad for t in kw.values()]


def _mark_visible(dev):
    from das3r_amd import GaussianRasterizer
    return [GaussianRasterizer(_settings(dev)).markVisible(_host()["means3D"].to(dev))]


CONFIGURATIONS = {
    "colors_precomp": lambda dev: _module(dev)[0],
    "shs_degree_3": lambda dev: _module(dev, ("shs",) + GEOMETRY)[0],
    "cov3D_precomp": lambda dev: _module(dev, ("colors_precomp", "means3D", "opacities", "cov3D_precomp"))[0],
    "invdepth_loss_on_both": lambda dev: _module(dev, loss=(0, 2), return_invdepth=True)[0],
    "invdepth_loss_on_colour": lambda dev: _module(dev, loss=(0,), return_invdepth=True)[0],
    "antialiasing": lambda dev: _module(dev, antialiasing=True)[0],
    "debug": lambda dev: _module(dev, settings={"debug": True})[0],
    "log_focal": lambda dev: _module(dev, log_focal=_log_focal(dev, True))[0],
    "log_focal_invdepth": lambda dev: _module(dev, loss=(0, 2), return_invdepth=True, log_focal=_log_focal(dev, True))[0],
    "log_focal_without_grad": lambda dev: _module(dev, log_focal=_log_focal(dev, False))[0],
    "no_grad": _no_grad,
    "features_3": lambda dev: _module(dev, loss=(0, 2), features=_features(dev, 3))[0],
    "features_11_alpha": lambda dev: _module(dev, loss=(0, 2), features=_features(dev, 11), return_alpha=True)[0],
    "aux_geometry_grad": lambda dev: _module(dev, loss=(0, 2, 3), features=_features(dev, 11), return_alpha=True, aux_geometry_grad=True)[0],
    "keep_state": _keep_state,
    "apply_with_nine_arguments": _apply_nine,
    "tuple_interface": _tuples,
    "empty_cloud": _empty_cloud,
    "mark_visible": _mark_visible,
}


def run(name, dev):
    """-> (trace, results) of one run of a configuration, from a library state that has learnt nothing.  With DAS3R_DETERMINISTIC=1, as
    every exact comparison of gradients in this suite: lists this short otherwise take the compositing backward that meets its waves with
    LDS float atomics, whose sums differ in the last bits from run to run by design (csrc/kernel_choice.h)."""
    from das3r_amd import _lib
    rec = _Recorder(_lib.load())
    real, before = _lib.load, os.environ.get("DAS3R_DETERMINISTIC")
    os.environ["DAS3R_DETERMINISTIC"] = "1"
    _lib.reload_switches()
    with torch.cuda.device(dev):
        _lib.forget_shapes()
    _lib.load = lambda: rec
    try:
        results = CONFIGURATIONS[name](dev)
        torch.cuda.synchronize(dev)
    finally:
        _lib.load = real
        if before is None:
            del os.environ["DAS3R_DETERMINISTIC"]
        else:
            os.environ["DAS3R_DETERMINISTIC"] = before
        _lib.reload_switches()
    return rec.calls, results


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and torch.equal(a, b))


_EXPECTED = {}


def _expected():
    if not _EXPECTED:
        with open(TRACE) as f:
            _EXPECTED.update(json.load(f))
    return _EXPECTED


def test_the_recording_covers_every_configuration():
    assert sorted(_expected()) == sorted(CONFIGURATIONS)


@pytest.mark.parametrize("name", list(CONFIGURATIONS))
def test_library_calls_are_the_recorded_ones_and_results_repeat_bit_for_bit(name):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda:0")
    first, a = run(name, dev)
    second, b = run(name, dev)
    want = _expected()[name]
    assert json.loads(json.dumps(first)) == want, f"{name}: the library calls differ from the recording"
    assert json.loads(json.dumps(second)) == want, f"{name}: the second run's library calls differ from the recording"
    assert len(a) == len(b) and len(a) > 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert _same(x, y), f"{name}: result {k} differs between two runs"
    if name == "empty_cloud":
        assert want == [], "P = 0: no library call"


if __name__ == "__main__":
    device = torch.device("cuda:0")
    traces, problems = {}, []
    for cfg in CONFIGURATIONS:
        traces[cfg], r1 = run(cfg, device)
        again, r2 = run(cfg, device)
        differ = [k for k, (x, y) in enumerate(zip(r1, r2)) if not _same(x, y)]
        if again != traces[cfg] or len(r1) != len(r2) or differ:
            problems.append(f"{cfg}: trace repeats: {again == traces[cfg]}; results {differ} of {len(r1)} do not repeat")
        print(f"{cfg}: {len(traces[cfg])} calls: " + ", ".join(c["entry"].replace("das3r_raster_", "") for c in traces[cfg]))
    os.makedirs(os.path.dirname(TRACE), exist_ok=True)
    with open(TRACE, "w") as f:
        json.dump(traces, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {TRACE}")
    if problems:
        raise SystemExit("a recording must repeat:\n" + "\n".join(problems))
