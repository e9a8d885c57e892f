"""CPU tests of the split preprocess (geometry kernel on the caller's stream, SH colour kernel on the library's side stream: preprocess.hip,
forward.hip): the DAS3R_SPLIT_COLOUR switch is parsed, the choice between the split and the fused form is a pure function of the call's shape,
the ABI did not move, and the per-kernel table folds the two new kernel names into the preprocess entry."""
import ctypes

import pytest


def test_switch_parsing(hip_lib, monkeypatch):
    from das3r_amd import _lib
    monkeypatch.delenv("DAS3R_SPLIT_COLOUR", raising=False)
    assert _lib.split_colour_switch() == 0
    for text, want in (("0", -1), ("1", 1), ("", 0), ("yes", 0)):
        monkeypatch.setenv("DAS3R_SPLIT_COLOUR", text)
        assert _lib.split_colour_switch() == want, text
    monkeypatch.delenv("DAS3R_SPLIT_COLOUR")
    assert _lib.split_colour_switch() == 0


GLOBAL_SORT, OWN_CHAIN, FUSED_EMIT = 0, 1, 2


def test_the_rule_is_a_function_of_the_shape_alone(hip_lib):
    from das3r_amd import _lib
    rule = _lib.split_colour_rule
    big, small = 1_000_000, 100_000
    # by shape (switch unset): SH at an active degree >= 2, a large scene, a binning chain of its own
    for D in range(4):
        assert rule(True, D, big, OWN_CHAIN, forced=0) == (D >= 2)
    assert rule(True, 3, 1 << 18, OWN_CHAIN, forced=0) and not rule(True, 3, (1 << 18) - 1, OWN_CHAIN, forced=0)
    assert not rule(True, 3, small, OWN_CHAIN, forced=0)
    assert not rule(False, 3, big, OWN_CHAIN, forced=0), "precomputed colours take the fused kernel"
    assert not rule(True, 3, big, OWN_CHAIN, forced=0, no_backward=True), "an evaluation forward takes the fused kernel"
    assert rule(True, 3, small, OWN_CHAIN, forced=1, no_backward=True) and not rule(True, 3, big, OWN_CHAIN, forced=-1, no_backward=True)
    for path in (GLOBAL_SORT, FUSED_EMIT):
        for forced in (0, 1):
            assert not rule(True, 3, big, path, forced=forced), "the global sort scatters the depth keys; the fused emission has no chain"
    # forced off: never; forced on: wherever the split form can run (SH, degree >= 1), whatever the size
    for D in range(4):
        for P in (1, small, big):
            assert not rule(True, D, P, OWN_CHAIN, forced=-1)
            assert rule(True, D, P, OWN_CHAIN, forced=1) == (D >= 1)
    assert not rule(False, 0, big, OWN_CHAIN, forced=1) and not rule(True, 0, big, OWN_CHAIN, forced=1)
    # the same question twice gives the same answer (no hidden state), and P == 0 has nothing to split
    assert [rule(True, 3, big, OWN_CHAIN, forced=0) for _ in range(3)] == [True] * 3
    assert not rule(True, 3, 0, OWN_CHAIN, forced=1)


def test_rule_follows_the_switch_when_not_told(hip_lib, monkeypatch):
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_SPLIT_COLOUR", "0")
    assert not _lib.split_colour_rule(True, 3, 1_000_000, OWN_CHAIN)
    monkeypatch.setenv("DAS3R_SPLIT_COLOUR", "1")
    assert _lib.split_colour_rule(True, 1, 1000, OWN_CHAIN)
    monkeypatch.delenv("DAS3R_SPLIT_COLOUR")
    assert _lib.split_colour_rule(True, 3, 1_000_000, OWN_CHAIN) and not _lib.split_colour_rule(True, 1, 1000, OWN_CHAIN)


def test_abi_number_and_struct_sizes_unchanged(hip_lib):
    from das3r_amd import _lib
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.RasterArgs) == 80 and ctypes.sizeof(_lib.RasterIn) == 64 and ctypes.sizeof(_lib.RasterOut) == 24
    assert ctypes.sizeof(_lib.RasterSaved) == 56 and _lib.RasterSaved.flags.offset == 52
    assert ctypes.sizeof(_lib.RasterGrads) == 80 and ctypes.sizeof(_lib.PreTransform) == 72
    assert ctypes.sizeof(_lib.RasterLayout) == 16 * ctypes.sizeof(ctypes.c_size_t)
    # the geometry buffer's layout is the same with either form: records of 64 bytes, rgb + depth in bytes 32 - 47
    L = _lib.layout(1000, 5000, 1920, 1080)
    assert L["splat_stride"] == 64 and L["rgbd"] == L["xy"] + 32


def test_roofline_folds_the_split_kernels_into_the_preprocess_entry():
    from das3r_amd import roofline
    report = {"preprocess_geometry_kernel": (10, 0.25), "sh_colour_kernel": (10, 0.5), "preprocess_kernel": (2, 0.125),
              "scan_emit_kernel": (10, 0.375), "onesweep_pass_kernel": (20, 0.625), "render_forward_rows_kernel": (10, 2.0)}
    g = roofline.group_kernel_times(report)
    assert g["preprocess_kernel"] == (22, pytest.approx(0.875))
    assert g["binning"] == (30, pytest.approx(1.0)) and g["render_forward_kernel"] == (10, pytest.approx(2.0))
    assert "sh_colour_kernel" not in g and "preprocess_geometry_kernel" not in g
    per_kernel, _, _ = roofline.algorithmic_bytes(1_000_000, 3, 16, 30_000_000, 1920, 1080)
    assert set(g) <= set(per_kernel), "every folded name has algorithmic bytes in the table"
