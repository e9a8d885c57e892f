"""CPU tests of das3r_amd/csrc/preprocess_choice.h: which form of preprocess_backward_kernel a backward launches
(choose_preprocess_backward), why a chained call is refused, the forward's rule for staging its SH rows, and the raw name a launch is
recorded under.  das3r_debug_choose_preprocess_backward / das3r_debug_preprocess_backward_name run the header's functions on the values the
test passes.  The expected forms are written out by hand from the rules (the kernel's comments in preprocess_bwd.hip), not
recorded from the code; tests/preprocess_choice_host_main.cpp walks every combination of the inputs under AddressSanitizer and UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "das3r_amd", "csrc", "preprocess_choice.h")
GXX = shutil.which("g++")
needs_gxx = pytest.mark.skipif(GXX is None, reason="g++ not installed")

ORDER = ("has_sh", "has_cov", "stage_in", "stage_out", "deg0", "chain", "depth", "jac", "aa")   # the kernel's template arguments


def choose(lib, **kw):
    """-> (refusal, form as a dict, base index, the forward's staging rule) for the inputs given; the rest are the plain case: SH rows with
    M = 16 at degree 3, both tensors aligned, nothing else."""
    from das3r_amd import _lib
    v = dict(has_sh=1, has_cov=0, M=16, sh_degree=3, shs_aligned16=1, dL_dshs_aligned16=1, no_sh_stage=0, jac_saved=0, chained=0, quad_rows=0,
             depth=0, aa=0)
    assert set(kw) <= set(v)
    v.update(kw)
    i = _lib.PreprocessBackwardInputs(**{k: int(x) for k, x in v.items()})
    out = _lib.PreprocessForm()
    why = lib.das3r_debug_choose_preprocess_backward(C.byref(i), C.byref(out))
    return why, {n: getattr(out, n) for n in ORDER}, out.base_index, out.sh_rows_staged


def form(text, depth=0, aa=0):
    """'sh cov stage_in stage_out deg0 chain jac' -> the form as a dict; words left out are 0."""
    words = text.split()
    assert set(words) <= {"sh", "cov", "stage_in", "stage_out", "deg0", "chain", "jac"}, text
    f = {n: 0 for n in ORDER}
    for w in words:
        f[{"sh": "has_sh", "cov": "has_cov"}.get(w, w)] = 1
    f["depth"], f["aa"] = depth, aa
    return f


def name_of(lib, f):
    from das3r_amd import _lib
    n = lib.das3r_debug_preprocess_backward_name(C.byref(_lib.PreprocessForm(**f)))
    return None if n is None else n.decode()


# Every row of the rule.  Unstaged SH layouts: M != 16, or dL_dshs off a 16-byte boundary, or DAS3R_NO_SH_STAGE.
#   (inputs, expected form, position of the base form in the header's list)
TABLE = [
    # a chained call: SH rows in an unstaged layout, scales + rotations; degree 0 first, then the Jacobian planes, then the rows
    (dict(chained=1, M=9, sh_degree=0), "sh deg0 chain", 0),
    (dict(chained=1, M=9, sh_degree=0, jac_saved=1), "sh deg0 chain", 0),
    (dict(chained=1, M=9, sh_degree=2, jac_saved=1), "sh chain jac", 1),
    (dict(chained=1, M=16, sh_degree=3, jac_saved=1, dL_dshs_aligned16=0), "sh chain jac", 1),
    (dict(chained=1, M=9, sh_degree=2), "sh chain", 2),
    (dict(chained=1, M=4, sh_degree=1), "sh chain", 2),
    (dict(chained=1, M=16, sh_degree=3, no_sh_stage=1), "sh chain", 2),
    # the forward left the Jacobian planes: they replace the SH input row, whatever the degree; dL_dsh rows through LDS at M = 16
    (dict(jac_saved=1, has_cov=1), "sh cov stage_out jac", 3),
    (dict(jac_saved=1, has_cov=1, M=9, sh_degree=2), "sh cov jac", 4),
    (dict(jac_saved=1, has_cov=1, dL_dshs_aligned16=0), "sh cov jac", 4),
    (dict(jac_saved=1), "sh stage_out jac", 5),
    (dict(jac_saved=1, shs_aligned16=0), "sh stage_out jac", 5),
    (dict(jac_saved=1, M=9, sh_degree=2), "sh jac", 6),
    (dict(jac_saved=1, no_sh_stage=1), "sh jac", 6),
    # SH rows, scales + rotations: rows in and out through LDS; out only; degree 0; plain
    (dict(), "sh stage_in stage_out", 7),
    (dict(sh_degree=2), "sh stage_in stage_out", 7),
    (dict(sh_degree=1), "sh stage_out", 8),
    (dict(sh_degree=0), "sh stage_out", 8),               # (the staged forms have no degree-0 variant)
    (dict(shs_aligned16=0), "sh stage_out", 8),
    (dict(M=9, sh_degree=0), "sh deg0", 9),
    (dict(M=1, sh_degree=0), "sh deg0", 9),
    (dict(sh_degree=0, dL_dshs_aligned16=0), "sh deg0", 9),
    (dict(M=9, sh_degree=2), "sh", 10),
    (dict(dL_dshs_aligned16=0), "sh", 10),
    (dict(no_sh_stage=1), "sh", 10),
    # the same four with cov3D
    (dict(has_cov=1), "sh cov stage_in stage_out", 11),
    (dict(has_cov=1, sh_degree=1), "sh cov stage_out", 12),
    (dict(has_cov=1, shs_aligned16=0), "sh cov stage_out", 12),
    (dict(has_cov=1, M=4, sh_degree=0), "sh cov deg0", 13),
    (dict(has_cov=1, M=4, sh_degree=1), "sh cov", 14),
    (dict(has_cov=1, no_sh_stage=1), "sh cov", 14),
    # precomputed colours: nothing about SH matters
    (dict(has_sh=0), "", 15),
    (dict(has_sh=0, jac_saved=1, sh_degree=0), "", 15),
    (dict(has_sh=0, has_cov=1), "cov", 16),
    (dict(has_sh=0, has_cov=1, jac_saved=1, sh_degree=0), "cov", 16),
]


@pytest.mark.parametrize("depth,aa", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_every_row_of_the_rule(hip_lib, depth, aa):
    for inputs, text, index in TABLE:
        why, got, base, _staged = choose(hip_lib, depth=depth, aa=aa, **inputs)
        assert why == 0, inputs
        assert got == form(text, depth, aa), inputs
        assert base == index, inputs
    assert sorted({index for _i, _t, index in TABLE}) == list(range(17)), "the table reaches every instantiated base form"


def test_why_a_chained_call_is_refused(hip_lib):
    ok = dict(chained=1, M=9, sh_degree=2)
    assert choose(hip_lib, **ok)[0] == 0
    assert choose(hip_lib, **ok, has_sh=0)[0] == 1, "precomputed colours"
    assert choose(hip_lib, **ok, has_cov=1)[0] == 2, "cov3D: no scales + rotations to chain through"
    assert choose(hip_lib, chained=1)[0] == 3, "M = 16, aligned: the dL_dsh rows would leave through LDS"
    assert choose(hip_lib, chained=1, sh_degree=0)[0] == 3, "... at every degree"
    assert choose(hip_lib, **ok, quad_rows=1)[0] == 4, "quadrant rows"
    assert choose(hip_lib, **ok, has_sh=0, has_cov=1, quad_rows=1)[0] == 1, "the first reason that applies"
    assert choose(hip_lib, chained=1, dL_dshs_aligned16=0)[0] == 0 and choose(hip_lib, chained=1, no_sh_stage=1)[0] == 0
    assert choose(hip_lib, has_cov=1, quad_rows=1)[0] == 0, "not chained: nothing to refuse"


def test_the_forwards_staging_rule(hip_lib):
    """preprocess_kernel<.., STAGE> / sh_colour_kernel<STAGE>: M == 16, degree >= 2, aligned rows, no DAS3R_NO_SH_STAGE."""
    assert choose(hip_lib)[3] == 1
    assert choose(hip_lib, sh_degree=2)[3] == 1
    for off in (dict(has_sh=0), dict(M=9), dict(M=15), dict(sh_degree=1), dict(sh_degree=0), dict(shs_aligned16=0), dict(no_sh_stage=1)):
        assert choose(hip_lib, **off)[3] == 0, off
    # what the gradient tensor looks like, the saved Jacobian, cov3D, depth: not the forward's business
    assert choose(hip_lib, dL_dshs_aligned16=0, jac_saved=1, has_cov=1, depth=1, aa=1)[3] == 1


def test_raw_names_are_the_launch_sites_text(hip_lib):
    """The names tests/test_gpu_forward_flows.py expects and docs/ledger.md (ci) lists, as das3r_profile_report gives them (less the
    parentheses _lib.profile_report strips)."""
    pinned = {
        ("sh stage_out jac", 0, 0): "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>",
        ("sh stage_out jac", 1, 0): "preprocess_backward_kernel<true, false, false, true, false, false, true, true, false>",
        ("sh deg0 chain", 0, 0): "preprocess_backward_kernel<true, false, false, false, true, true, false, false, false>",
        ("sh stage_out", 0, 0): "preprocess_backward_kernel<true, false, false, true, false, false, false, false, false>",
        ("cov", 1, 1): "preprocess_backward_kernel<false, true, false, false, false, false, true, false, true>",
    }
    for (text, depth, aa), name in pinned.items():
        assert name_of(hip_lib, form(text, depth, aa)) == "(" + name + ")"
    src = open(os.path.join(ROOT, "tests", "test_gpu_forward_flows.py")).read()
    for name in list(pinned.values())[:2] + [list(pinned.values())[3]]:
        assert '"' + name + '"' in src, name
    assert name_of(hip_lib, form("stage_in stage_out")) is None, "not instantiated: no name"
    assert name_of(hip_lib, form("sh deg0 jac")) is None
    # every form the table chooses has a name that spells the form
    for inputs, _text, _index in TABLE:
        _why, got, _base, _staged = choose(hip_lib, **inputs)
        flags = ", ".join("true" if got[n] else "false" for n in ORDER)
        assert name_of(hip_lib, got) == f"(preprocess_backward_kernel<{flags}>)"


@needs_gxx
def test_header_compiles_alone():
    r = subprocess.run([GXX, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", "-include", HEADER, os.devnull],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(HEADER).read()
    assert "#include" not in text, "pure host arithmetic: no HIP, no other header"
    assert "switches()" not in text.split("namespace das3r")[1] and "set_error" not in text.split("namespace das3r")[1]


@needs_gxx
def test_every_combination_of_the_inputs(tmp_path):
    exe = str(tmp_path / "preprocess_choice_host")
    b = subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "preprocess_choice_host_main.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
