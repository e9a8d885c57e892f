"""The format of a forward's three buffers (das3r_amd/csrc/buffers.h: Layout, the field table, the typed view the launchers take) without a
GPU: the header compiles with a host compiler given float4 and uint2, and tests/buffers_host_main.cpp — a stand-alone program — checks every
accessor and derived convention over fake buffers under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "das3r_amd", "csrc", "buffers.h")
GXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not installed")


def test_buffers_header_is_pure_host_code(tmp_path):
    src = tmp_path / "includer.cpp"
    src.write_text('struct float4 { float x, y, z, w; };\nstruct uint2 { unsigned x, y; };\n#include "%s"\n' % HEADER)
    r = subprocess.run([GXX, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "#include <hip" not in open(HEADER).read(), "pure host code: no HIP"


def test_buffer_format_over_fake_bases(tmp_path):
    exe = str(tmp_path / "buffers_host")
    b = subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "buffers_host_main.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
