"""The host <-> device hand-off protocol of a forward (das3r_amd/csrc/mailbox.h: tags, check slots, the examination of a self-check word,
the emission ring's rule) without a GPU: the header compiles alone with a host compiler, and tests/mailbox_host_main.cpp — a stand-alone
program that includes nothing else — drives it over plain memory under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "das3r_amd", "csrc", "mailbox.h")
GXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not installed")


def test_mailbox_header_compiles_alone():
    r = subprocess.run([GXX, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", "-include", HEADER, os.devnull],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(HEADER).read()
    assert "#include <hip" not in text and '#include "' not in text, "pure host arithmetic: no HIP, no other header of the library"


def test_mailbox_protocol_over_plain_memory(tmp_path):
    exe = str(tmp_path / "mailbox_host")
    b = subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "mailbox_host_main.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
