"""The arena that lays out every device workspace of libofx.so (ofighters_amd/csrc/ofx_arena.h) is plain C++: its
measuring pass, its handing-out pass, the overflow rule and the typed helpers are checked on the host, without a GPU, by
the stand-alone program tests/arena_host.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_host_program(tmp_path):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "arena_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ofighters_amd", "csrc"),
                            os.path.join(ROOT, "tests", "arena_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
