"""The triangular tile decode of the symmetric Gram build (sparse-solvers_amd/csrc/tri_decode.h), on the host.

k_gemm_tn_f32<SYM> (csrc/gemm.hip) turns blockIdx.x into a tile pair with a float square root and two correcting loops; the
launcher admits up to 2^31 - 1 blocks, far beyond what a GPU test can build (2 000 tiles are a 260 k-column dictionary).
tests/cpp/test_tri_decode.cpp calls the same function for every panel boundary below 2^31 and for every block below 2^22 and
compares with the integer definition.  It is built with the compiler and the target build.py uses and launches no kernel.
"""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-solvers_amd")


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("ss_amd_build", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path_factory.mktemp("tri_decode") / "test_tri_decode")
    cmd = [build.HIPCC, "--offload-arch=" + build.ARCH, "-x", "hip", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-comment",
           "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_tri_decode.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_host_program_passes(program_output):
    assert "all checks passed" in program_output, program_output
    assert "FAILED" not in program_output, program_output


def test_it_checked_what_it_says(program_output):
    # panels 0 .. 65535: three blocks each where below 2^31 (t = 0 has no block before its first), plus block 2^31 - 1
    want = 1
    for t in range(65536):
        first = t * (t + 1) // 2
        want += (t > 0 and first - 1 < 2 ** 31) + (first < 2 ** 31) + (first + t < 2 ** 31)
    assert int(re.search(r"^boundaries checked (\d+)$", program_output, flags=re.M).group(1)) == want
    assert int(re.search(r"^sweep checked (\d+)$", program_output, flags=re.M).group(1)) == 2 ** 22


def test_the_kernel_calls_the_header():
    src = open(os.path.join(PKG, "csrc", "gemm.hip")).read()
    assert '#include "tri_decode.h"' in src
    assert re.search(r"\btri_tile_decode\s*\(\s*blockIdx\.x\s*,\s*bm\s*,\s*bn\s*\)", src)
    assert "__fsqrt_rn" not in src, "a second copy of the decode in gemm.hip"
