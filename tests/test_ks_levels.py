"""The level schedule of the K-SVD sweep (sparse-solvers_amd/csrc/ks_levels.h), on the host.

ss_hip_homotopy_ksvd_sweep_* is defined as sequential over the requested atoms and runs them level by level: atoms that share no signal
commute exactly, so the schedule may only put two atoms in one level when they share none.  tests/cpp/test_ks_levels.cpp generates
random atom -> user lists and checks that
  * every pair of atoms that shares a signal sits in different levels, in `cols` order;
  * every atom's level is the smallest that allows this (1 + the largest level of an earlier atom it shares a signal with);
  * atoms without users take level 1;
  * the serial flag gives s + 1;
and that the (level, s) order is a permutation with the levels' ranges.  It is built with the compiler and the target build.py uses,
once plainly and once with the host sanitizers (address, undefined) linked in, and launches no kernel.
"""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-solvers_amd")


def _build_and_run(tmp, name, extra):
    spec = importlib.util.spec_from_file_location("ss_amd_build", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp / name)
    cmd = [build.HIPCC, "--offload-arch=" + build.ARCH] + extra + ["-x", "hip", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-comment",
           "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_ks_levels.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("ks_levels"), "test_ks_levels", [])


def test_host_program_passes(program_output):
    assert "all checks passed" in program_output, program_output
    assert "FAILED" not in program_output, program_output


def test_it_checked_what_it_says(program_output):
    def count(what):
        return int(re.search(r"^%s (\d+)$" % what, program_output, flags=re.M).group(1))
    assert count("cases checked") == 8 * 5 * 2
    assert count("atoms checked") == 2 * 5 * (0 + 1 + 1 + 7 + 40 + 200 + 64 + 150)
    assert count("sharing pairs checked") > 10000 and count("atoms without users") > 100


def test_host_program_passes_with_the_host_sanitizers(tmp_path_factory):
    """the same program with -fsanitize=address,undefined on its host code (the header is host code), run directly"""
    out = _build_and_run(tmp_path_factory.mktemp("ks_levels_san"), "test_ks_levels_san", ["-Xarch_host", "-fsanitize=address,undefined"])
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out, out


def test_the_sweep_calls_the_header():
    src = open(os.path.join(PKG, "csrc", "ksvd.hip")).read()
    assert '#include "ks_levels.h"' in src
    assert re.search(r"\bks_levels\s*\(", src) and re.search(r"\bks_order\s*\(", src) and re.search(r"\bks_first_duplicate\s*\(", src)
    hdr = open(os.path.join(PKG, "csrc", "ks_levels.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|\bhip[A-Z]\w*|__device__|__global__", hdr), "ks_levels.h must stay plain C++ (no HIP types)"
