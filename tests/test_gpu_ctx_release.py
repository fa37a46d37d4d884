"""A context, and every form it prepares lazily, gives back to the HIP runtime everything it took.

tests/cpp/test_ctx_release.cpp is a host program linked against the built libss_hip.so that defines the runtime's allocation and
release calls itself, keeps a ledger of what is live and drives the C-ABI phase by phase (its header has the list).  It is built
the way tests/test_host_common.py builds its program and run ONCE, as a child process under a time limit of its own; the tests
below read its output per phase.  A phase whose form stepped aside fails there, it does not pass empty.

The failed creations: for each create entry point and every k, the k-th allocation of the creation is refused (the runtime is not
called).  Create must return null with a message, keep nothing, and the next create must succeed.  The (entry, k, message) list is
pinned to tests/golden/create_failures_parent.json, recorded from the commit before the owners (host_common.h: Holdings) were
introduced: it fixes the allocation order of creation and the texts.
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-solvers_amd")
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

PHASES = ["homotopy_f32_1000x512", "homotopy_f32_256x16896_early", "homotopy_f32_reserved_never_formed", "homotopy_f64_256x8192_screened",
          "records_f32", "records_f64", "irls_f32", "irls_f64", "colshard_f32", "colshard_f64"]
CREATES = ["homotopy_create_f32", "homotopy_create_f64", "irls_create_f32", "irls_create_f64"]


def build_program(out_dir):
    """-> the path of the built program (the compiler and the target of build.py, linked against the built library)"""
    spec = importlib.util.spec_from_file_location("ss_amd_build", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert os.path.exists(os.path.join(build.LIB, "libss_hip.so")), "build the library first (__graft_entry__.build)"
    exe = os.path.join(str(out_dir), "test_ctx_release")
    cmd = [build.HIPCC, "--offload-arch=" + build.ARCH, "-x", "hip", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-comment",
           "-I", build.INCLUDE, os.path.join(ROOT, "tests", "cpp", "test_ctx_release.cpp"), "-o", exe,
           "-rdynamic", "-L", build.LIB, "-lss_hip", "-ldl", "-lpthread", "-Wl,-rpath," + build.LIB]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    exe = build_program(tmp_path_factory.mktemp("ctx_release"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode in (0, 1), r.stdout          # (1: a phase failed — the tests below say which)
    return r.stdout


def _phase_lines(output):
    return {m.group(1): m.group(2) for m in re.finditer(r"^PHASE (\S+) (ok|FAILED: .*)$", output, flags=re.M)}


def test_every_phase_ran(program_output):
    assert sorted(_phase_lines(program_output)) == sorted(PHASES + CREATES), program_output


@pytest.mark.parametrize("phase", PHASES)
def test_context_returns_everything(program_output, phase):
    assert _phase_lines(program_output).get(phase) == "ok", program_output


@pytest.mark.parametrize("entry", CREATES)
def test_failed_creation_keeps_nothing(program_output, entry):
    assert _phase_lines(program_output).get(entry) == "ok", program_output


def test_failed_creations_report_what_the_parent_reported(program_output):
    got = [[e, int(k), msg] for e, k, msg in re.findall(r"^CREATE_FAIL (\S+) (\d+) (.*)$", program_output, flags=re.M)]
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "create_failures_parent.json")))
    assert want and sorted({e for e, _, _ in want}) == sorted(CREATES)
    assert got == want
