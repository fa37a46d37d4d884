"""The option surface of a context (ss_hip_set_option / ss_hip_get_option, include/ss_hip.h): every key reads back its
default on a fresh context, a written value reads back normalised (flag, clamp, floor, snap, as given), `ro_slots` rejects
what it does not accept, retired and unknown keys are SS_HIP_EINVAL at both entry points, and the header's option list names
exactly the keys that exist.  No solve is run.  The defaults and the expected read-backs are literals: what the context
stated and what the per-key dispatcher stored before both entry points walked one table."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

EINVAL = 1          # SS_HIP_EINVAL

# key: (default, [(written, read back), ...]) — one value in range first; where values are clamped or snapped, one on each side
FLAG = [(1, 1), (0, 0), (7, 1), (-3, 1)]
OPTIONS = {
    "sweep_variant":         (5, [(3, 3), (11, 11), (-1, -1)]),                 # as given (the launcher maps what it does not know to 0)
    "lookahead":             (4, [(2, 2), (0, 0)]),
    "strict_sign":           (0, FLAG),
    "screen_first8":         (1, FLAG),
    "screen_rescue":         (1, FLAG),
    "trace":                 (0, FLAG),
    "zero_on_removal":       (0, FLAG),
    "tie_guard":             (0, FLAG),
    "profile_every":         (1, [(4, 4), (0, 1), (-5, 1)]),
    "profile_solve_every":   (1, [(4, 4), (0, 1), (-5, 1)]),
    "engine":                (1, [(2, 2), (-1, 0), (9, 3)]),
    "tie_rerun":             (1, FLAG),
    "ro_force_resweep":      (0, FLAG),
    "ro_staged":             (1, FLAG),
    "batch_subset":          (1, FLAG),
    "ro_slots":              (8, [(4, 4), (1, 1), (8, 8)]),
    "batch_fused_scan":      (1, FLAG),
    "sweep32_variant":       (0, [(7, 7), (-1, 0), (12, 9)]),
    "first_sweep_cols":      (32, [(64, 64), (32, 32), (33, 64), (0, 32), (100, 64)]),
    "early_solo":            (1, FLAG),
    "early_pass":            (2, [(0, 0), (2, 2)]),
    "early_adapt":           (1, FLAG),
    "early_se":              (1, [(2, 2), (-1, 0), (5, 3)]),
    "la_fused":              (3, [(1, 1), (-1, 0), (4, 3)]),
    "solo_subset":           (256, [(12, 12), (-1, 0), (300, 256)]),
    "solo_full_gram":        (0, FLAG),
    "cache_mib":             (2048, [(64, 64), (3, 16), (1 << 33, 1 << 33)]),   # (a long: not cut to 32 bits)
    "batch_min":             (192, [(4, 4), (1, 2), (-7, 2)]),
    "batch_gram_min":        (512, [(100, 100), (-1, 0)]),
    "batch_cols_min":        (24, [(8, 8), (-1, 0)]),
    "gram_full_gib":         (64, [(8, 8), (-2, 0)]),
    "gram_full_after":       (0, [(5, 5), (-1, 0)]),
    "gram_single":           (1, FLAG),
    "gram_symmetric":        (1, FLAG),
    "batch_chunk":           (4096, [(64, 64), (1, 4)]),
    "irls_batch_max":        (256, [(8, 8), (0, 1), (70000, 65535)]),
    "dl_chunk_max":          (0, [(5, 5), (-1, 0), (40000, 32768)]),
    "screen_single":         (1, [(2, 2), (-1, 0), (3, 2)]),
    "screen_first16":        (1, FLAG),
    "batch_screen":          (1, FLAG),
    "screen_resident":       (1, FLAG),
    "screen_recheck":        (1, FLAG),
    "gram_reserve":          (1, FLAG),
    "colshard_fail_prepare": (0, FLAG),
}
WRITE_ONLY = ["pass_dbg_ptr"]       # an action (a device pointer): not written here
RETIRED = ["cq_cols", "cq_rows", "cq_vec4", "scan_blocks", "temporal_cols", "sweep_cols_f64", "sweep_cols_f64_late",
           "sweep_f64_variant", "early_probe", "batch_cols_max", "dbg_ndone", "dbg_skip_sum"]
UNKNOWN = RETIRED + ["no_such_option"]


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def matrices():
    rng = np.random.default_rng(64256)
    A = rng.standard_normal((64, 256)) / 8.0
    return {np.float32: A.astype(np.float32), np.float64: A}


@pytest.fixture
def no_env(monkeypatch):
    monkeypatch.delenv("SS_HIP_SCREEN_SINGLE", raising=False)     # (the initial value of "screen_single" when set)


def _raw_set(sship, h, key, value):
    return sship.lib().ss_hip_set_option(h._h, key.encode(), int(value))


def _raw_get(sship, h, key):
    v = ctypes.c_long(-12345)
    return sship.lib().ss_hip_get_option(h._h, key.encode(), ctypes.byref(v)), int(v.value)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fresh_context_reads_back_the_defaults(sship, matrices, no_env, dtype):
    with sship.Homotopy(matrices[dtype]) as h:
        got = {key: h.get_option(key) for key in OPTIONS}
    assert got == {key: default for key, (default, _) in OPTIONS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_written_values_read_back_normalised(sship, matrices, no_env, dtype):
    with sship.Homotopy(matrices[dtype]) as h:
        for key, (_, probes) in OPTIONS.items():
            for written, expected in probes:
                h.set_option(key, written)
                assert h.get_option(key) == expected, (key, written)
        # nothing written above leaked into another key: every key still holds its last probe
        for key, (_, probes) in OPTIONS.items():
            assert h.get_option(key) == probes[-1][1], key


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ro_slots_rejects_instead_of_clamping(sship, matrices, dtype):
    with sship.Homotopy(matrices[dtype]) as h:
        h.set_option("ro_slots", 3)
        for bad in (0, 9, -1):
            assert _raw_set(sship, h, "ro_slots", bad) == EINVAL
            assert h.get_option("ro_slots") == 3
            with pytest.raises(sship.SsHipError):
                h.set_option("ro_slots", bad)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_retired_and_unknown_keys_are_invalid(sship, matrices, dtype):
    with sship.Homotopy(matrices[dtype]) as h:
        for key in UNKNOWN:
            for value in (0, 1, 16):
                assert _raw_set(sship, h, key, value) == EINVAL, key
            rc, v = _raw_get(sship, h, key)
            assert rc == EINVAL and v == -12345, key
            with pytest.raises(sship.SsHipError) as e:
                h.set_option(key, 1)
            assert e.value.code == EINVAL
            with pytest.raises(sship.SsHipError) as e:
                h.get_option(key)
            assert e.value.code == EINVAL
        for key in WRITE_ONLY:
            rc, v = _raw_get(sship, h, key)
            assert rc == EINVAL and v == -12345, key
        assert _raw_set(sship, h, "pass_dbg_ptr", 0) == 0          # (0 = off: the one value that needs no buffer)


def test_the_header_lists_the_keys_that_exist():
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    missing = [key for key in list(OPTIONS) + WRITE_ONLY if '"%s"' % key not in hdr]
    assert not missing, "options without a line in include/ss_hip.h: %s" % missing
    stale = [key for key in RETIRED if key in hdr]
    assert not stale, "retired options still named in include/ss_hip.h: %s" % stale


def test_the_table_holds_the_keys_that_exist():
    """the rows of kOptions (csrc/homotopy.hip) are exactly the keys above: a key added to the table is added here"""
    import re
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    body = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    keys = re.findall(r'^\s*\{ "([a-z0-9_]+)",', body, flags=re.M)
    assert sorted(keys) == sorted(list(OPTIONS) + WRITE_ONLY) and len(set(keys)) == len(keys)
