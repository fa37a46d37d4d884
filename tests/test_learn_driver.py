"""The host driver of the three atom learning calls stays single (sparse-solvers_amd/csrc/learn_driver.h): atom_update, ksvd_sweep
and weighted_atom_update check their arguments, fetch the atom list, carve the one arena, open and finish through the same steps,
every dictlearn.hip kernel is launched from one place, and the device helpers they share with refit.hip live in record_common.h.  A
fourth learner that pastes the driver once more fails here.  Source-level: counts over csrc/*.hip and *.h, comments left out.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
UNITS = ["dictlearn.hip", "ksvd.hip", "wdictlearn.hip"]
DRIVER = "learn_driver.h"


def _sources():
    """csrc's units and headers without their // comments (which may name what the code must not hold)"""
    return {name: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
            for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}


def _callers(fn):
    """the files that call `fn` (with or without template arguments): a use that is no declaration, definition or explicit
    instantiation — those have the return type in front of the name on their line"""
    hits = set()
    for name, text in _sources().items():
        for m in re.finditer(r"\b%s\s*(?:<[^<>()]*>)?\s*\(" % re.escape(fn), text):
            line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
            if not re.search(r"\b(hipError_t|int|template)\b", line):
                hits.add(name)
    return sorted(hits)


def test_the_atom_list_is_checked_in_one_place():
    hits = [name for name, text in _sources().items() if "adjacent_find" in text]
    assert hits == ["dictupdate.hip", DRIVER], hits


def test_the_shared_launches_are_called_from_the_driver():
    assert _callers("dl_launch_count") == [DRIVER]
    assert _callers("dl_launch_gather") == [DRIVER]
    assert _callers("replace_columns_device") == ["dictupdate.hip", DRIVER]          # (dictupdate.hip: its own entry point)
    for fn in ("dl_launch_lists", "dl_launch_objective"):
        hits = _callers(fn)
        assert hits and set(hits) <= set(UNITS + [DRIVER]), (fn, hits)


def test_every_dictlearn_kernel_is_launched_once():
    """a kernel = an instantiation: k_dl_count<false> (the counts) and k_dl_count<true> (the fill) are two"""
    src = _sources()
    text = "\n".join(src.values())
    defined = set(re.findall(r"\bvoid\s+(k_dl_\w+)\s*\(", src["dictlearn.hip"]))
    assert defined == {"k_dl_count", "k_dl_scan", "k_dl_sort", "k_dl_long", "k_dl_residual", "k_dl_atoms", "k_dl_finish",
                       "k_dl_signal_sums", "k_dl_objective", "k_dl_gather"}, defined
    launched = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(k_dl_\w+(?:<\s*(?:true|false)\s*>)?)", text)
    assert len(launched) == len(set(launched)), sorted(launched)
    assert {k.split("<")[0] for k in launched} == defined, sorted(launched)
    assert sorted(k for k in launched if "<" in k) == ["k_dl_count<false>", "k_dl_count<true>"], sorted(launched)
    # ... and all of them from dictlearn.hip
    assert not [name for name, t in src.items() if name != "dictlearn.hip" and re.search(r"hipLaunchKernelGGL\(\s*\(?\s*k_dl_", t)]


def test_the_copies_are_gone():
    every = "\n".join(open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h")))
    for gone in ("KsvdState", "WdlState", "DictLearnState", "ksvd_free", "wdictlearn_free", "dictlearn_free", "k_ks_gather", "ks_pack",
                 "wdl_pack", "wdl_lower_bound", "kWdlLeft", "kKsLeft", "kWdlNone", "kKsNone"):
        assert gone not in every, gone


def test_the_device_helpers_are_stated_once():
    src = _sources()
    # store_val: its two overloads, in record_common.h
    defs = [name for name, text in src.items() for _ in re.finditer(r"inline\s+void\s+store_val\s*\(", text)]
    assert defs == ["record_common.h", "record_common.h"], defs
    # the pack of a thread's accumulators into the vector it stores: a brace list of four consecutive elements, as float4{ a[0], a[1],
    # a[2], a[3] } or under any other name of the type
    pack = r"\{\s*(\w+(?:\[\w+\])?)\[0\],\s*\1\[1\],\s*\1\[2\],\s*\1\[3\]\s*\}"
    hits = [name for name in UNITS + [DRIVER, "record_common.h", "refit.hip"] if re.search(pack, src[name])]
    assert hits == ["record_common.h"], hits
    assert not [name for name in UNITS + [DRIVER, "refit.hip"] if re.search(r"\b(float4|double2)\s*\{", src[name])]
    # one lower bound over a list, one pair of constants
    for pat in (r"uint32_t\s+\w*lower_bound\s*\(", r"constexpr\s+uint32_t\s+k\w*None\s*=\s*0xffffffffu", r"constexpr\s+uint32_t\s+k\w*Left\s*="):
        hits = [name for name in UNITS + [DRIVER, "record_common.h"] for _ in re.finditer(pat, src[name])]
        assert hits == ["record_common.h"], (pat, hits)


def test_the_three_calls_share_one_arena():
    src = _sources()
    ctx = re.search(r"struct ss_hip_ctx \{(.*?)\n\};", src["ss_hip_internal.h"], re.S).group(1)
    for member in ("dl", "ks", "wdl"):
        assert not re.search(r"void\*\s+%s\b" % member, ctx), member
    assert re.search(r"\bPart\s+learn\b", ctx)
    # one way to the arena: the accessor (and the release beside it) in dictlearn.hip, asked by the driver and the units
    every = "\n".join(src.values())
    assert len(re.findall(r"ctx->learn\b", every)) == len(re.findall(r"ctx->learn\b", src["dictlearn.hip"]))
    assert len(re.findall(r"LearnArena&\s+learn_arena\s*\(ss_hip_ctx\*\s*ctx\)\s*\{", every)) == 1
    assert "learn_arena(" in src[DRIVER]
    for name in UNITS:
        assert "state_of" not in src[name], name
    # ... released with the context by the slot itself: no release function, nothing for the destructor to call
    assert "learn_free" not in every


def test_the_double_lambdas_are_gone():
    every = "\n".join(_sources().values())
    assert not re.search(r"\bcarve_(index|work)\b", every)
    # each unit carves through the driver, sizes included
    for name in UNITS:
        assert "Carver cv(" not in _sources()[name], name


def test_each_entry_point_checks_through_the_driver():
    src = _sources()
    for name in UNITS:
        assert len(re.findall(r"\blearn_check_args\s*\(", src[name])) == 1, name
        for step in ("learn_atoms", "learn_open", "learn_finish"):
            assert len(re.findall(r"\b%s\s*(?:<[^<>()]*>)?\s*\(" % step, src[name])) == 1, (name, step)
        assert "check_common" not in src[name] and "B * kmax must stay below" not in src[name], name
    assert len(re.findall(r"\blearn_chunk\s*\(", src["ksvd.hip"])) == 0           # (the sweep holds all residuals at once)
