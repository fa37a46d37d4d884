"""The host driver and the selection kernel of the four top-correlation calls stay single (sparse-solvers_amd/csrc/tc_driver.h,
tc_select.h): top_correlations, nonneg_top_correlations, weighted_top_correlations and group_top_correlations go through one
driver, one record check, one residual block, one arena and — the three whose row is a signal — one selection kernel.  A variant
that pastes the driver or the kernel once more fails here.  Source-level: counts over csrc/*.hip and *.h, comments left out.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-solvers_amd", "csrc")


def _sources():
    """csrc's units and headers without their // comments (which may name what the code must not hold)"""
    return {name: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
            for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}


def _calls(fn):
    """'file:line' of every call of `fn` (with or without template arguments): a use that is no declaration, definition or
    explicit instantiation — those have the return type in front of the name on their line"""
    hits = []
    for name, text in _sources().items():
        for m in re.finditer(r"\b%s\s*(?:<[^<>()]*>)?\s*\(" % re.escape(fn), text):
            line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
            if "hipError_t" not in line:
                hits.append("%s:%d" % (name, text.count("\n", 0, m.start()) + 1))
    return hits


def _kernels(text):
    """(name, body) of every __global__ function of `text`, the body by matching braces"""
    out = []
    for m in re.finditer(r"__global__", text):
        head = re.compile(r"void\s+(\w+)\s*\(").search(text, m.end())
        open_ = text.index("{", head.end())
        depth, pos = 1, open_ + 1
        while depth:
            depth += {"{": 1, "}": -1}.get(text[pos], 0)
            pos += 1
        out.append((head.group(1), text[open_:pos]))
    return out


def test_the_record_check_and_the_residual_block_are_launched_in_one_place():
    for fn in ("tc_launch_record_check", "tc_launch_residual_block"):
        hits = _calls(fn)
        assert len(hits) == 1 and hits[0].startswith("tc_driver.h:"), (fn, hits)


def test_the_workspace_message_is_stated_once():
    # (ksvd.hip's message names its own workspace and is another text)
    hits = [name for name, text in _sources().items() if name != "ksvd.hip"
            for _ in re.finditer(r"no device memory for a workspace of", text)]
    assert hits == ["tc_driver.h"], hits


def test_at_most_two_kernels_select():
    callers = [(name, k) for name, text in _sources().items() for k, body in _kernels(text) if "tc_select_sorted(" in body]
    assert sorted(callers) == [("joint.hip", "k_js_select"), ("tc_select.h", "k_tc_select")], callers


def test_the_copies_are_gone():
    every = "\n".join(open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h")))
    for gone in ("k_w_norms", "k_nn_select", "k_w_select", "nn_grow", "wt_grow", "js_grow", "NonnegState", "nonneg_free"):
        assert gone not in every, gone
    # the quiet NaN that strikes a column out is one function
    assert len(re.findall(r"__int_as_float\(0x7fc00000\)", "\n".join(
        _sources()[f] for f in ("topcorr.hip", "nonneg.hip", "weighted.hip", "joint.hip", "tc_select.h", "tc_driver.h")))) == 1


def test_the_four_calls_share_one_arena():
    src = _sources()
    # the context holds no arena of the non-negative call, the weighted state holds the staged weights alone
    assert not re.search(r"void\*\s+nn\b", src["ss_hip_internal.h"])
    state = re.search(r"struct WeightedState \{(.*?)\};", src["weighted.hip"], re.S).group(1)
    assert re.findall(r"\b(\w+)\s*=", state) == ["wbuf", "wbuf_bytes"], state
    # one way to the arena, asked by the driver, the record extension and the offsets' staging of the group call
    assert len(re.findall(r"ctx->tc\b", "\n".join(src.values()))) == len(re.findall(r"ctx->tc\b", src["topcorr.hip"]))
    assert "topcorr_arena(ctx)" in src["tc_driver.h"] and "topcorr_arena(ctx)" in src["joint.hip"]
