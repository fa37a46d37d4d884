"""The host steps of the calls that read compact records stay single (sparse-solvers_amd/csrc/record_common.h): where the records
live on the device, the bad-record flag's read-back, a chunk's signals, the carving of a workspace into named pieces, the clauses
the entry points repeat and the release of a workspace are stated there once, and classify.hip, refit.hip, topcorr.hip, joint.hip
and the two drivers (tc_driver.h, learn_driver.h) call them.  A record call that pastes a step once more fails here.  Source-level:
counts over csrc/*.hip and *.h, comments left out.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
HOME = "record_common.h"


def _sources():
    """csrc's units and headers without their // comments (which may name what the code must not hold)"""
    return {name: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
            for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}


def _calls(fn):
    """'file:line' of every call of `fn`: a use that is no definition — those have nothing but the return type in front of the name
    on their line"""
    hits = []
    for name, text in _sources().items():
        for m in re.finditer(r"\b%s\s*(?:<[^<>()]*>)?\s*\(" % re.escape(fn), text):
            line = text[text.rfind("\n", 0, m.start()) + 1:m.start()].strip()
            if not re.fullmatch(r"(template\s*<[^()]*>\s*)?(__device__\s+)?(inline\s+)?(?!return$)[\w:<>*&]+", line):
                hits.append("%s:%d" % (name, text.count("\n", 0, m.start()) + 1))
    return hits


def _files(hits):
    return sorted({h.split(":")[0] for h in hits})


def test_the_staged_or_in_place_rule_is_stated_once():
    hits = [name for name, text in _sources().items() if re.search(r"out_dev\s*\?\s*static_cast<unsigned char\*>", text)]
    assert hits == [HOME], hits
    # ... and the four hosts of a record staging go through it
    assert _files(_calls("place.stage_in")) == ["learn_driver.h", "refit.hip", "tc_driver.h", "topcorr.hip"], _calls("place.stage_in")
    assert _files(_calls("place.copy_out")) == ["learn_driver.h", "refit.hip", "topcorr.hip"], _calls("place.copy_out")


def test_the_double_lambdas_are_gone():
    src = _sources()
    assert not [name for name, text in src.items() if re.search(r"\[\]\s*\(\s*auto\s*\.\.\.\s*\)\s*\{\s*\}", text)]
    # each call names its pieces in a struct and sizes and places it through the one helper
    for name in ("classify.hip", "refit.hip", "topcorr.hip", "joint.hip", "learn_driver.h"):
        assert "carve_into(" in src[name], name
    assert len(re.findall(r"size_t\s+carve_into\s*\(", "\n".join(src.values()))) == 1


def test_the_flag_is_read_back_in_one_place():
    src = _sources()
    # the seven calls: the residuals, the reconstruction, the refit and the top correlations' driver take the verdict of one word;
    # the extension (two words), the learners and the group offsets (a second read-back rides along) fetch; so do the weights (64 bits)
    sites = _calls("flag_fetch") + _calls("flag_verdict")
    outside = [s for s in sites if not s.startswith(HOME)]
    assert len(outside) >= 7, sites
    assert _files(outside) == ["classify.hip", "joint.hip", "learn_driver.h", "refit.hip", "tc_driver.h", "topcorr.hip", "weighted.hip"], sites
    # nobody copies a first_bad word back by hand
    by_hand = [name for name, text in src.items() if name != HOME and re.search(r"hipMemcpy\w*\(\s*&?\s*first_bad\b", text)]
    assert not by_hand, by_hand
    # armed where the check kernel is launched from the call itself (the record check and the learners' count arm inside their launch)
    assert _files(s for s in _calls("flag_arm") if not s.startswith(HOME)) == ["classify.hip", "joint.hip", "refit.hip", "topcorr.hip", "weighted.hip"]


def test_a_chunk_of_signals_is_placed_in_one_place():
    # upload_rows: through chunk_signals, and the sweep's one upload of the whole batch
    assert _files(s for s in _calls("upload_rows") if not s.startswith(HOME)) == ["ksvd.hip"], _calls("upload_rows")
    assert _files(_calls("chunk_signals")) == ["classify.hip", "dictlearn.hip", "refit.hip", "tc_driver.h", "wdictlearn.hip"], _calls("chunk_signals")


def test_each_repeated_clause_is_stated_once():
    every = "\n".join(_sources().values())
    for text in ("records_out must be 8-byte aligned", "records and records_out overlap in part", "B must stay below 2^31",
                 "r_stride must be at least num_classes"):
        assert every.count(text) == 1 and text in _sources()[HOME], text


def test_the_states_are_arenas():
    src = _sources()
    for unit, state in (("classify.hip", "ClassifyState"), ("refit.hip", "RefitState")):
        body = re.search(r"struct %s \{(.*?)\n\};" % state, src[unit], re.S).group(1)
        assert "_bytes" not in body and "WorkArena" in body, body
    # one release: the arena owns its block (host_common.h: Holdings), so no unit that holds a workspace releases it by name
    arena = re.search(r"struct WorkArena \{(.*?)\n\};", src["ss_hip_internal.h"], re.S).group(1)
    assert re.search(r"\bHoldings\s+own\b", arena), arena
    assert not _calls("arena_free")
    by_hand = [name for name in ("classify.hip", "refit.hip", "joint.hip", "topcorr.hip", "dictlearn.hip")
               if re.search(r"(hipFree|drop)\(\s*\w+(->|\.)(buf|arena|batch)\b", src[name])]
    assert not by_hand, by_hand


def test_the_index_check_is_one_device_function():
    src = _sources()
    assert _files(_calls("rec_check_indices")) == ["refit.hip", "topcorr.hip"] and len(_calls("rec_check_indices")) == 3
    assert not [name for name, text in src.items() if name != HOME and re.search(r"\w\[e\]\s*>=\s*n\)\s*atomicMin\(", text)]
