"""The host half of the screened solve states each stage's launch once (sparse-solvers_amd/csrc/screen.hip): the screening pass, the
residuals, the fp32 subset Gram matrix, the exact tail, the rescue's ranking, the conversion of the dictionary, the headroom word, the
read-back of a rescue scan and the all-or-nothing takes of the preparations.  A driver that pastes a launch once more fails here.
Source-level, in the manner of tests/test_record_driver.py: counts over csrc/*.hip and *.h, comments left out.
"""
import re

from test_record_driver import _sources

UNIT = "screen.hip"


def _functions(text):
    """[(name, start, end)] of the function definitions at namespace level of a unit without comments: a line that starts in column 0,
    ends its parameter list without a semicolon and is followed by a line holding '{' alone; the body ends at the next line holding '}'
    alone"""
    out = []
    for m in re.finditer(r"^(?!struct |typedef |namespace |template |#|static_assert)[^\s}][^;{}]*?\b(\w+)\s*\([^;{}]*\)\s*\n\{\n", text, flags=re.M):
        end = text.index("\n}\n", m.end() - 1)
        out.append((m.group(1), m.start(), end))
    return out


def _owner(text, pos):
    """the function whose definition holds text[pos] (a definition written on one line: the name in front of its parameter list)"""
    for name, a, b in _functions(text):
        if a <= pos <= b:
            return name
    line = text[text.rfind("\n", 0, pos) + 1:text.index("\n", pos)]
    m = re.match(r"(?:static |inline )*[\w:<>*& ]+?\b(\w+)\s*\([^;{}]*\)\s*\{.*\}\s*$", line)
    return m.group(1) if m else None


def _host(text):
    """the unit's host half: from its first host function on"""
    return text[text.index("static ScreenState* scr_of("):]


def _launchers(kernel):
    """{unit: [function]} of every launch of `kernel` (a regular expression) in csrc"""
    hits = {}
    for unit, text in _sources().items():
        for m in re.finditer(r"hipLaunchKernelGGL\(\(?%s" % kernel, text):
            hits.setdefault(unit, []).append(_owner(text, m.start()))
    return hits


def test_the_function_finder_sees_the_drivers():
    names = [n for n, _, _ in _functions(_sources()[UNIT])]
    for fn in ("launch_screen_form", "launch_screen_rescue_scan", "launch_screen_batch", "screen64_certify", "launch_screen64_rescue_scan",
               "launch_screen64_resident", "launch_screen64_batch", "screen_form_usable", "screen64_usable", "screen_reconvert", "scr_pass"):
        assert names.count(fn) == 1, (fn, names)


def test_the_screening_pass_is_launched_from_one_function():
    # one launcher, a template on the number of state tiles; the dispatcher of the sub-dictionary tier names three of them
    assert _launchers(r"k_scr_gemm<") == {UNIT: ["scr_pass"]}
    text = _sources()[UNIT]
    a, b = next((a, b) for n, a, b in _functions(text) if n == "scr_pass_tiles")
    assert sorted(re.findall(r"scr_pass<(\d)>", text[a:b])) == ["3", "4", "5"]
    # ... whose LDS ceilings are raised beside it, nowhere else
    assert [_owner(text, m.start()) for m in re.finditer(r"hipFuncSetAttribute\([^;]*k_scr_gemm<", text)] == ["scr_pass_attr"]


def test_every_other_stage_has_one_launcher():
    for kernel, fn in (("k_scr_residuals", "launch_scr_residuals"), ("k_sgram_part", "launch_sgram32"), ("k_sgram_sum", "launch_sgram32"),
                       ("k_scr_recheck<", "launch_scr_exact_tail"), ("k_scr_repair<", "launch_scr_exact_tail"),
                       ("k_scr_rescue_rank", "launch_scr_rescue_rank"), ("k_a16_convert<", "launch_a16_convert"), ("k_a8_convert<", "launch_a8_convert")):
        assert _launchers(kernel) == {UNIT: [fn]}, (kernel, _launchers(kernel))


def test_the_headroom_word_is_spelled_once():
    text = _sources()[UNIT]
    spelled = [_owner(text, m.start()) for m in re.finditer(r"meta\s*\)\s*\+\s*3\b", text)]
    assert spelled == ["scr_headroom"], spelled
    assert not re.search(r"meta\s*\+\s*3\b", text)


def test_the_preparations_take_their_lists_through_one_helper():
    text = _sources()[UNIT]
    assert "ok = ok &&" not in text and not re.search(r"\bok\s*&=", text)
    # every device allocation of the unit's preparations goes through Takes; by hand only what is taken alone (the fp8 copy, the rescue's
    # ranking vector, the sub-context's pass partials)
    text = re.sub(r"struct Takes \{.*?\n\};", "", text, flags=re.S)
    by_hand = [_owner(text, m.start()) for m in re.finditer(r"\.device\(", text)]
    assert sorted(by_hand) == ["launch_screen64_rescue_scan", "launch_screen_rescue_scan", "screen64_usable", "screen_first8_ready"], by_hand
    # the residual block is taken and cleared by its own struct, for the single signal and both batch chunks
    assert len(re.findall(r"res\.take\(", text)) == 3 and len(re.findall(r"res\.clear\(", text)) == 3
    assert not re.search(r"hipMemsetAsync\([^;]*r16", re.sub(r"struct ResBlock \{.*?\n\};", "", text, flags=re.S))


def test_the_rescue_lists_are_read_back_in_one_function():
    text = _host(_sources()[UNIT])
    assert [_owner(text, m.start()) for m in re.finditer(r"kScrFlCap \+ 12u", text)] == ["scr_rescue_readback"]
    for scan in ("launch_screen_rescue_scan", "launch_screen64_rescue_scan"):
        a, b = next((a, b) for n, a, b in _functions(text) if n == scan)
        assert text[a:b].count("scr_rescue_readback(") == 1 and "hipStreamSynchronize" not in text[a:b]


def test_the_form_tests_its_state_before_reading_it():
    text = _sources()[UNIT]
    a, b = next((a, b) for n, a, b in _functions(text) if n == "launch_screen_form")
    body = text[a:b]
    null_test = body.index("S == nullptr")
    assert null_test < body.index("S->")
    assert "scr_of(ctx)->" not in body
