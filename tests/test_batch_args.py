"""CPU: csrc/batch_args.hpp — the argument checks and job lists of the batch entry points — through libiyk_emul.so, against what the
parent commit's library answered on an MI355X to the same argument sets (tests/golden/batch_refusals_parent.json, recorded by
tools/record_refusals.py) and against job words written out by hand (tests/batch_refusal_cases.py)."""
import json
import os
import re

import numpy as np
import pytest

import batch_refusal_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "batch_refusals_parent.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
# what iyk_hip_circuit_bootstrap_batch composes: a refusal it gives may be one of theirs
COMPOSED = {"check_circuit_bootstrap_batch": ("check_cb_rotate_batch", "check_privks_batch", "check_trgsw_from_rows")}


def test_every_set_is_recorded():
    assert sorted(GOLDEN) == sorted(c["id"] for c in cases.CASES)
    for c in cases.CASES:   # a set is legal in the table exactly when the parent accepted it
        assert (GOLDEN[c["id"]][0] == cases.OK) == (c["words"] is not None), c["id"]


@pytest.mark.parametrize("c", cases.CASES, ids=[c["id"] for c in cases.CASES])
def test_refusal_and_job_words(c):
    code, text, words, counts = cases.call_emul(c)
    assert [code, text] == GOLDEN[c["id"]]
    if c["words"] is not None:
        want, want_counts = cases.expected_words(c)
        assert counts == want_counts
        assert np.array_equal(words, want), (words, want)


def _texts_per_function():
    """every string literal inside an `inline Refusal check_*(...)` of batch_args.hpp: its refusal texts"""
    src = open(os.path.join(ROOT, "iyokan_amd", "csrc", "batch_args.hpp")).read()
    found = {}
    for m in re.finditer(r"^inline Refusal (check_\w+)\(.*?^}$", src, re.M | re.S):
        found[m.group(1)] = set(re.findall(r'"([^"\n]+)"', m.group(0)))
    return found


def test_every_refusal_has_a_set():
    """The (function, text) pairs the recorded sets reach == the refusal texts a plain-text search of batch_args.hpp finds per function,
    but for cases.UNREACHED.  A check added without a set, and a set whose check was dropped, both fail here."""
    in_source = _texts_per_function()
    assert set(in_source) == {fn for fn, _ in cases.ENTRY.values()}
    reached = {fn: set() for fn in in_source}
    for c in cases.CASES:
        code, text = GOLDEN[c["id"]]
        if code != cases.OK:
            reached[cases.ENTRY[c["entry"]][0]].add(text)
    unreached = {}
    for (entry, text), why in cases.UNREACHED.items():
        assert why
        unreached.setdefault(cases.ENTRY[entry][0], set()).add(text)
    for fn, texts in in_source.items():
        own = reached[fn] & texts
        borrowed = reached[fn] - texts
        assert own | unreached.get(fn, set()) == texts and not own & unreached.get(fn, set()), (fn, texts - own, unreached.get(fn))
        assert borrowed <= set().union(*[in_source[g] for g in COMPOSED.get(fn, ())]), (fn, borrowed)
