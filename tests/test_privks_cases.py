"""CPU: the cases of tests/privks_edge_cases.py are what they claim to be — which launch plan each batch size gets at every CU count, that
every job reads key rows in every split of its plan, the digits of the built words (restatement and the library's shared digit
function), which side of each 32-bit limit the selected rows lie on, and that a read or write through an offset cut to 32 bits would
give other words than the expected ones.  test_gpu_privks_edges runs the same cases through the kernels."""
import numpy as np
import pytest

import privks_edge_cases as cases
import privks_ref as ref


def _distinct(rows):
    flat = np.stack(rows)
    return len(np.unique(flat, axis=0)) == len(flat)


@pytest.mark.parametrize("cus", [1, 8, 256, 304])
def test_plan_characters(cus):
    """the search finds every character or says it does not exist; every job selects a row in every split; no two (in, c) give equal rows"""
    missing = []
    for character, ok in cases.CHARACTERS.items():
        case = cases.plan_case(character, cus)
        if case is None:
            # really none: no batch size up to one job per wanted workgroup (and one more: from there on the plan is one split)
            assert all(not ok(n, cus, *cases.plan(n, cases.PLAN_WORDS, cus)) for n in range(1, cases.WG_PER_CU * cus + 2)), character
            assert cases.plan(1 << 20, cases.PLAN_WORDS, cus) == (1, cases.PLAN_WORDS)
            missing.append(character)
            continue
        count, splits, per = case["count"], case["splits"], case["per"]
        assert (splits, per) == cases.plan(count, cases.PLAN_WORDS, cus) and ok(count, cus, splits, per), character
        assert (splits - 1) * per < cases.PLAN_WORDS <= splits * per
        jobs = [j for b in case["batches"] for j in b]
        assert len(jobs) == max(count, 2) and all(len(b) == count for b in case["batches"])
        for in_ in {j[0] for j in jobs}:
            assert cases.rows_per_split(case["tlwe2"][in_], splits, per).min() > 0, (character, in_)
        assert {j[1] for j in jobs} == {0, 1}
        outs = [j[2] for j in jobs]
        rows = case["T"].shape[0]
        assert len(set(outs)) == len(outs) and 0 in outs and rows - 1 in outs and rows == count + cases.PLAN_EXTRA_ROWS
        assert _distinct(list(case["rows_of"].values())), character
        if count > 64:
            assert len(case["rows_of"]) < count          # `in` repeats
        untouched = sorted(set(range(rows)) - set(outs))
        assert len(untouched) >= 2 and np.all(case["want"][untouched] == cases.FILL)
        assert not np.any(np.all(case["want"][outs] == cases.FILL, axis=1))
    print(f"{cus} CUs: no plan of character {missing}" if missing else f"{cus} CUs: every character found")
    if cus == 256:
        assert not missing
        for character, count in cases.AT_256_CUS.items():
            case = cases.plan_case(character, cus)
            assert case["count"] == count and (case["splits"], case["per"]) == cases.PLANS_AT_256_CUS[character], character
    if cus == 1:
        assert "finest cut" in missing                   # 4 workgroups wanted: never 13 splits


def test_plan_store_has_the_edge_words():
    tl, K = cases.plan_store()
    assert K.shape == (1820, cases.WORDS) and tl.shape == (64, 13)
    edges = [w for w, _ in ref.edge_words(cases.PLAN_T, cases.PLAN_BB).values()]
    for pos in (0, cases.PLAN_N_IN - 1, cases.PLAN_N_IN):
        assert set(edges) <= {int(w) for w in tl[40:55, pos]}
    # the edge TLWEs take part in the plans that allow it: the coarse plans use all of them, the finest cut only those without a zero word
    used = {j[0] for b in cases.plan_case("one split", 256)["batches"] for j in b}
    assert set(range(40, 55)) <= used and 39 not in used
    fine = {j[0] for b in cases.plan_case("finest cut", 256)["batches"] for j in b}
    assert all((ref.digits(tl[g], cases.PLAN_T, cases.PLAN_BB) != 0).any(axis=1).all() for g in fine)


@pytest.mark.parametrize("t,bb", cases.DIGIT_SHAPES)
def test_digit_words_have_their_digits(t, bb):
    assert 1 <= bb <= 8 and bb * t <= 63
    nb = (1 << bb) - 1
    words = cases.digit_words(t, bb)
    names = [n for n, _, _ in words]
    assert len(set(names)) == len(names)
    arr = np.array([w for _, w, _ in words], dtype=np.uint64)
    got = ref.digits(arr, t, bb)
    assert np.array_equal(cases.emul_digits(arr, t, bb), got)            # the function the kernel shares with the CPU
    edges = ref.edge_words(t, bb)
    for (name, w, d), g in zip(words, got):
        if d is not None:
            assert list(g) == list(d), name
        elif name in edges and edges[name][1] is not None:
            assert np.all(g == edges[name][1]), name
    by = dict(zip(names, got))
    assert np.all(by["every digit nb"] == nb)
    assert by["only digit t - 1"][t - 1] != 0 and np.count_nonzero(by["only digit t - 1"]) == 1
    j = cases.UNROLL * ((t - 1) // cases.UNROLL)
    assert by["only the first digit of the last round"][j] != 0 and np.count_nonzero(by["only the first digit of the last round"]) == 1
    assert by["only digit 0"][0] != 0 and np.count_nonzero(by["only digit 0"]) == 1
    if t > 1:
        a, b = by["0, nb, 0, nb"], by["nb, 0, nb, 0"]
        assert np.all(a[1::2] == nb) and not a[0::2].any() and np.all(b[0::2] == nb) and not b[1::2].any()
    case = cases.digit_case(t, bb)
    assert case["K"].shape[0] == cases.key_rows(cases.DIGIT_N_IN, t, bb)
    assert {j[1] for j in case["jobs"]} == {0, 1} and len({j[2] for j in case["jobs"]}) == len(case["jobs"])
    # words with a non-zero digit give rows that differ between c = 0 and c = 1 and from each other
    live = [g for g in range(len(case["tlwe2"])) if (ref.digits(case["tlwe2"][g], t, bb) != 0).any()]
    out = {j[:2]: j[2] for j in case["jobs"]}
    if (t, bb) != (1, 1):   # one digit of one bit: every live word selects the same four rows
        distinct = {tuple(ref.digits(case["tlwe2"][g], t, bb).ravel()): g for g in live}   # one TLWE per digit pattern
        assert _distinct([case["want"][out[(g, c)]] for g in distinct.values() for c in (0, 1)])
    assert len(live) >= 4


def test_largest_digit_key_size():
    assert max(cases.key_rows(cases.DIGIT_N_IN, t, bb) for t, bb in cases.DIGIT_SHAPES) == 14280


def test_big_tlwe2_case():
    """the high slots sit on both sides of byte offset 2^32 and u64 word index 2^31; every aliased read would give another row"""
    case = cases.big_tlwe2_case()
    words = cases.BIG2_N_IN + 1
    assert cases.BIG2_SLOTS * words * 8 > 17 * 10 ** 9 and case["K"].shape[0] == 16384
    off = lambda s: s * words * 8
    assert off((1 << 16) - 1) < 1 << 32 <= off(1 << 16) and ((1 << 18) - 1) * words < 1 << 31 <= (1 << 18) * words
    assert max(cases.BIG2_HIGH) == cases.BIG2_SLOTS - 1
    assert {0, 1, 2} <= set(case["low"]) and all(a in case["low"] or a in case["high"] for s in cases.BIG2_HIGH for a in cases.big2_aliases(s))
    assert cases.big2_aliases(1 << 16) == [0] and cases.big2_aliases((1 << 18) + 2) == [2, (1 << 18) + 2 - (1 << 16)]
    assert cases.big2_aliases((1 << 16) - 1) == []      # under every limit: the control
    outs = {(s, c): out for s, c, out in case["jobs"]}
    assert len(outs) == 2 * len(cases.BIG2_HIGH)
    for (s, c, a), row in case["alias_rows"].items():
        assert not np.array_equal(row, case["want"][outs[(s, c)]]), (s, c, a)
    assert _distinct([case["want"][o] for o in outs.values()])
    assert np.all(case["want"][-1] == cases.FILL)


@pytest.mark.parametrize("per", [6, 4])
def test_big_trlwe_case(per):
    case = cases.big_trlwe_case(per)
    assert cases.BIGT_ROWS * cases.ROW_BYTES > 1 << 34
    high = cases.BIGT_HIGH
    assert [r * cases.ROW_BYTES >= 1 << 32 for r in high] == [False] + [True] * 6
    assert [r * cases.WORDS >= 1 << 31 for r in high] == [False] * 3 + [True] * 4
    assert [r * cases.WORDS >= 1 << 32 for r in high] == [False] * 5 + [True] * 2
    assert max(high) == cases.BIGT_ROWS - 1
    # what a cut offset lands on is a sentinel row or another job's row, and the jobs' rows all differ
    for r in high:
        assert all(a in cases.BIGT_LOW or a in high for a in cases.bigt_aliases(r))
    assert {a for r in high for a in cases.bigt_aliases(r)} >= {0, 2}
    assert _distinct(list(case["want"].values()) + list(case["sentinels"]))
    assert case["sel_rows"].shape == (2, per) and set(case["sel_rows"].ravel()) == set(high)


def test_big_key_case():
    """c = 1: the selected rows of i = 1445 lie under byte offset 2^32, of i = 1446 on both sides, of i = 1447 and i = n_in over it"""
    case = cases.big_key_case()
    L = cases.BIGK_LIMIT
    assert L == 524288 and cases.key_rows(cases.BIGK_N_IN, cases.BIGK_T, cases.BIGK_BB) == 614700
    assert 614700 * cases.ROW_BYTES > 5 * 10 ** 9 and 614700 * 512 < 1 << 32   # past 2^32 bytes, not past 2^32 uint4 elements
    sel = case["selected"]
    assert sel[0].max() < L
    of_i = lambda i: sel[1][(sel[1] >= cases.bigk_row(1, i, 0, 1)) & (sel[1] < cases.bigk_row(1, i + 1, 0, 1))]
    assert of_i(0).size and of_i(0).max() < L
    assert of_i(1445).size and of_i(1445).max() < L
    assert of_i(1446).min() < L <= of_i(1446).max()
    assert of_i(1447).size and of_i(1447).min() >= L
    assert of_i(cases.BIGK_N_IN).size and of_i(cases.BIGK_N_IN).max() == 614699      # the key's last row
    up = np.concatenate([np.arange(f, f + n) for f, n in case["upload"]])
    assert len(np.unique(up)) == len(up) and up.max() == 614699 and len(up) < 2500
    over = sel[1][sel[1] >= L]
    assert np.isin(np.concatenate([sel[0], sel[1], over - L]), up).all()       # every true row and every alias row is written
    assert not np.any(np.all(cases.formula_rows(over) == cases.formula_rows(over - L), axis=1))
    # a key offset cut to 32 bits changes every c = 1 row and no c = 0 row
    for g, c, out in case["jobs"]:
        assert np.array_equal(case["want"][out], case["want_aliased"][out]) == (c == 0), (g, c)
    assert np.all(case["want"][-1] == cases.FILL)


@pytest.mark.parametrize("per", [6, 4])
def test_host_runtime_cases(per):
    q = cases.queue_case(per)
    kinds = [c[0] for c in q["program"]]
    assert kinds.count("privks") == 14 and kinds.count("from_rows") == 3 and len(kinds) > 2 * 8
    lists = [tuple(c[1]) for c in q["program"] if c[0] == "privks"]
    assert len(set(lists)) == 14
    counts = [len(c[1]) for c in q["program"] if c[0] == "from_rows"]
    assert counts == [1, 5, 40]
    cap = 0
    grows = 0
    for n in counts:                                     # ensure_sel's rule: n + n / 2 + 2
        if n > cap:
            cap, grows = n + n // 2 + 2, grows + 1
    assert grows == 3                                    # the first allocation and two reallocations behind queued work
    first_sel_rows = set(q["program"][2][2].ravel())
    assert first_sel_rows <= {j[2] for j in q["program"][-3][1]}          # the last batch writes over the first selector's rows
    for name, slots in cases.SLOT_LISTS.items():
        s = cases.slot_case(name, per)
        runs = 1 + sum(b != a + 1 for a, b in zip(slots, slots[1:]))
        assert runs == {"several runs": 4, "descending": 3, "the last slot inside a run": 2}[name]
        assert len(set(slots)) == len(slots) and max(slots) < cases.SLOT_STORE
        assert all(s["rows"][g, 0] in s["rows"][g - 1] for g in range(1, len(slots)))
    assert cases.SLOT_STORE - 1 in cases.SLOT_LISTS["the last slot inside a run"][1:3]
    two = cases.two_stream_case(per)
    touched = []
    for prog in two["programs"]:
        rows = {j[2] for c in prog if c[0] == "privks" for j in c[1]}
        slots = {s for c in prog if c[0] == "from_rows" for s in c[1]}
        crow = {r for c in prog if c[0] == "cmux" for j in c[1] for r in j[1:3] + j[4:]}
        touched.append((rows, slots, crow))
    assert all(not (a & b) for a, b in zip(*touched))
    assert max(touched[1][1]) == two["slots"] - 1
