"""The schedules of tests/exchange_cases.py can tell a wrong replica exchange from a right one, and the arithmetic the GPU cases of
tests/test_gpu_zz_exchange.py rest on holds for the constants of iyokan_amd/csrc/iyokan_hip.hip as its source text states them.  No GPU."""
import os
import re

import numpy as np
import pytest

import arena_cases as ac
import exchange_cases as ec
from iyokan_amd.params import params_128bit, params_80bit

N1 = [params_128bit().n + 1, params_80bit().n + 1]
TINY = 9                    # words per row of the mutant runs: the model does not care, and the rows differ in every word at any width
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iyokan_amd", "csrc", "iyokan_hip.hip")
KINDS = {"drop", "late", "stale", "future", "short", "shift", "skipdst"}


@pytest.fixture(scope="module")
def source():
    with open(SRC) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


@pytest.fixture(scope="module")
def constants(source):
    """STAGE_RING, the growth rule of ensure_stage, what the exchange asks acquire_stage for and its limits, from the source text."""
    ring = int(_one(r"constexpr int STAGE_RING = (\d+);", source))
    div, add, rnd, mask = map(int, _one(r"size_t cap = \(bytes \+ bytes / (\d+) \+ (\d+) \+ (\d+)\) & ~\(size_t\)(\d+);", source))
    assert rnd == mask and mask & (mask + 1) == 0
    assert _one(r"size_t stage_cap = (\d+);", source) == "0"           # a new stream has no staging: its first list allocates
    body = source[source.index("int iyk_hip_arena_sync_slots_multi("):source.index("int iyk_hip_arena_sync_slots(")]
    pad = _one(r"idx_bytes = \(count \* sizeof\(int32_t\) \+ (\d+)\) & ~\(size_t\)(\d+), row_bytes = count \* n1 \* sizeof\(u32\);", body)
    assert pad[0] == pad[1] and body.count("acquire_stage(") == 2 and len(re.findall(r"acquire_stage\(\w+, idx_bytes \+ row_bytes, ", body)) == 2
    max_dst = int(_one(r"constexpr int MAX_GPUS = (\d+);", source))
    assert "if (ndst > MAX_GPUS) return fail(IYK_ERR_INVALID" in body
    shift = int(_one(r"if \(count > \(1u << (\d+)\)\) return fail\(IYK_ERR_INVALID", body))
    return dict(ring=ring, cap=lambda b: (b + b // div + add + rnd) & ~mask, list_bytes=lambda c, n1: ((c * 4 + int(pad[0])) & ~int(pad[0])) + c * n1 * 4,
                max_dst=max_dst, max_count=1 << shift)


def test_the_mirrors_are_the_source_texts(constants):
    assert ec.STAGE_RING == constants["ring"] == ac.STAGE_RING
    assert ec.MAX_DST == constants["max_dst"] and ec.MAX_COUNT == constants["max_count"]
    for b in (0, 1, 72, 4097, 20416, 34816, 571_648, 6_921_024, 167_255_684):
        assert ec.stage_cap_after(b) == constants["cap"](b) == ac.stage_cap_after(b)
    for n1 in N1 + [TINY]:
        for c in (1, 3, 4, 5, 8, 40, 8192, 65539):
            assert ec.list_stage_bytes(c, n1) == constants["list_bytes"](c, n1) == ac.slot_list_stage_bytes(c, n1)


def test_rows_differ_in_every_word():
    n1 = 637
    base = ec.rows(2, [5], 3, n1)[0]
    for r, s, g in ((1, 5, 3), (2, 6, 3), (2, 5, 2), (2, 5, 4), (0, 0, 0), (7, (1 << 22) - 1, 126), (2, 5, ec.HIST_GEN)):
        assert np.all(ec.rows(r, [s], g, n1)[0] != base)
    two = ec.rows(2, [5, 6], 3, n1 + 40).reshape(-1)
    for off in (1, 2, 40):                                               # a row read at a word offset
        assert np.all(ec.rows(2, [5], 3, n1 + 40)[0][off:off + n1] != base) and np.all(two[off:off + n1] != base)
    many = ec.rows(1, np.arange(70000), 9, 3)
    assert len(np.unique(many[:, 0])) == 70000 and np.array_equal(many, ec.rows(1, np.arange(70000), 9, 3))
    for bad in ((8, [0], 0), (0, [0], 128), (0, [1 << 22], 0)):
        with pytest.raises(AssertionError):
            ec.rows(*bad, 4)


def _schedules(n1):
    return ec.small_cases(n1, big_n1=N1[0]) + [ec.long_case(n1, count=300)]


@pytest.mark.parametrize("name", [c["name"] for c in _schedules(TINY)])
def test_every_mutant_changes_the_result(name):
    """Every wrong exchange of exchange_cases.mutants, at every exchange of the schedule, leaves arenas or history that differ from the
    expected ones; every kind of mutant that the schedule's shape admits is among them."""
    case = next(c for c in _schedules(TINY) if c["name"] == name)
    want = ec.run(case)
    assert not ec.differ(want, ec.run(case))                             # the model is deterministic
    assert all(a.shape == ((s if case["tracked"] is None else len(case["tracked"])), case["n1"]) for a, s in zip(want, case["sizes"]))
    assert len(want) == case["R"] * (1 + [st[0] for st in case["steps"]].count("check"))
    exchanges = [k for k, st in enumerate(case["steps"]) if st[0] == "exchange" and len(st[2]) and len(st[3])]
    seen = {}
    for m in ec.mutants(case):
        assert ec.differ(want, ec.run(case, m)), (name, m)
        seen.setdefault(m[0], set()).add(m[1])
    for kind in ("drop", "stale", "short", "shift"):
        assert seen[kind] == set(exchanges)
    fanouts = {k for k in exchanges if len(case["steps"][k][2]) > 1}
    assert seen.get("skipdst", set()) == fanouts
    # only an exchange that nothing follows on its slots cannot be late: the last ones of a schedule
    never_late = set(exchanges) - seen.get("late", set())
    assert all(not any(st[0] == "snap" and st[1] in case["steps"][k][2] for st in case["steps"][k + 1:]) for k in never_late)
    if name in ("wrap", "all_to_all", "growth", "relay", "refusals"):
        assert "future" in seen and not never_late
    assert set(seen) <= KINDS


def test_snapshots_follow_every_exchange_and_fit_the_history():
    for case in _schedules(TINY):
        if case["name"] in ("chain", "long", "big"):
            continue                                                     # judged by their final arenas (and "big" after every stage)
        steps = case["steps"]
        used = [set() for _ in range(case["R"])]
        for k, st in enumerate(steps):
            if st[0] == "snap":
                to = set(range(st[4], st[4] + st[3]))
                assert not to & used[st[1]] and min(to) >= case["live"] and max(to) < case["live"] + case["hist"]
                assert st[2] + st[3] <= case["live"] or st[2] >= case["live"] + case["hist"]
                used[st[1]] |= to
            if st[0] == "exchange" and len(st[2]) and len(st[3]):
                for d in st[2]:
                    snapped = set()
                    for nx in steps[k + 1:]:
                        if nx[0] == "snap" and nx[1] == d:
                            snapped |= set(range(nx[2], nx[2] + nx[3]))
                        elif nx[0] in ("write", "exchange") and (nx[1] == d or (nx[0] == "exchange" and d in nx[2])) and nx is not st:
                            break
                    if not (case["name"] == "relay" and d == 1):         # replica 1 of the relay snapshots once, after 0's overwrite
                        assert set(st[3].tolist()) <= snapped, (case["name"], k, d)


def test_wrap_case_wraps_every_ring_several_times(constants):
    ring = constants["ring"]
    for R in (3, 4):
        case = ec.wrap_case(TINY, R=R, ring=ring)
        ex = [st for st in case["steps"] if st[0] == "exchange"]
        assert len(ex) >= 3 * ring and all(st[1] == 0 and len(st[2]) == 1 for st in ex)
        assert [st[2][0] for st in ex[:2 * (R - 1)]] == list(range(1, R)) * 2         # destinations in turn
        acq = ec.acquisitions(case)
        assert acq[0] >= 12 * ring and all(a >= 6 * ring // (R - 1) for a in acq[1:])
        if R == 3:
            assert all(a >= 3 * ring for a in acq)                       # every ring of the three-replica form wraps three times
        assert case["steps"][0] == ("busy", R - 1) == ("busy", case["slow"])
        # each exchange follows a write of a NEW generation to the same source slots
        for k, st in enumerate(case["steps"]):
            if st[0] == "exchange":
                w = case["steps"][k - 1]
                assert w[0] == "write" and w[1] == 0 and sorted(w[2]) == sorted(st[3])
        gens = [st[3] for st in case["steps"] if st[0] == "write"]
        assert gens == list(range(1, len(ex) + 1))


def test_all_to_all_re_records_the_events(constants):
    case = ec.all_to_all_case(TINY)
    assert case["rounds"] == 20 and case["R"] == 3
    ex = [st for st in case["steps"] if st[0] == "exchange"]
    for r in range(3):
        assert sum(st[1] == r for st in ex) == 20 and sum(r in st[2] for st in ex) == 40
    # 60 staging slots per stream for the exchanges alone (80 with the uploads): xfer and xfer2 are recorded again 20 and 40 times
    assert all(a - 20 == 60 and a > 7 * constants["ring"] for a in ec.acquisitions(case))
    own = [set(range(4 * r, 4 * r + 4)) for r in range(3)]
    assert all(set(st[3].tolist()) == own[st[1]] for st in ex) and case["live"] == 12


@pytest.mark.parametrize("n1", N1)
def test_growth_case_reallocates_where_the_gpu_test_says(n1, constants):
    """Under ensure_stage's rule: every stream allocates at its first list and reallocates at L1 and at L2, whatever a busy round's
    descriptors take (none, a 256-CU part's 2 048 gates, four times that); the stream that grows as destination was the source of
    the exchange just before, to the busy replica."""
    small, big1, big2 = ec.growth_sizes(n1)
    cap0 = constants["cap"](constants["list_bytes"](small, n1))
    cap1 = constants["cap"](constants["list_bytes"](big1, n1))
    assert constants["list_bytes"](big1, n1) > cap0 and constants["list_bytes"](big2, n1) > cap1
    assert small < big1 < big2 <= 8192
    assert constants["ring"] * constants["cap"](constants["list_bytes"](big2, n1)) < 250e6          # the pinned ring per stream
    case = ec.growth_case(n1)
    assert case["sizes3"] == (small, big1, big2)
    steps = case["steps"]
    ex = [k for k, st in enumerate(steps) if st[0] == "exchange"]
    sizes = [len(steps[k][3]) for k in ex]
    assert sizes[:3] == [8] * 3 and sizes[3:9] == [8, big1, 8, big2, 40, 8] and len(ex) - 8 > constants["ring"]
    k1, k2 = ex[4], ex[6]
    for gates in (0, 2048, 8192):
        busy = ((gates * 20 + 15) & ~15) + gates * 16                     # arena_cases.gate_batch_stage_bytes of `gates` NANDs
        assert busy < constants["list_bytes"](big1, n1)
        grown = ec.stage_growth(case, busy_bytes=busy)
        for r in range(3):
            mine = [(k, role) for k, s, role in grown if s == r and role != "busy"]
            assert [k for k, _ in mine][-2:] == [k1, k2] and len(mine) == 3 and mine[0][0] <= ex[0]
        roles = {(k, s): role for k, s, role in grown}
        assert roles[(k1, 0)] == "source" and roles[(k1, 1)] == roles[(k1, 2)] == "destination"
        assert roles[(k2, 2)] == "source" and roles[(k2, 0)] == roles[(k2, 1)] == "destination"
    # the exchange just before each: from the stream that is about to grow as destination, to the busy replica alone
    for k, grows, busy_replica in ((k1, 1, 2), (k2, 0, 1)):
        before = steps[ex[ex.index(k) - 1]]
        assert before[1] == grows and before[2] == (busy_replica,)
        between = steps[ex[ex.index(k) - 1] + 1:k]
        assert all(st[0] == "snap" and st[1] == busy_replica for st in between)           # nothing more on the growing stream
        assert any(st == ("busy", busy_replica) for st in steps[:ex[ex.index(k) - 1]][-6:])


def test_chain_case_reads_across_replicas():
    for R in (3, 4):
        case = ec.chain_case(TINY, R=R)
        deals = case["deals"]
        assert len(deals) == 6 and all(len(d["out"]) == 48 for d in deals)
        owner_of = {}
        for k, d in enumerate(deals):
            if k:
                below = set(deals[k - 1]["out"].tolist())
                for g in range(48):
                    assert int(d["in0"][g]) in below and owner_of[int(d["in0"][g])] != d["owner"][g]
            owner_of.update(zip(d["out"].tolist(), d["owner"].tolist()))
            assert np.array_equal(np.bincount(d["owner"], minlength=R), np.bincount(np.arange(48) % R, minlength=R))
        gates = [st for st in case["steps"] if st[0] == "gates"]
        assert len(gates) == 6 * R and {int(k) for st in gates for k in st[2]["kind"]} == {0, 1, 2}
        assert all(np.all((st[2]["in2"] >= 0) == (st[2]["kind"] == 2)) for st in gates)
        # a level's gates are independent: no gate reads or overwrites an output of its own level
        for st in gates:
            lv = st[2]
            assert len(set(lv["out"].tolist())) == len(lv["out"]) and not set(lv["out"].tolist()) & set(np.concatenate([lv["in0"], lv["in1"], lv["in2"]]).tolist())
        # after each level every replica fans ALL its outputs out to all the others
        kinds = [st[0] for st in case["steps"]]
        assert kinds == (["gates"] * R + ["exchange"] * R) * 6
        for k, d in enumerate(deals):
            for st in case["steps"][2 * R * k + R:2 * R * (k + 1)]:
                assert sorted(st[3].tolist()) == d["out"][d["owner"] == st[1]].tolist() and sorted(st[2]) == [x for x in range(R) if x != st[1]]
        want = ec.run(case)
        assert all(np.array_equal(a[case["nin"]:case["live"]], want[0][case["nin"]:case["live"]]) for a in want)   # all replicas agree


def test_shapes_case_holds_the_shapes():
    case = ec.shapes_case(TINY)
    T = min(case["sizes"])
    ex = [st for st in case["steps"] if st[0] == "exchange"]
    assert case["R"] == 8 and len(set(case["sizes"])) > 1 and any(len(st[2]) == 7 for st in ex)
    assert any(len(st[3]) == 1 for st in ex) and any(sorted(st[3]) == [0, T - 1] for st in ex)
    assert any(len(set(st[3].tolist())) < len(st[3]) and list(st[3]).count(st[3][-1]) == 1 for st in ex)
    assert any(len(st[2]) == 0 and len(st[3]) for st in ex) and any(len(st[2]) and len(st[3]) == 0 for st in ex)
    refused = [st for st in case["steps"] if st[0] == "refused"]
    assert len(refused) == 3
    for _, src, dsts, slots in refused:
        assert int(slots.max()) >= min(case["sizes"][r] for r in (src,) + dsts)
    assert any(int(st[3].max()) < case["sizes"][st[1]] and int(st[3].max()) == T for st in refused)   # valid on the source, first slot past the smallest
    last = max(k for k, st in enumerate(case["steps"]) if st[0] == "refused")
    after = [st for st in case["steps"][last + 1:] if st[0] == "exchange"]
    assert {after[0][1], *after[0][2]} == {5, 6, 7} == {after[1][1], *after[1][2]}                    # the refused calls' streams exchange again
    long = ec.long_case(TINY)
    lst = long["steps"][1][3]
    assert len(lst) == 65539 > 1 << 16 and len(set(lst.tolist())) == 65539 and 0 in lst and long["R"] == 2
    # pinned staging of that list: one ring slot, and the whole ring that ensure_stage allocates, per stream
    slot = ec.stage_cap_after(ec.list_stage_bytes(65539, N1[0]))
    assert 165e6 < ec.list_stage_bytes(65539, N1[0]) < 170e6 and ec.STAGE_RING * slot < 2.1e9


@pytest.mark.parametrize("n1", N1)
def test_big_case_straddles_byte_2_32(n1):
    case = ec.big_case(n1)
    slots = ec.big_arena_slots(n1)
    c = case["chosen"]
    assert case["sizes"] == [slots, slots] and (slots - 1) * n1 * 4 < (1 << 32) + 3 * n1 * 4 and slots * n1 * 4 > 1 << 32
    assert slots * n1 * 4 < 4.4e9
    assert c["before"] + 1 == c["after"] and c["before"] * n1 * 4 < 1 << 32 <= c["after"] * n1 * 4 and c["last"] == slots - 1 > c["after"]
    lists = [set(st[3].tolist()) for st in case["steps"] if st[0] == "exchange"]
    assert lists == [{0, c["before"], c["after"], c["last"]}] * 2
    tracked = set(case["tracked"].tolist())
    assert ec.byte_alias_slots(c["before"], n1) == [] and ec.byte_alias_slots(0, n1) == []
    for s in (c["after"], c["last"]):
        al = ec.byte_alias_slots(s, n1)
        assert al and set(al) <= tracked and max(al) <= 3
        # the cut offset's row starts inside al[0] and ends inside al[-1]
        w = (s * n1) % (1 << 30)
        assert al[0] * n1 <= w < (al[0] + 1) * n1 and w + n1 <= (al[-1] + 1) * n1
    assert any(a not in (0,) for s in (c["after"], c["last"]) for a in ec.byte_alias_slots(s, n1))   # a sentinel nobody exchanges
    assert [st[0] for st in case["steps"]].count("check") == 3
