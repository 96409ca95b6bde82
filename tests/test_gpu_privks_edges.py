"""GPU: the private key switch, the lvl2 TLWE store and iyk_hip_trgsw_from_rows at the launch plans, digit shapes, store sizes and host
situations the other tests do not run — the cases of tests/privks_edge_cases.py, whose claims tests/test_privks_cases.py proves on the
CPU.  Every comparison is word for word against tests/privks_ref.py (and tests/cmux_ref.py for what a selector does); where two routes
of the library are compared with each other the test says so.

The replica and re-initialisation cases run in a child process (tests/privks_edges_child.py)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import cmux_ref
import privks_edge_cases as cases

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("gpu", ["128", "80"], indirect=True)
ONE = pytest.mark.parametrize("gpu", ["128"], indirect=True)


@pytest.fixture(scope="module")
def gpu(request):
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + request.param)
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    made = {}
    yield hip, keys, st, made
    for x in made.values():
        x.free()
    st.destroy()
    hip.cleanup()


def _plan_store(gpu):
    """The key and the 64 lvl2 TLWEs of tests/privks_edge_cases.plan_store, resident once per module."""
    hip, _, st, made = gpu
    if "key" not in made:
        tl, K = cases.plan_store()
        made["key"] = hip.PrivKsKey(cases.PLAN_N_IN, cases.PLAN_T, cases.PLAN_BB)
        made["key"].upload(st, 0, K)
        made["tlwe2"] = hip.Tlwe2(cases.PLAN_N_IN, cases.PLAN_TLWES)
        made["tlwe2"].upload(st, 0, tl)
    return made["key"], made["tlwe2"]


def _assert_rows(got, want, what=""):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: rows that differ from the reference: {bad[:10]} of {got.shape[0]}"


def _need_free(nbytes, what):
    import torch

    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + (1 << 30):
        pytest.skip(f"{what}: the allocation of {nbytes} bytes cannot succeed, the device has {free} free")


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. launch plans ------------------------------------------------------------------------------------------------------------------

@ONE
@pytest.mark.parametrize("character", list(cases.CHARACTERS))
def test_launch_plans(gpu, character):
    """n_in = 12: one split (about a thousand jobs at 256 CUs), two uneven splits, three with a short tail, a last split of one word,
    fewer splits than asked for, one word per split.  The batch size comes from a search with the device's CU count; every job reads
    rows in every split, so a dropped or shortened split changes its row.  The whole store is compared, the rows no job writes too."""
    hip, _, st, _ = gpu
    cus = _cus()
    case = cases.plan_case(character, cus)
    assert case is not None, f"no batch size gives a plan of this character at {cus} CUs"
    count, splits, per = case["count"], case["splits"], case["per"]
    assert cases.CHARACTERS[character](count, cus, splits, per)
    if cus == 256:
        assert count == cases.AT_256_CUS[character] and (splits, per) == cases.PLANS_AT_256_CUS[character]
    key, store = _plan_store(gpu)
    rows = case["T"].shape[0]
    trl = hip.Trlwe(rows)
    try:
        trl.upload(st, 0, case["T"])
        for jobs in case["batches"]:
            st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
        got = trl.download(st, 0, rows)
    finally:
        trl.free()
    _assert_rows(got, case["want"], f"{character}: {count} jobs, {splits} splits of {per} at {cus} CUs")


# ---- 2. digit shapes ------------------------------------------------------------------------------------------------------------------

@ONE
@pytest.mark.parametrize("t,bb", cases.DIGIT_SHAPES)
def test_digit_shapes(gpu, t, bb):
    """n_in = 3: t = 1; exactly one round of five rows; rounds plus a tail of one, two, three, four rows; basebit 1 (one row per digit) and 8
    (255); 63 bits (rounding constant 1).  Words built from their digits: every digit at its largest, zero and non-zero digits
    alternating inside a round, one digit alone at the end, at the start of the last round, at the start."""
    hip, _, st, _ = gpu
    case = cases.digit_case(t, bb)
    key = hip.PrivKsKey(cases.DIGIT_N_IN, t, bb)
    tl = case["tlwe2"]
    store, trl = hip.Tlwe2(cases.DIGIT_N_IN, len(tl)), hip.Trlwe(case["T"].shape[0])
    try:
        assert key.rows == case["K"].shape[0]
        key.upload(st, 0, case["K"])
        store.upload(st, 0, tl)
        trl.upload(st, 0, case["T"])
        jobs = case["jobs"]
        st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
        got = trl.download(st, 0, case["T"].shape[0])
    finally:
        key.free()
        store.free()
        trl.free()
    _assert_rows(got, case["want"], f"t = {t}, basebit = {bb}")


# ---- 3. offsets past 32 bits ----------------------------------------------------------------------------------------------------------

@ONE
def test_tlwe2_store_beyond_16_gib(gpu):
    """A lvl2 store of 2^18 + 3 TLWEs of 64 KiB (17.18 GB): jobs read slots 2^16 - 1 and 2^16 (byte offset 2^32), 2^18 - 1 and 2^18 (u64
    word index 2^31) and the last slot, uploaded and downloaded with `first`; the low slots an offset cut to 32 bits lands on hold other
    TLWEs (tests/test_privks_cases.py: the rows they would give differ).  Only the pages used are touched.
    Not covered: a u64 word index past 2^32 (slot 2^19: a store of 34 GB)."""
    hip, _, st, _ = gpu
    case = cases.big_tlwe2_case()
    _need_free(cases.BIG2_SLOTS * (cases.BIG2_N_IN + 1) * 8 + case["K"].nbytes, "lvl2 TLWE store")
    key = hip.PrivKsKey(cases.BIG2_N_IN, cases.BIG2_T, cases.BIG2_BB)
    store, trl = hip.Tlwe2(cases.BIG2_N_IN, cases.BIG2_SLOTS), hip.Trlwe(case["T"].shape[0])
    try:
        key.upload(st, 0, case["K"])
        for s, tl in case["low"].items():            # the sentinels first: a high upload that lands low would write over them
            store.upload(st, s, tl)
        for s, tl in case["high"].items():
            store.upload(st, s, tl)
        trl.upload(st, 0, case["T"])
        jobs = case["jobs"]
        st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
        got = trl.download(st, 0, case["T"].shape[0])
        back = {s: store.download(st, s, 1)[0] for s in list(case["high"]) + list(case["low"])}
        pair = store.download(st, (1 << 16) - 1, 2)  # one transfer across the 2^32-byte line
    finally:
        key.free()
        store.free()
        trl.free()
    for s, tl in {**case["low"], **case["high"]}.items():
        assert np.array_equal(back[s], tl), f"slot {s} came back changed"
    assert np.array_equal(pair, np.stack([case["high"][(1 << 16) - 1], case["high"][1 << 16]]))
    _assert_rows(got, case["want"], "lvl2 store beyond 16 GiB")


@BOTH
def test_trlwe_store_beyond_16_gib(gpu):
    """A row store of 2^21 + 3 rows: privks_batch writes rows 2^19 - 1, 2^19, 2^20 - 1, 2^20, 2^21 - 1, 2^21 and the last one,
    trgsw_from_rows gathers two selectors from those rows.  The selectors are compared through one two-row CMUX job each with selectors
    uploaded from the downloaded rows (two routes of the library) and with cmux_ref on the restated rows.  Rows 0, 1, 2, which the high
    rows alias modulo 2^19 / 2^20 / 2^21 rows, hold sentinels and are compared after each stage."""
    hip, keys, st, _ = gpu
    p = keys.params
    per = p.trgsw_rows
    case = cases.big_trlwe_case(per)
    _need_free(cases.BIGT_ROWS * cases.ROW_BYTES, "row store")
    key, store = _plan_store(gpu)
    high, low = cases.BIGT_HIGH, cases.BIGT_LOW
    C0, cjobs = case["cmux_T"], case["cmux_jobs"]
    big, a, b, ta, tb = hip.Trlwe(cases.BIGT_ROWS), hip.Trgsw(2), hip.Trgsw(2), hip.Trlwe(len(C0)), hip.Trlwe(len(C0))
    fill = np.full((1, cases.WORDS), cases.FILL, dtype=np.uint32)
    try:
        big.upload(st, 0, case["sentinels"])
        for r in high:
            big.upload(st, r, fill)
        ta.upload(st, 0, C0)
        tb.upload(st, 0, C0)
        jobs = case["jobs"]
        st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], big, [j[2] for j in jobs])
        got = {r: big.download(st, r, 1)[0] for r in high}
        low_after_privks = big.download(st, 0, len(low))
        st.trgsw_from_rows(a, [0, 1], big, case["sel_rows"])
        st.cmux_batch(a, ta, *zip(*cjobs))
        for g in range(2):
            b.upload(st, g, np.stack([got[r] for r in case["sel_rows"][g]]).reshape(1, -1))
        st.cmux_batch(b, tb, *zip(*cjobs))
        got_a, got_b = ta.download(st, 0, len(C0)), tb.download(st, 0, len(C0))
        low_after_gather = big.download(st, 0, len(low))
        high_after_gather = {r: big.download(st, r, 1)[0] for r in high}
    finally:
        for x in (big, a, b, ta, tb):
            x.free()
    for r in high:
        assert np.array_equal(got[r], case["want"][r]), f"row {r} (2^{np.log2(r):.2f})"
        assert np.array_equal(high_after_gather[r], case["want"][r]), f"row {r} after the gather"
    assert np.array_equal(low_after_privks, case["sentinels"]) and np.array_equal(low_after_gather, case["sentinels"])
    trg = np.stack([np.stack([case["want"][r] for r in case["sel_rows"][g]]).reshape(per, 2, p.N) for g in range(2)])
    want = cmux_ref.run_jobs(p, C0.copy(), trg, cjobs)
    _assert_rows(got_a, want, "CMUX through the selectors gathered from the high rows")
    _assert_rows(got_b, got_a, "CMUX through the uploaded selectors")


@ONE
def test_key_beyond_4_gib(gpu):
    """n_in = 2048, t = 10, basebit = 4: a key of 5.04 GB of which only the rows of five input words are ever written (and, 2^32 bytes
    under those that lie over byte offset 2^32, rows of other content).  The TLWEs are zero elsewhere: a zero word selects no row (its
    masked re-read of the first row of its i may read memory nobody wrote).  For c = 1 the selected rows of i = 1445 lie under the limit,
    of 1446 on both sides, of 1447 and n_in over it.
    Not covered: 2^32 uint4 ELEMENTS of the key (row 2^23: a key of 64 GB)."""
    hip, _, st, _ = gpu
    case = cases.big_key_case()
    _need_free(cases.key_rows(cases.BIGK_N_IN, cases.BIGK_T, cases.BIGK_BB) * cases.ROW_BYTES, "private key-switch key")
    key = hip.PrivKsKey(cases.BIGK_N_IN, cases.BIGK_T, cases.BIGK_BB)
    store, trl = hip.Tlwe2(cases.BIGK_N_IN, len(case["tlwe2"])), hip.Trlwe(case["T"].shape[0])
    try:
        assert key.rows == 614700 and hip.privks_key_bytes(0) >= key.rows * cases.ROW_BYTES
        for first, n in case["upload"]:
            key.upload(st, first, cases.formula_rows(np.arange(first, first + n)))
        store.upload(st, 0, case["tlwe2"])
        trl.upload(st, 0, case["T"])
        jobs = case["jobs"]
        st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
        got = trl.download(st, 0, case["T"].shape[0])
    finally:
        key.free()
        store.free()
        trl.free()
    _assert_rows(got, case["want"], "key beyond 4 GiB")


# ---- 4. host runtime ------------------------------------------------------------------------------------------------------------------

def _issue(st, call, key, store, rows, sel, crows, sync=False):
    if call[0] == "privks":
        st.privks_batch(key, store, [j[0] for j in call[1]], [j[1] for j in call[1]], rows, [j[2] for j in call[1]])
    elif call[0] == "from_rows":
        st.trgsw_from_rows(sel, call[1], rows, call[2])
    else:
        st.cmux_batch(sel, crows, *zip(*call[1]))
    if sync:
        st.sync()


@BOTH
def test_queue_past_the_staging_ring(gpu):
    """ONE fresh stream, no synchronisation: fourteen privks_batch calls with fourteen job lists (the ring has eight staging slots, and
    the job list lives in it), trgsw_from_rows with 1, 5 and 40 selectors in between (the stream's selector scratch is reallocated twice
    behind queued work) and a cmux_batch through every selector; the last privks batch writes over the rows of the first selector,
    which must have been gathered before.  Everything is downloaded at the end."""
    hip, keys, _, _ = gpu
    p = keys.params
    case = cases.queue_case(p.trgsw_rows)
    key, store = _plan_store(gpu)
    R0, C0 = case["R0"], case["C0"]
    st = hip.Stream(0)
    rows, crows, sel = hip.Trlwe(len(R0)), hip.Trlwe(len(C0)), hip.Trgsw(case["slots"])
    try:
        rows.upload(st, 0, R0)
        crows.upload(st, 0, C0)                      # (an upload synchronises: nothing is queued before the program starts)
        for call in case["program"]:
            _issue(st, call, key, store, rows, sel, crows)
        got_R, got_C = rows.download(st, 0, len(R0)), crows.download(st, 0, len(C0))
    finally:
        for x in (rows, crows, sel):
            x.free()
        st.destroy()
    trg = np.zeros((case["slots"], p.trgsw_rows, 2, p.N), dtype=np.uint32)
    want_R, want_C = cases.run_reference(p, case, case["program"], R0.copy(), C0.copy(), trg)
    _assert_rows(got_R, want_R, "rows of fourteen queued batches")
    _assert_rows(got_C, want_C, "CMUX through the selectors of three queued trgsw_from_rows calls")


@BOTH
@pytest.mark.parametrize("name", list(cases.SLOT_LISTS))
def test_slot_lists(gpu, name):
    """trgsw_from_rows with several runs of slots in one call, descending slots (one launch each), the store's last slot inside a run, a
    row shared by two selectors: one CMUX job through every slot against cmux_ref on the rows, and against selectors uploaded from the
    same rows (two routes of the library)."""
    hip, keys, st, _ = gpu
    p = keys.params
    per = p.trgsw_rows
    case = cases.slot_case(name, per)
    R, C0, slots = case["R"], case["C0"], case["slots"]
    rows, a, b, ta, tb = hip.Trlwe(len(R)), hip.Trgsw(cases.SLOT_STORE), hip.Trgsw(cases.SLOT_STORE), hip.Trlwe(len(C0)), hip.Trlwe(len(C0))
    try:
        rows.upload(st, 0, R)
        ta.upload(st, 0, C0)
        tb.upload(st, 0, C0)
        st.trgsw_from_rows(a, slots, rows, case["rows"])
        st.cmux_batch(a, ta, *zip(*case["jobs"]))
        for g, slot in enumerate(slots):
            b.upload(st, slot, R[case["rows"][g]].reshape(1, -1))
        st.cmux_batch(b, tb, *zip(*case["jobs"]))
        got_a, got_b = ta.download(st, 0, len(C0)), tb.download(st, 0, len(C0))
    finally:
        for x in (rows, a, b, ta, tb):
            x.free()
    trg = np.zeros((cases.SLOT_STORE, per, 2, p.N), dtype=np.uint32)
    for g, slot in enumerate(slots):
        trg[slot] = R[case["rows"][g]].reshape(per, 2, p.N)
    _assert_rows(got_a, cmux_ref.run_jobs(p, C0.copy(), trg, case["jobs"]), f"slots {slots}")
    _assert_rows(got_b, got_a, f"slots {slots}, uploaded")


@BOTH
def test_two_streams_two_threads(gpu):
    """Two host threads, a stream each, one key, one lvl2 store, one row store, one selector store, disjoint rows and slots: five
    rounds of privks_batch + trgsw_from_rows + cmux_batch per thread, unsynchronised.  The words equal the reference, and the same
    programs on one stream with a sync after every call."""
    hip, keys, st, _ = gpu
    p = keys.params
    case = cases.two_stream_case(p.trgsw_rows)
    key, store = _plan_store(gpu)
    R0, C0 = case["R0"], case["C0"]

    def run(streams, sync):
        rows, crows, sel = hip.Trlwe(len(R0)), hip.Trlwe(len(C0)), hip.Trgsw(case["slots"])
        errors = []

        def worker(s, prog):
            try:
                for call in prog:
                    _issue(s, call, key, store, rows, sel, crows, sync)
            except Exception as e:   # noqa: BLE001 — reported by the parent thread
                errors.append(e)

        try:
            rows.upload(st, 0, R0)
            crows.upload(st, 0, C0)
            if len(streams) == 2:
                threads = [threading.Thread(target=worker, args=(s, prog)) for s, prog in zip(streams, case["programs"])]
                for t in threads:
                    t.start()
                for t in threads:
                    t.join()
            else:
                for prog in case["programs"]:
                    worker(streams[0], prog)
            assert not errors, errors
            for s in streams:
                s.sync()
            return rows.download(st, 0, len(R0)), crows.download(st, 0, len(C0))
        finally:
            for x in (rows, crows, sel):
                x.free()

    s0, s1 = hip.Stream(0), hip.Stream(0)
    try:
        got_R, got_C = run([s0, s1], False)
        one_R, one_C = run([s0], True)
    finally:
        s0.destroy()
        s1.destroy()
    trg = np.zeros((case["slots"], p.trgsw_rows, 2, p.N), dtype=np.uint32)
    want_R, want_C = R0.copy(), C0.copy()
    for prog in case["programs"]:
        cases.run_reference(p, case, prog, want_R, want_C, trg)
    _assert_rows(got_R, want_R, "rows, two streams")
    _assert_rows(got_C, want_C, "CMUX rows, two streams")
    assert np.array_equal(one_R, got_R) and np.array_equal(one_C, got_C)


def test_second_replica_and_reinitialisation():
    """In a fresh process (tests/privks_edges_child.py): two replicas aliased to device 0, a key on replica 1 — refused with a stream
    of replica 0, the reference's words with a stream of replica 1, the key bytes counted per replica — then cleanup + initialize with
    the key alive: the counters are 0 and stay 0 when the old key is freed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "privks_edges_child.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok replica reinit" in r.stdout, r.stdout + r.stderr
