"""GPU: the exchange between in-process replicas (iyk_hip_arena_sync_slots / _multi) where no other test drives it — a staging ring
that wraps behind a slow destination, events re-recorded while earlier waits on them are queued, staging reallocated behind queued
exchanges, dependent levels chained across replicas with no host synchronisation, relays and overwrites, edge shapes, refusals and
two arenas past 4 GiB.  The schedules and the arenas they must leave are tests/exchange_cases.py's (checked on the CPU by
tests/test_exchange_cases.py); rows are sentinels that differ in every word, every comparison is word for word, every schedule runs
once with one host synchronisation, at the end.  Replicas are aliased to device 0, so the file runs on a one-GPU box; `distinct`
repeats three cases on real devices.  Own library lifetime (named zz like test_gpu_zz_debug.py): each test initialises and cleans up."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import exchange_cases as ec
from iyokan_amd import client
from iyokan_amd.params import OPS

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
IYK_OK, IYK_ERR_INVALID = 0, -1
WHICH = ["aliased", "distinct"]


def _device_ids(which, R=3):
    """(0,) * R, or for `distinct` max(R, n) replicas dealt over the n = min(device_count, 4) visible GPUs."""
    if which == "aliased":
        return (0,) * R
    import torch

    n = min(torch.cuda.device_count(), 4)
    if n < 2:
        pytest.skip("needs at least two visible GPUs")
    return tuple(g % n for g in range(max(R, n)))


@contextlib.contextmanager
def _replicas(keys, ids, sizes):
    from iyokan_amd import hip

    hip.initialize(keys, device_ids=ids)
    streams, arenas = [], []
    try:
        for g, size in enumerate(sizes):
            streams.append(hip.Stream(g))
            arenas.append(hip.Arena(size, gpu_index=g))
        yield hip, streams, arenas
    finally:
        for ar in arenas:
            ar.free()
        for st in streams:
            st.destroy()
        hip.cleanup()


class _Busy:
    """("busy", r): one full round of NANDs of the same two fresh ciphertexts on a scratch arena of replica r, on r's stream."""

    def __init__(self, hip, keys, orc, replicas):
        self.hip, self.used = hip, []
        self.cts = client.encrypt_bits(keys, [1, 0], seed=91)
        self.want = orc.gate(OPS["NAND"], self.cts[0], self.cts[1])
        self.scratch = {}
        for r in replicas:
            n = hip.rotation_round(r)
            self.scratch[r] = (hip.Arena(n + 2, gpu_index=r), n)

    def prepare(self, streams):
        for r, (ar, _) in self.scratch.items():
            streams[r].upload(ar, 0, self.cts)

    def __call__(self, streams, r):
        ar, n = self.scratch[r]
        nand = np.full(n, OPS["NAND"], dtype=np.int32)
        streams[r].gate_batch(ar, nand, np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32), np.full(n, -1, dtype=np.int32),
                              np.arange(2, n + 2, dtype=np.int32))
        self.used.append(r)

    def check_and_free(self, streams):
        for r, (ar, n) in self.scratch.items():
            if r in self.used:
                got = streams[r].download(ar, 2, n)
                assert np.all(got == self.want[None, :]), f"busy round of replica {r}"
            ar.free()


def _execute(hip, case, streams, arenas, busy=None, gates=None, refuse=None, check=None):
    """Enqueue the schedule, in program order, with no synchronisation of its own."""
    n1 = case["n1"]
    for st in case["steps"]:
        k = st[0]
        if k == "write":
            streams[st[1]].upload_slots(arenas[st[1]], st[2], ec.rows(st[1], st[2], st[3], n1))
        elif k == "exchange":
            src, dsts, slots = st[1:]
            if len(dsts) == 1:
                streams[src].sync_slots_to(arenas[src], streams[dsts[0]], arenas[dsts[0]], slots)
            else:
                streams[src].sync_slots_to_many(arenas[src], [streams[d] for d in dsts], [arenas[d] for d in dsts], slots)
        elif k == "snap":
            streams[st[1]].arena_copy(arenas[st[1]], st[4], arenas[st[1]], st[2], st[3])
        elif k == "gates":
            gates(st[1], st[2])
        elif k == "busy":
            busy(streams, st[1])
        elif k == "refused":
            src, dsts, slots = st[1:]
            with pytest.raises(hip.IykHipError, match="slot index outside the arena"):
                streams[src].sync_slots_to_many(arenas[src], [streams[d] for d in dsts], [arenas[d] for d in dsts], slots)
        elif k == "refuse":
            refuse(st[1])
        elif k == "check":
            check()
        else:
            raise AssertionError(k)


def _compare(got, want, what):
    for r, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f"{what}: replica {r}: {bad.size} slots differ from the model, first {bad[:12].tolist()}"


def _run_model_case(keys, orc, case, ids, **kw):
    """Upload the initial arenas, run the schedule once, download everything behind it, compare with the model."""
    init = ec.initial(case)
    want = ec.run(case)
    with _replicas(keys, ids, case["sizes"]) as (hip, streams, arenas):
        assert hip.lib().iyk_hip_num_gpus() == len(ids) == case["R"]
        busy = None
        if any(st[0] == "busy" for st in case["steps"]):
            busy = _Busy(hip, keys, orc, sorted({st[1] for st in case["steps"] if st[0] == "busy"}))
            busy.prepare(streams)
        for st, ar, rows in zip(streams, arenas, init):
            st.upload(ar, 0, rows)                                   # synchronises: the last time before the downloads
        _execute(hip, case, streams, arenas, busy=busy, **kw)
        got = [st.download(ar, 0, size) for st, ar, size in zip(streams, arenas, case["sizes"])]
        if busy:
            busy.check_and_free(streams)
    _compare(got, want, case["name"])
    assert ec.differ(init, want)
    return got


@pytest.mark.parametrize("which", WHICH)
def test_ring_wraps_behind_a_slow_destination(which, keys128, oracle128):
    """(a) The last replica starts with a full round of NANDs; replica 0 then uploads a new generation of five slots and sends it on,
    6 x STAGE_RING times with no host synchronisation, to the other replicas in turn, each of which snapshots what arrived.  The
    source takes 12 rings of staging slots, so it reuses slots whose peer copies the busy replica queued long before; every arena
    and every snapshot equals the model."""
    ids = _device_ids(which)
    _run_model_case(keys128, oracle128, ec.wrap_case(keys128.params.n + 1, R=len(ids)), ids)


def test_all_to_all_rounds(keys128, oracle128):
    """(b) 20 rounds, no host synchronisation: each replica writes its third of the slots and fans it out to the other two, which
    snapshot it.  Every stream is source 20 times and destination 40 times: xfer and xfer2 are recorded again while waits on their
    earlier records are still queued."""
    _run_model_case(keys128, oracle128, ec.all_to_all_case(keys128.params.n + 1), (0, 0, 0))


@pytest.mark.parametrize("which", WHICH)
def test_staging_grows_behind_queued_exchanges(which, keys128, oracle128):
    """(c) Lists of 8 rows, then one that outgrows the staging slot they left, then one that outgrows the grown slot, then 40 rows and
    a ring and a half of small lists, no host synchronisation.  Each stream grows once as source or destination at either list; the
    stream that grows as destination has just been the source of an exchange to a replica busy with a round of gates, so its old
    staging buffer is still to be read by that replica's stream when ensure_stage comes to free it (tests/test_exchange_cases.py
    derives the sizes and the roles from the growth rule)."""
    ids = _device_ids(which)
    case = ec.growth_case(keys128.params.n + 1, R=len(ids))
    small, big1, big2 = case["sizes3"]
    assert small < big1 < big2 <= 8192
    _run_model_case(keys128, oracle128, case, ids)


@pytest.mark.parametrize("which,bits", [("aliased", "128"), ("aliased", "80"), ("distinct", "128")])
def test_chained_levels_against_the_oracle(which, bits, request):
    """(d) Six levels of 48 NAND / XOR / MUX gates on fresh encryptions, dealt round-robin; every gate above the first level reads an
    output another replica produced one level below; after each level every replica fans its outputs out; no host synchronisation
    anywhere.  All whole arenas equal the oracle's, applied level by level through the same schedule."""
    keys = request.getfixturevalue("keys" + bits)
    orc = request.getfixturevalue("oracle" + bits)
    ids = _device_ids(which)
    n1 = keys.params.n + 1
    case = ec.chain_case(n1, R=len(ids))
    ops_of = lambda lv: np.array([OPS[ec.GATE_KINDS[k]] for k in lv["kind"]], dtype=np.int32)
    host = np.zeros((case["sizes"][0], n1), dtype=np.uint32)
    rng = np.random.default_rng(12)
    host[:case["nin"]] = client.encrypt_bits(keys, rng.integers(0, 2, size=case["nin"]).astype(np.uint8), seed=93)
    with _replicas(keys, ids, case["sizes"]) as (hip, streams, arenas):
        for st, ar in zip(streams, arenas):
            st.upload(ar, 0, host)
        gates = lambda r, lv: streams[r].gate_batch(arenas[r], ops_of(lv), lv["in0"], lv["in1"], lv["in2"], lv["out"])
        _execute(hip, case, streams, arenas, gates=gates)
        got = [st.download(ar, 0, len(host)) for st, ar in zip(streams, arenas)]
    oracle_gates = lambda lv, arena: orc.gate_batch(ops_of(lv), lv["in0"], lv["in1"], lv["in2"], lv["out"], arena, nthreads=NTHREADS)
    want = ec.run(case, gate_fn=oracle_gates, arenas=[host] * len(ids))
    _compare(got, want, "chain")
    assert all(np.array_equal(w, want[0]) for w in want) and np.all(want[0][case["nin"]:case["live"]].any(axis=1))


def test_relay_and_overwrite(keys128, oracle128):
    """(e) 0 -> 1 and at once 1 -> 2 of the same slots; 0 overwrites them as soon as its call returns and sends the new generation to
    2; again with a third generation and a fourth that never leaves 0.  Replicas 1 and 2 and their snapshots hold the generations
    the model says, not the overwritten ones."""
    _run_model_case(keys128, oracle128, ec.relay_case(keys128.params.n + 1), (0, 0, 0))


def test_shapes(keys128, oracle128):
    """(f) Eight aliased replicas of different sizes: a fan-out to seven; a list of one slot; slot 0 with the last slot; repeated
    slots; no destination and no slot (IYK_OK, nothing changes); lists with a slot valid on the source but outside the smallest
    destination, or outside the source (IYK_ERR_INVALID before anything is queued: no arena word changes, and the same streams then
    exchange again, so no staging slot leaked)."""
    _run_model_case(keys128, oracle128, ec.shapes_case(keys128.params.n + 1), (0,) * 8)


def test_list_of_65539_slots(keys128, oracle128):
    """(f) One list of 65 539 slots (more workgroups than 2^16, 167 MB of rows) between two replicas, a sub-case of its own: ensure_stage
    allocates the whole ring of eight slots at 1.5 times the list, 2 GB pinned and 2 GB of device memory per stream."""
    _run_model_case(keys128, oracle128, ec.long_case(keys128.params.n + 1), (0, 0))


def test_refusals(keys128, oracle128):
    """(g) Through the C interface: a destination equal to the source, a repeated destination, a null pointer in each position,
    ndst = 65 and count = 2^24 + 1 each return IYK_ERR_INVALID.  First all of them, after which every arena is unchanged; then each
    of them followed by a valid fan-out on the same streams, after which arenas and snapshots equal the model."""
    from iyokan_amd import hip as H

    vp, i32p, u64 = H._vp, H._i32p, ctypes.c_uint64
    state = {}
    slots = np.array([1, 5, 9], dtype=np.int32)
    huge = np.zeros(ec.MAX_COUNT + 1, dtype=np.int32)

    def call(src=0, dsts=(1, 2), ndst=None, count=None, lst=slots, null=()):
        streams, arenas = state["streams"], state["arenas"]
        n = len(dsts)
        sts = (vp * n)(*[None if f"st_dst[{i}]" in null else streams[d].h for i, d in enumerate(dsts)])
        ptrs = (vp * n)(*[None if f"d_dst[{i}]" in null else arenas[d].ptr for i, d in enumerate(dsts)])
        caps = (u64 * n)(*[arenas[d].slots for d in dsts])
        pick = lambda name, v: None if name in null else v
        return H.lib().iyk_hip_arena_sync_slots_multi(
            pick("st_src", streams[src].h), pick("d_src", arenas[src].ptr), arenas[src].slots, n if ndst is None else ndst,
            pick("st_dst", sts), pick("d_dst", ptrs), pick("dst_slots", caps), len(lst) if count is None else count,
            pick("slots", lst.ctypes.data_as(i32p)))

    many = tuple([1, 2] * 33)[:ec.MAX_DST + 1]
    refusals = [dict(dsts=(0, 1)), dict(dsts=(1, 0)), dict(dsts=(1, 1)), dict(dsts=(1, 2, 1)),
                *[dict(null=(name,)) for name in ("st_src", "d_src", "slots", "st_dst", "d_dst", "dst_slots", "st_dst[0]", "st_dst[1]", "d_dst[0]", "d_dst[1]")],
                dict(dsts=many), dict(lst=huge), dict(lst=huge, dsts=(1,))]
    assert len(many) == 65 and len(huge) == (1 << 24) + 1

    def refuse(k):
        assert call(**refusals[k]) == IYK_ERR_INVALID, refusals[k]
        assert H.lib().iyk_hip_last_error()

    case = ec.refusal_rounds_case(keys128.params.n + 1, len(refusals))
    init = ec.initial(case)
    want = ec.run(case)
    with _replicas(keys128, (0, 0, 0), case["sizes"]) as (hip, streams, arenas):
        state.update(streams=streams, arenas=arenas)
        for st, ar, rows in zip(streams, arenas, init):
            st.upload(ar, 0, rows)
        # the single-destination entry point refuses the same way
        assert H.lib().iyk_hip_arena_sync_slots(streams[0].h, arenas[0].ptr, arenas[0].slots, streams[0].h, arenas[1].ptr, arenas[1].slots,
                                                3, slots.ctypes.data_as(i32p)) == IYK_ERR_INVALID
        assert H.lib().iyk_hip_arena_sync_slots(streams[0].h, arenas[0].ptr, arenas[0].slots, None, arenas[1].ptr, arenas[1].slots,
                                                3, slots.ctypes.data_as(i32p)) == IYK_ERR_INVALID
        for k in range(len(refusals)):
            refuse(k)
        assert call(ndst=0) == IYK_OK and call(count=0) == IYK_OK and call(dsts=(), lst=slots) == IYK_OK
        _compare([st.download(ar, 0, size) for st, ar, size in zip(streams, arenas, case["sizes"])], init, "after the refusals")
        _execute(hip, case, streams, arenas, refuse=refuse)
        got = [st.download(ar, 0, size) for st, ar, size in zip(streams, arenas, case["sizes"])]
    _compare(got, want, "refusals")


def test_two_arenas_past_4_gib(keys128, oracle128):
    """(h) Two replicas with an arena of 2^32 // (4 (n + 1)) + 3 slots each (4.3 GB, only the tracked rows are touched).  The list
    names the last slot that starts below byte 2^32, the first at or above it, slot 0 and the last slot; a row's byte offset cut to
    32 bits in the gather, the scatter or the copies would land in slots 0 .. 3 of the same arena, which hold sentinels (slot 0 a
    row of the list).  After the upload_slots, after 0 -> 1 and after 1 -> 0 of a new generation every tracked slot of both arenas
    is compared with the model.  Skips only when the allocation itself is refused."""
    n1 = keys128.params.n + 1
    case = ec.big_case(n1)
    tracked = [int(s) for s in case["tracked"]]
    init = ec.initial(case)
    want = ec.run(case)
    from iyokan_amd import hip as H

    try:
        ctx = _replicas(keys128, (0, 0), case["sizes"])
        hip, streams, arenas = ctx.__enter__()
    except H.IykHipError as e:
        if "out of memory" in str(e).lower():
            pytest.skip(f"hipMalloc of two arenas of {case['sizes'][0] * n1 * 4} bytes: {e}")
        raise
    try:
        assert arenas[0].slots * n1 * 4 > 1 << 32
        for st, ar, rows in zip(streams, arenas, init):
            for s, row in zip(tracked, rows):
                st.upload(ar, s, row)
        stage = [0]

        def check():
            stage[0] += 1
            got = [np.stack([st.download(ar, s, 1)[0] for s in tracked]) for st, ar in zip(streams, arenas)]
            _compare(got, want[2 * stage[0]:2 * stage[0] + 2], f"stage {stage[0]} (rows are the tracked slots {tracked})")

        _execute(hip, case, streams, arenas, check=check)
        assert stage[0] == 3
        got = [np.stack([st.download(ar, s, 1)[0] for s in tracked]) for st, ar in zip(streams, arenas)]
        _compare(got, want[:2], "big, final")
    finally:
        ctx.__exit__(None, None, None)
