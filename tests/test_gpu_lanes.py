"""GPU: iyk_hip_gate_batch_lanes — K copies of one circuit's arena image as ONE batch of count x K gates (csrc/lane_jobs.hpp) — against the
path the library had before it: ONE iyk_hip_gate_batch of the host-replicated descriptors (lane_cases.replicate) on a copy of the same
input arena.  The arithmetic is exact and the kernels are the same, so every comparison is of the WHOLE arena, word for word: the lanes'
outputs, their inputs, the slots of a stride that no gate names and the slots behind the last lane, which hold a canary.
Each test initialises and cleans up the library itself."""
import contextlib
import ctypes

import numpy as np
import pytest

import lane_cases as lc
from iyokan_amd import client

pytestmark = pytest.mark.gpu

TAIL = 3      # arena slots behind the last lane


@contextlib.contextmanager
def library(keys, monkeypatch):
    from iyokan_amd import hip

    for v in ("IYK_HIP_NTT", "IYK_HIP_DECOMP", "IYK_HIP_ROT_KERNEL", "IYK_HIP_LATENCY_KERNEL", "IYK_HIP_KS_KERNEL", "IYK_HIP_KS_SHARED_MAX",
              "IYK_HIP_KS_SHARED_WG", "IYK_HIP_DEBUG", "IYK_HIP_COALESCE", "IYK_HIP_KS_MATRIX_MAX_BYTES"):
        monkeypatch.delenv(v, raising=False)
    hip.initialize(keys, device_ids=(0,))
    try:
        yield hip
    finally:
        hip.cleanup()


def canary(slots, n1):
    """a row no kernel produces by accident, different in every slot"""
    return (np.uint32(0xC0DE0000) + np.arange(slots, dtype=np.uint32)[:, None] * np.uint32(977) + np.arange(n1, dtype=np.uint32)[None, :]).astype(np.uint32)


def input_arena(keys, c, seed):
    """lanes * stride + TAIL rows: fresh encryptions of random bits in every lane's input slots — other bits in every lane — and the
    canary everywhere else"""
    n1 = keys.params.n + 1
    slots = c["lanes"] * c["stride"] + TAIL
    rows = canary(slots, n1)
    ins = lc.input_slots(c)
    rng = np.random.default_rng(seed)
    for r in range(c["lanes"]):
        rows[[r * c["stride"] + s for s in ins]] = client.encrypt_bits(keys, rng.integers(0, 2, size=len(ins)).astype(np.uint8), seed=seed * 100 + r)
    return rows


class Run:
    """an arena with the case's input on a stream; lanes() / flat() enqueue, words() synchronises and downloads everything"""

    def __init__(self, hip, st, c, rows):
        self.hip, self.st, self.c = hip, st, c
        self.arena = hip.Arena(len(rows))
        st.upload(self.arena, 0, rows)

    def lanes(self):
        c = self.c
        self.st.gate_batch(self.arena, c["ops"], c["in0"], c["in1"], c["in2"], c["out"], lanes=c["lanes"], lane_stride=c["stride"])
        return self

    def flat(self):
        self.st.gate_batch(self.arena, *lc.replicate(self.c))
        return self

    def words(self):
        self.st.sync()
        got = self.st.download(self.arena, 0, self.arena.slots)
        self.arena.free()
        return got


def written_slots(c):
    return sorted({r * c["stride"] + int(o) for r in range(c["lanes"]) for o in c["out"]})


def check_against_flat(hip, st, keys, c, seed):
    rows = input_arena(keys, c, seed)
    got = Run(hip, st, c, rows).lanes().words()
    want = Run(hip, st, c, rows).flat().words()
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert len(diff) == 0, (c["name"], "first differing slot", int(diff[0]), "of", len(diff))
    untouched = np.setdiff1d(np.arange(len(rows)), written_slots(c))
    assert np.array_equal(got[untouched], rows[untouched]), c["name"]              # inputs and canaries are what was uploaded
    out = written_slots(c)
    assert not np.array_equal(got[out], rows[out])                                 # and the outputs were written
    return got, rows


def test_word_for_word_against_the_flat_batch(keys128, monkeypatch):
    with library(keys128, monkeypatch) as hip:
        st = hip.Stream(0)
        for i, name in enumerate(lc.GPU_CASES):
            got, rows = check_against_flat(hip, st, keys128, lc.CASES[name], seed=40 + i)
        # the last case (37 x 7) also in plain bits, lane by lane: every lane computed ITS inputs' gates
        c = lc.CASES[lc.GPU_CASES[-1]]
        from iyokan_amd.frontier import PlainBitBackend

        for r in range(c["lanes"]):
            lane = slice(r * c["stride"], r * c["stride"] + c["used"])
            be = PlainBitBackend(c["used"])
            ins = lc.input_slots(c)
            be.write_many(ins, client.decrypt_bits(keys128, rows[lane][ins]))
            be.gate_batch(c["ops"], c["in0"], c["in1"], c["in2"], c["out"])
            assert list(client.decrypt_bits(keys128, got[lane][c["out"]])) == be.read_many(list(c["out"])), r
        st.destroy()


def test_one_case_at_the_80_bit_set(keys80, monkeypatch):
    with library(keys80, monkeypatch) as hip:
        st = hip.Stream(0)
        check_against_flat(hip, st, keys80, lc.CASES["mux-3"], seed=80)
        st.destroy()


THRESHOLDS = [
    lc.wide("rot-narrow-to-round", 641, 2),       # 641 rotations: the narrow-frontier kernel; 1 282: one partial round of the wave-per-rotation kernel
    lc.wide("rot-full-round", 1025, 2),           # 2 050: a full round of 2 048 and a narrow remainder of 2
    lc.wide("ks-shared-to-table", 1025, 4),       # 1 025 key switches: the shared-gates form; 4 100 > 4 096: the table
    lc.wide("ks-matrix", 1152, 4),                # 4 608: the matrix form starts
]


@pytest.mark.parametrize("c", THRESHOLDS, ids=[c["name"] for c in THRESHOLDS])
def test_dispatch_thresholds(keys128, monkeypatch, c):
    """per lane below, in total at or above a threshold of dispatch.hpp (tests/test_lane_jobs.py::test_the_threshold_cases_straddle
    holds the figures on 256 CUs): the lane batch runs what the flat batch of the same total runs, and gives its words"""
    with library(keys128, monkeypatch) as hip:
        st = hip.Stream(0)
        check_against_flat(hip, st, keys128, c, seed=90)
        st.destroy()


def test_stream_behaviour(keys128, monkeypatch):
    with library(keys128, monkeypatch) as hip:
        small, big, one = lc.CASES["mux-3"], lc.CASES["37x7"], lc.CASES["every-op-1"]
        rows_small, rows_big, rows_one = input_arena(keys128, small, 61), input_arena(keys128, big, 62), input_arena(keys128, one, 63)
        st, st2, ref = hip.Stream(0), hip.Stream(0), hip.Stream(0)
        want_small, want_big = Run(hip, ref, small, rows_small).flat().words(), Run(hip, ref, big, rows_big).flat().words()
        # two lane batches queued on ONE fresh stream, nothing synchronised in between: the second grows the expansion scratch (and the
        # rotation buffer) behind the first
        a, b = Run(hip, st, small, rows_small), Run(hip, st, big, rows_big)
        a.lanes()
        b.lanes()
        assert np.array_equal(b.words(), want_big) and np.array_equal(a.words(), want_small)
        # and the first again on the grown buffers, twice in a row on one arena: the second pass reads what the first wrote
        twice, twice_ref = Run(hip, st, small, rows_small).lanes().lanes(), Run(hip, ref, small, rows_small).flat().flat()
        assert np.array_equal(twice.words(), twice_ref.words())
        # two streams at once
        a, b = Run(hip, st, big, rows_big), Run(hip, st2, small, rows_small)
        a.lanes()
        b.lanes()
        assert np.array_equal(a.words(), want_big) and np.array_equal(b.words(), want_small)
        # lanes = 1 through the new entry point: the words of iyk_hip_gate_batch
        assert one["lanes"] == 1
        assert np.array_equal(Run(hip, st, one, rows_one).lanes().words(), Run(hip, ref, one, rows_one).flat().words())
        for s in (st, st2, ref):
            s.destroy()


def test_refusals_on_the_device(keys128, monkeypatch):
    """every refusal of the CPU list: IYK_ERR_INVALID with its text, nothing enqueued, the arena as it was"""
    with library(keys128, monkeypatch) as hip:
        st = hip.Stream(0)
        n1 = keys128.params.n + 1
        rows = canary(64, n1)
        arena = hip.Arena(64)
        st.upload(arena, 0, rows)
        L = hip.lib()
        p = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        for name, desc, arena_slots, lanes, stride, word in lc.REFUSALS:
            keep = [np.ascontiguousarray(a, dtype=np.int32) for a in desc]
            # arena_slots is what the caller states: a refusal comes before anything reads it
            rc = L.iyk_hip_gate_batch_lanes(st.h, arena.ptr, arena_slots, len(keep[0]), *[p(a) for a in keep], lanes, stride)
            assert rc == lc.INVALID and word in L.iyk_hip_last_error().decode(), (name, rc, L.iyk_hip_last_error())
            cpu = lc.lane_args(desc, arena_slots, lanes, stride)
            assert (rc, L.iyk_hip_last_error().decode()) == cpu[:2], name                    # the mirror's answer
        with pytest.raises(hip.IykHipError, match="lanes is zero"):
            st.gate_batch(arena, *lc._G, lanes=0, lane_stride=11)
        st.sync()
        assert np.array_equal(st.download(arena, 0, 64), rows)
        arena.free()
        st.destroy()


class SeededEngine:
    """mixin over runner.CipherEngine: the ciphertexts of a lane depend on (seed_lane(lane), how many writes the lane has seen) alone, so
    that a single-lane run can be fed the SAME ciphertexts as lane r of a laned run"""

    def seeded(self, keys, seed_lane):
        self._keys, self._seed_lane, self._writes = keys, seed_lane, {}
        return self

    def set_nodes(self, nids, bits, lane=0):
        if len(nids):
            key = self._seed_lane(lane)
            n = self._writes[key] = self._writes.get(key, 0) + 1
            self.encrypt = lambda b: client.encrypt_bits(self._keys, b, seed=1000003 * (key + 1) + n)
        super().set_nodes(nids, bits, lane=lane)


@pytest.mark.parametrize("blueprint,req,cycles", [("counter-4bit.toml", "test13.in", 3), ("mux-ram-addr8bit.toml", "test06.in", 3)],
                         ids=["counter-4bit", "mux-ram-addr8bit"])
def test_run_packets_under_real_keys(keys128, monkeypatch, blueprint, req, cycles):
    """K = 3 requests in one run: every result decrypts to the plaintext engine's packet, and lane r's arena holds, word for word, what a
    single-lane run_packet of request r fed the same input ciphertexts leaves"""
    import copy

    import torch

    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend
    from iyokan_amd.packet import PlainPacket
    from iyokan_amd.runner import CipherEngine, run_packet, run_packets
    from iyokan_amd.system import load_blueprint
    from netlist_util import gold

    class Engine(SeededEngine, CipherEngine):
        pass

    K = 3
    sysm = load_blueprint(gold(blueprint))
    base = PlainPacket.load(gold(req))
    reqs = [base, copy.deepcopy(base), copy.deepcopy(base)]
    for port, stream in reqs[1].bits.items():
        reqs[1].bits[port] = stream[1:] + stream[:1]
    for ram, image in reqs[2].ram.items():
        reqs[2].ram[ram] = [1 - b for b in image]
    want = [run_packet(sysm, r, cycles=cycles) for r in reqs]                                   # the plaintext engine
    plan = FrontierPlan(sysm.nl, 1)
    dec, zero = (lambda rows: client.decrypt_bits(keys128, rows)), client.trivial(keys128.params, 0)
    with library(keys128, monkeypatch):
        dev = torch.device("cuda", 0)
        be = HipBackend(plan.num_slots, keys128.params, dev, lanes=K)
        eng = Engine(FrontierExecutor(plan, be), None, dec, zero, lanes=K).seeded(keys128, lambda lane: lane)
        got = run_packets(sysm, reqs, cycles=cycles, engine=eng)
        be.sync()
        lanes_arena = be.arena.cpu().numpy().view(np.uint32).reshape(K, plan.num_slots, -1)
        be.close()
        for r in range(K):
            assert got[r].same_content(want[r]), (r, got[r].diff(want[r]))
        for r in range(K):
            be1 = HipBackend(plan.num_slots, keys128.params, dev)
            eng1 = Engine(FrontierExecutor(plan, be1), None, dec, zero).seeded(keys128, lambda lane, r=r: r)
            alone = run_packet(sysm, reqs[r], cycles=cycles, engine=eng1)
            be1.sync()
            words = be1.arena.cpu().numpy().view(np.uint32)
            be1.close()
            assert alone.same_content(want[r])
            assert np.array_equal(lanes_arena[r], words), (r, int(np.nonzero((lanes_arena[r] != words).any(axis=1))[0][0]))
