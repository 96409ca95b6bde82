"""CPU: cmux.Rom / cmux.Ram with lanes on recording streams — what a laned memory enqueues.  The CMUX lists stay ONE lane's and carry
lanes / sel_stride / row_stride (expanded on the device, csrc/cmux_lane_jobs.hpp; here through the emulation of tests/cmux_lane_cases.py);
the flat arrays of the extraction, MUXwoSE, the add and the refresh are lane 0's replicated lane-major.  One lane: the calls of a memory
without the argument (tests/test_cmux_tree_emulation.py holds those against the lists).  Further down the engines: run_packets with
ports on StagedBitsEngine(lanes=3), and runner.CmuxLaneEngine on the recording rig of tests/test_cmux_stage_cb.py — two lanes with
stage_cb, and one lane against the digest that file holds from the commit before CMUX memories had lanes."""
import numpy as np
import pytest

import cmux_lane_cases as cc
from iyokan_amd import cmux

N, MU = 1024, 1 << 29
FAMILY = {name: f for f, name in cc.FAMILY_NAME.items()}


class Recorder:
    """a stream that writes down its calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name,) + tuple(np.asarray(a).tolist() if isinstance(a, (np.ndarray, list, tuple)) else a for a in args) + ((kw,) if kw else ()))
        return call


class Store:
    def __init__(self, slots):
        self.slots, self.ptr = slots, "ptr"

    def __eq__(self, other):
        return isinstance(other, Store)   # the stores of two recordings stand for each other; their sizes are compared where they matter


def _rom(aw, lw, max_reads, lanes=1, sel_base=0, sel_stride=None, arena_stride=None):
    """a cmux.Rom without its device stores, on a recording stream"""
    rom = object.__new__(cmux.Rom)
    rom.stream, rom.addr_width, rom.N, rom.max_reads, rom.word_bits = Recorder(), aw, N, max_reads, 1 << lw
    rom.layout, rom.plan = cmux.rom_layout(aw, lw, N), cmux.rom_read_plan(aw, lw, N)
    rom.sel_base, rom.lanes, rom.arena_stride = sel_base, lanes, arena_stride
    rom.sel_stride = aw * max_reads if sel_stride is None else sel_stride
    rom.row_stride = rom.layout.data_rows + max_reads * rom.layout.scratch_rows
    rom.trgsw, rom.trlwe = "selectors", "rows"
    return rom


def _ram(aw, dw, lanes=1, sel_base=0, sel_stride=None, arena_stride=None):
    ram = object.__new__(cmux.Ram)
    ram.stream, ram.addr_width, ram.data_width, ram.N, ram.mu, ram.cells_per_plane = Recorder(), aw, dw, N, MU, 1 << aw
    ram.layout, ram.plan = cmux.ram_layout(aw, N), cmux.ram_read_plan(aw, N)
    ram.ncells, ram.plane_scratch = dw << aw, ram.layout.scratch_rows + 2
    ram.acc0 = ram.ncells + dw * ram.plane_scratch
    ram.row_stride = ram.acc0 + ram.ncells
    ram.sel_base, ram.lanes, ram.arena_stride = sel_base, lanes, arena_stride
    ram.sel_stride = aw if sel_stride is None else sel_stride
    ram.trgsw, ram.trlwe, ram.arena = "selectors", Store(lanes * ram.row_stride), "cells"
    return ram


def _cmux_calls(calls):
    return [c for c in calls if c[0] in FAMILY]


def _flat(call, trgsw_slots, trlwe_slots):
    """a recorded CMUX call as the flat job list of all its lanes: the emulated expansion of its one-lane list"""
    kw = call[-1] if isinstance(call[-1], dict) else {}
    arrays = call[3:-1] if kw else call[3:]
    f = FAMILY[call[0]]
    code, text, (jobs, steps), _ = cc.lanes_args(f, arrays, trgsw_slots, trlwe_slots, kw.get("lanes", 1), kw.get("sel_stride") or 0, kw.get("row_stride") or 0)
    assert code == cc.OK, text
    if kw.get("lanes", 1) == 1:
        return jobs, steps
    return cc.expand(f, jobs, steps, kw["lanes"], kw["sel_stride"], kw["row_stride"])


@pytest.mark.parametrize("kw", [{}, dict(fused=True), dict(fused=True, fused_tree=True)], ids=["unfused", "fused", "fused_tree"])
@pytest.mark.parametrize("sel_base,sel_stride", [(0, None), (5, 3)], ids=["own-store", "stage-major"])
def test_rom_lanes_enqueue_one_lanes_lists_and_replicated_flat_arrays(kw, sel_base, sel_stride):
    aw, lw, reads, K, A = 9, 3, 1, 3, 40
    wb = 1 << lw
    slots = np.arange(reads * wb).reshape(reads, wb)
    one = _rom(aw, lw, reads, sel_base=sel_base)
    one.read(None, "arena", slots, resident=True, **kw)
    rom = _rom(aw, lw, reads, lanes=K, sel_base=sel_base, sel_stride=sel_stride, arena_stride=A)
    rom.read(None, "arena", slots, resident=True, **kw)
    S, R = rom.sel_stride, rom.row_stride
    assert len(rom.stream.calls) == len(one.stream.calls)
    stride = dict(lanes=K, sel_stride=S, row_stride=R)
    for got, want in zip(_cmux_calls(rom.stream.calls), _cmux_calls(one.stream.calls)):
        assert got == want + (stride,)                                                     # ONE lane's lists, and the strides
    # lane r's words are a one-lane ROM's at its offsets: the expansion against the one-lane lists moved by hand
    trgsw_slots, trlwe_slots = sel_base + (K - 1) * S + aw * reads, K * R
    for got, want in zip(_cmux_calls(rom.stream.calls), _cmux_calls(one.stream.calls)):
        f = FAMILY[got[0]]
        flat = cc.parent_lists(f, cc.replicate(f, want[3:], K, S, R), trgsw_slots, trlwe_slots)
        assert flat[0] == cc.OK, flat[1]
        assert all(np.array_equal(a, b) for a, b in zip(_flat(got, trgsw_slots, trlwe_slots), flat[2]))
    ex, ex1 = rom.stream.calls[-1], one.stream.calls[-1]
    assert ex[0] == ex1[0] == "sample_extract_index_keyswitch_batch"
    assert ex[2] == [r + k * R for k in range(K) for r in ex1[2]] and ex[3] == ex1[3] * K and ex[4] == [s + k * A for k in range(K) for s in ex1[4]]


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_ram_lanes_enqueue_one_lanes_lists_and_replicated_flat_arrays(fused):
    aw, dw, K, A = 3, 2, 2, 11
    wren, wdata, rdata = 0, [1, 2], [3, 4]
    one = _ram(aw, dw)
    one.clock(None, "arena", wren, wdata, rdata, fused=fused, resident=True, fused_tree=fused)
    ram = _ram(aw, dw, lanes=K, arena_stride=A)
    ram.clock(None, "arena", wren, wdata, rdata, fused=fused, resident=True, fused_tree=fused)
    R, C = ram.row_stride, ram.ncells
    assert [c[0] for c in ram.stream.calls] == [c[0] for c in one.stream.calls]
    stride = dict(lanes=K, sel_stride=aw, row_stride=R)
    for got, want in zip(_cmux_calls(ram.stream.calls), _cmux_calls(one.stream.calls)):
        assert got == want + (stride,)
        f = FAMILY[got[0]]
        flat = cc.parent_lists(f, cc.replicate(f, want[3:], K, aw, R), K * aw, K * R)
        assert flat[0] == cc.OK and all(np.array_equal(a, b) for a, b in zip(_flat(got, K * aw, K * R), flat[2]))

    def lanes_of(a, s):
        return [x + k * s if x >= 0 else x for k in range(K) for x in a]

    by = lambda calls, name: [c for c in calls if c[0] == name]
    (ex_r, ex_c), (ex_r1, ex_c1) = by(ram.stream.calls, "sample_extract_index_keyswitch_batch"), by(one.stream.calls, "sample_extract_index_keyswitch_batch")
    assert (ex_r[2], ex_r[4]) == (lanes_of(ex_r1[2], R), lanes_of(ex_r1[4], A))                  # rdata: rows + r R, arena slots + r A
    assert (ex_c[2], ex_c[4], ex_c[5]) == (lanes_of(ex_c1[2], R), list(range(K * C)), "cells")   # refresh: lane r's private slots r C ..
    (mux, back), (mux1, back1) = by(ram.stream.calls, "bootstrap_trlwe_batch"), by(one.stream.calls, "bootstrap_trlwe_batch")
    assert (mux[2], mux[3]) == (lanes_of(mux1[2], A), lanes_of(mux1[3], A)) and mux[4:7] == tuple(a * K for a in mux1[4:7])
    out = lambda call: np.asarray(call[-1]["trlwe_out"]).tolist()
    assert out(mux) == lanes_of(out(mux1), R) and mux[-1]["trlwe_slots"] == K * R
    assert back[2] == list(range(K * C)) and back[3] == [-1] * (K * C) and out(back) == lanes_of(list(range(C)), R)
    add, add1 = by(ram.stream.calls, "trlwe_add_batch")[0], by(one.stream.calls, "trlwe_add_batch")[0]
    assert add[2:5] == tuple(lanes_of(a, R) for a in add1[2:5]) and add[5] == add1[5] == MU


def test_what_cannot_hold_is_refused_before_anything_is_allocated(monkeypatch):
    from iyokan_amd import hip

    class P:
        N = 1024
        mu = MU

    monkeypatch.setattr(hip, "current_params", lambda: P)
    made = []
    monkeypatch.setattr(hip, "Trlwe", lambda *a, **k: made.append("trlwe"))
    monkeypatch.setattr(hip, "Trgsw", lambda *a, **k: made.append("trgsw"))
    monkeypatch.setattr(hip, "Arena", lambda *a, **k: made.append("arena"))
    lay = cmux.rom_layout(9, 3, 1024)
    data = np.zeros((lay.data_rows, 2048), dtype=np.uint32)
    cells = np.zeros((2 << 3, 2048), dtype=np.uint32)
    st = Recorder()
    with pytest.raises(ValueError, match="needs arena_stride"):
        cmux.Rom(st, data, 9, 3, lanes=2)
    with pytest.raises(ValueError, match="needs arena_stride"):
        cmux.Ram(st, cells, 3, 2, lanes=2)
    with pytest.raises(ValueError, match="for 2 lanes, the store has 17"):          # 9 + 9 slots needed
        cmux.Rom(st, data, 9, 3, trgsw=Store(17), lanes=2, arena_stride=8)
    with pytest.raises(ValueError, match="for 3 lanes, the store has 12"):          # stage-major: base 5, stride 3: 5 + 6 + 3 = 14 slots
        cmux.Ram(st, cells, 3, 2, trgsw=Store(12), sel_base=5, sel_stride=3, lanes=3, arena_stride=8)
    with pytest.raises(ValueError, match="at least one"):
        cmux.Ram(st, cells, 3, 2, lanes=0)
    assert made == [] and st.calls == []


def test_lane_flat():
    assert cmux.lane_flat([3, -1, 5], 2, 10).tolist() == [3, -1, 5, 13, -1, 15]
    assert cmux.lane_flat([3, -1], 1, 10).tolist() == [3, -1] and cmux.lane_tile([1, 2], 3).tolist() == [1, 2, 1, 2, 1, 2]


# ---- engines: run_packets with ports -------------------------------------------------------------------------------------------------

import copy

import cmux_stage_cases as stage_cases
import test_cmux_stage_cb as rigs
from iyokan_amd import runner
from iyokan_amd.frontier import FrontierExecutor, FrontierPlan
from iyokan_amd.packet import PlainPacket
from iyokan_amd.system import load_blueprint
from netlist_util import gold


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """DESIGN.md section 6e's hand-built system: a ROM and three RAMs in three stages"""
    return load_blueprint(stage_cases.write_blueprint(str(tmp_path_factory.mktemp("cmux_lanes_stage"))), cmux_memories=True)


def _ram8_requests():
    base = PlainPacket.load(gold("test06.in"))
    reqs = [copy.deepcopy(base) for _ in range(3)]
    rng = np.random.default_rng(5)
    for r, req in enumerate(reqs[1:], 1):                      # other RAM images and other input streams
        for name in req.ram:
            req.ram[name] = [int(b) for b in rng.integers(0, 2, size=len(req.ram[name]))]
        for name in req.bits:
            req.bits[name] = [int(b) for b in rng.integers(0, 2, size=len(req.bits[name]))]
    return reqs


def test_run_packets_on_staged_bits_engine_equals_run_packet_per_request(four):
    """K = 3 lanes of ports: result r is run_packet(requests[r]) on a one-lane engine; the requests differ in ROM image, RAM images and
    (ram-addr8bit) inputs; one changed ROM bit changes its own lane's result only"""
    reqs = [stage_cases.request(seed, 5) for seed in (1, 2, 3)]
    assert reqs[0].rom != reqs[1].rom and reqs[0].ram != reqs[2].ram
    want = [runner.run_packet(four, r, engine=runner.StagedBitsEngine(four)) for r in reqs]
    got = runner.run_packets(four, reqs, engine=runner.StagedBitsEngine(four, lanes=3))
    assert all(w.same_content(g) for w, g in zip(want, got)), [w.diff(g) for w, g in zip(want, got)]
    assert not want[0].same_content(want[1])
    changed = None
    for bit in range(len(reqs[1].rom["rom"])):                 # a ROM bit of lane 1 that matters to its result
        trial = copy.deepcopy(reqs)
        trial[1].rom["rom"][bit] ^= 1
        if not runner.run_packet(four, trial[1], engine=runner.StagedBitsEngine(four)).same_content(want[1]):
            changed = trial
            break
    assert changed is not None
    again = runner.run_packets(four, changed, engine=runner.StagedBitsEngine(four, lanes=3))
    assert want[0].same_content(again[0]) and want[2].same_content(again[2]) and not want[1].same_content(again[1])

    sysm = load_blueprint(gold("ram-addr8bit.toml"), cmux_memories=True)
    reqs = _ram8_requests()
    want = [runner.run_packet(sysm, r, cycles=16, engine=runner.StagedBitsEngine(sysm)) for r in reqs]
    got = runner.run_packets(sysm, reqs, cycles=16, engine=runner.StagedBitsEngine(sysm, lanes=3))
    assert all(w.same_content(g) for w, g in zip(want, got)) and want[0].same_content(PlainPacket.load(gold("test06.out")))
    assert not want[0].same_content(want[1])


def test_run_packets_still_refuses_ports_without_port_lanes(four):
    reqs = [stage_cases.request(1, 2), stage_cases.request(2, 2)]
    text = "a system with CMUX memory ports runs one request at a time: CMUX memories have no lanes"
    with pytest.raises(ValueError, match=text):
        runner.run_packets(four, reqs)
    with pytest.raises(ValueError, match=text):
        runner.run_packets(four, reqs, engine=runner.PlainEngine(four.nl, lanes=2))
    assert not getattr(runner.CmuxCipherEngine, "port_lanes", False) and runner.CmuxLaneEngine.port_lanes and runner.StagedBitsEngine.port_lanes
    with pytest.raises(ValueError, match="2 request packets for an engine with 3 lanes"):
        runner.run_packets(four, reqs, engine=runner.StagedBitsEngine(four, lanes=3))


class _LaneBackend(rigs._Backend):
    """the recording backend with lanes: lane r's slots + r * num_slots"""

    def __init__(self, rig, num_slots, lanes):
        self.stream, self._arena = rigs._Stream(rig), rigs._Store(rig, "Arena", lanes * num_slots, int(rigs.P.n) + 1)
        self.lanes, self.lane_stride = lanes, num_slots

    def gate_batch(self, ops, in0, in1, in2, out):
        if len(ops):
            self.stream.gate_batch(self._arena, ops, in0, in1, in2, out, lanes=self.lanes, lane_stride=self.lane_stride)

    def write_many(self, slots, rows, lane=0):
        self.stream.upload_slots(self._arena, [int(s) + lane * self.lane_stride for s in slots])

    def read_many(self, slots, lane=0):
        return np.zeros((len(slots), int(rigs.P.n) + 1), dtype=np.uint32)


def _lane_engine(monkeypatch, sysm, K, **kw):
    rig = rigs._Rig(monkeypatch)
    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    be = _LaneBackend(rig, plan.num_slots, K)
    n1 = int(rigs.P.n) + 1
    eng = runner.CmuxLaneEngine(sysm, FrontierExecutor(plan, be), lambda bits: np.zeros((len(bits), n1), dtype=np.uint32),
                                lambda rows: [0] * len(rows), np.zeros(n1, dtype=np.uint32), rigs._Key("bk2", int(rigs.P.n)), rigs._Key("pk"),
                                packets=[rigs._Packet(sysm) for _ in range(K)], decrypt_ram=lambda rows: [0] * len(rows), **kw)
    return eng, rig, plan


@pytest.mark.parametrize("fused", [False, True])
def test_two_lanes_with_stage_cb_is_one_batch_per_stage_into_stage_major_slots(monkeypatch, four, fused):
    K, L, PER = 2, rigs.L, rigs.PER
    eng, rig, plan = _lane_engine(monkeypatch, four, K, stage_cb=True, rom_fused=fused, tree_fused=fused, refresh_aside=fused)
    rigs._clocks(eng, four)
    slot, S = plan.slot, plan.num_slots
    # stage-major: the stage of the ROM and two RAMs (3 + 1 + 2 bits) owns 2 x 6 slots, the last RAM's stage 2 x 1 behind them
    assert [eng.mem[n].sel_base for _, n, _, _ in stage_cases.PORTS] == [0, 3, 4, 12] and eng.trgsw.slots == K * 7
    assert [eng.mem[n].sel_stride for _, n, _, _ in stage_cases.PORTS] == [6, 6, 6, 1]
    assert eng.tlwe2.slots == K * 6 * L and eng.scratch.slots == K * 6 * PER
    batches = [c for c in rig.log if c[1] == "circuit_bootstrap_batch"]
    assert len(batches) == 4 * 2                                                    # two stages with ports, four run()s: as with one lane
    stages = sorted({pt.stage for pt in four.ports})
    for k, (_, _, args, _) in enumerate(batches):
        pts = [pt for pt in four.ports if pt.stage == stages[k % 2]]
        one = [slot[a] for pt in pts for a in pt.addr]
        assert args[3] == [s + r * S for r in range(K) for s in one], k               # all lanes, all ports of the stage, lane-major
        assert args[8] is eng.trgsw and args[9] == eng.mem[pts[0].name].sel_base and args[6] == 0
    # every CMUX call names ONE lane's selector slots inside its port's, and the strides
    owner = {eng.mem[pt.name].trlwe: pt for pt in four.ports}
    for _, name, args, kw in rig.log:
        if name in rigs.SEL_POS:
            pt, mem = owner[args[1]], eng.mem[owner[args[1]].name]
            assert set(rigs._selectors(name, args)) <= set(range(mem.sel_base, mem.sel_base + pt.addr_width))
            assert dict(kw) == dict(lanes=K, sel_stride=mem.sel_stride, row_stride=mem.row_stride)
    eng.free()


def test_one_lane_engines_enqueue_the_parents_calls(monkeypatch, four):
    """CmuxLaneEngine on a one-lane backend, and CmuxCipherEngine, against the digest recorded from the commit before CMUX memories had
    lanes (tests/test_cmux_stage_cb.py: three clocks, the memories' constructor uploads and image loads included)"""
    eng, rig = rigs._engine(monkeypatch, four)
    rigs._clocks(eng, four)
    eng.free()
    assert rigs._digest(rig.log) == rigs.PARENT_DIGEST
    rig = rigs._Rig(monkeypatch)
    plan = FrontierPlan(four.nl, 1, stages=four.stages)
    n1 = int(rigs.P.n) + 1
    eng = runner.CmuxLaneEngine(four, FrontierExecutor(plan, rigs._Backend(rig, plan.num_slots)), lambda bits: np.zeros((len(bits), n1), dtype=np.uint32),
                                lambda rows: [0] * len(rows), np.zeros(n1, dtype=np.uint32), rigs._Key("bk2", int(rigs.P.n)), rigs._Key("pk"),
                                packets=[rigs._Packet(four)], decrypt_ram=lambda rows: [0] * len(rows))
    rigs._clocks(eng, four)
    eng.free()
    assert rigs._digest(rig.log) == rigs.PARENT_DIGEST


def test_lane_engine_refusals(monkeypatch, four):
    with pytest.raises(ValueError, match="1 packets for a backend with 2 lanes"):
        rig = rigs._Rig(monkeypatch)
        plan = FrontierPlan(four.nl, 1, stages=four.stages)
        runner.CmuxLaneEngine(four, FrontierExecutor(plan, _LaneBackend(rig, plan.num_slots, 2)), None, None, None, rigs._Key("bk2", int(rigs.P.n)),
                              rigs._Key("pk"), packets=[None])
    monkeypatch.setattr(runner, "MAX_CB_BATCH", 6 * rigs.L * 2 - 1)
    with pytest.raises(ValueError, match="more than the"):
        _lane_engine(monkeypatch, four, 2, stage_cb=True)
