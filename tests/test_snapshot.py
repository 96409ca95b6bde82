"""CPU: snapshot and resume of a run (iyokan_amd/snapshot.py, runner.run_packet / run_packets(snapshot_path=, snapshot_every=, resume=)).

The engines are deterministic, so a run that is split — some clocks, state() -> save -> load -> a NEW engine, load_state, the rest —
has to give the packets of the straight run, and every mistake in what is saved or restored has to show as another packet.  The system
is the four-stage one of tests/cmux_system_cases.py (counter in DFFs -> ROM 3 x 4 -> logic -> RAM 2 x 2, wdata from the RAM's own
rdata) with a two-bit @in mixed into the RAM's address and write data, so that the circular input streams matter.  The cipher engines
run on the recording rig of tests/test_cmux_stage_cb.py / tests/test_read_early_engine.py: a wait_stream is an ordering edge."""
import json
import os
import shutil

import numpy as np
import pytest

import cmux_stage_cases as stage_cases
import cmux_system_cases as small
import read_early_cases
import test_cmux_stage_cb as rigs
import test_read_early_engine as early
from iyokan_amd import cmux, netlist, runner, snapshot
from iyokan_amd.packet import PlainPacket
from iyokan_amd.snapshot import Snapshot
from iyokan_amd.system import load_blueprint

SEEDS = range(6)
SPLIT, CLOCKS = 3, 6


# ---- the system: tests/cmux_system_cases.py's, with @in[0:1] ----------------------------------------------------------------------------

def core_json():
    c = small._Core()
    reset = c.inp("reset", 0)
    romd = [c.inp("romd", i) for i in range(4)]
    ramr = [c.inp("ramr", i) for i in range(2)]
    inp = [c.inp("inp", i) for i in range(2)]
    cnt = [c.dff() for _ in range(3)]
    wq, q0, q1 = c.dff(), c.dff(), c.dff()
    nxt = [c.gate("NOT", A=cnt[0]), c.gate("XOR", A=cnt[0], B=cnt[1]), c.gate("XOR", A=cnt[2], B=c.gate("AND", A=cnt[0], B=cnt[1]))]
    for d, x in zip(cnt, nxt):
        c.feed(d, c.gate("ANDNOT", A=x, B=reset))
    for i in range(3):
        c.out("rom_addr", i, cnt[i])
    ra0 = c.gate("XOR", A=romd[0], B=cnt[0])
    ra1 = c.gate("XOR", A=c.gate("XOR", A=romd[1], B=romd[2]), B=inp[0])
    c.out("ram_addr", 0, ra0)
    c.out("ram_addr", 1, ra1)
    c.feed(wq, romd[3])
    c.out("wren", 0, wq)
    wd0, wd1 = c.gate("XOR", A=ramr[0], B=romd[2]), c.gate("XNOR", A=ramr[1], B=c.gate("XOR", A=romd[0], B=inp[1]))
    c.out("wdata", 0, wd0)
    c.out("wdata", 1, wd1)
    c.feed(q0, ramr[0])
    c.feed(q1, ramr[1])
    for i, drv in enumerate([q0, c.gate("XOR", A=q1, B=cnt[2]), wd0, ra1]):
        c.out("out", i, drv)
    return {"ports": c.ports, "cells": c.cells}


def write_blueprint(directory):
    with open(os.path.join(directory, "core.json"), "w") as f:
        json.dump(core_json(), f)
    path = os.path.join(directory, "system.toml")
    with open(path, "w") as f:
        f.write(small.BLUEPRINT + '"core/inp[0:1]" = "@in[0:1]"\n')
    return path


def request(seed, cycles=CLOCKS):
    """a random program: the ROM image, the initial RAM, and an @in stream of 5 bits for a 2-bit port (it wraps inside a clock)"""
    req = small.request(seed, cycles)
    req.bits["in"] = [int(b) for b in np.random.default_rng(1000 + seed).integers(0, 2, size=5)]
    return req


@pytest.fixture(scope="module")
def systems(tmp_path_factory):
    path = write_blueprint(str(tmp_path_factory.mktemp("snapshot")))
    sysm, lowered = load_blueprint(path, cmux_memories=True), load_blueprint(path)
    assert [(pt.kind, pt.addr_width, pt.data_width, pt.stage) for pt in sysm.ports] == [("rom", 3, 4, 0), ("ram", 2, 2, 1)]
    assert sysm.num_stages == 3 and ("in", 1) in sysm.nl.inputs
    return sysm, lowered


def _every_clock(sysm, req, engine, **kw):
    out = []
    res = runner.run_packet(sysm, req, engine=engine, on_cycle=lambda done, eng: out.append(runner.result_packet(sysm, eng, done)), **kw)
    return out, res


@pytest.fixture(scope="module")
def straight(systems):
    """the uninterrupted runs, computed once: per seed the result packet after every clock, StagedBitsEngine's and (equal) PlainEngine's"""
    sysm, lowered = systems
    out = {}
    for seed in SEEDS:
        want, res = _every_clock(sysm, request(seed), runner.StagedBitsEngine(sysm))
        low, _ = _every_clock(lowered, request(seed), runner.PlainEngine(lowered.nl))
        assert len(want) == CLOCKS and res.same_content(want[-1]) and all(a.same_content(b) for a, b in zip(want, low))
        out[seed] = want
    assert sum(out[s][c].ram["ram"] != out[s][c + 1].ram["ram"] for s in SEEDS for c in range(CLOCKS - 1)) >= 6   # the programs do write
    return out


def _split_run(sysm, req, make, path, make_second=None, through_file=True):
    """SPLIT clocks on make()'s engine, its state to `path` and back, then the rest on a NEW engine: the packets after the later clocks"""
    first = make()
    res = runner.run_packet(sysm, req, cycles=SPLIT, engine=first, snapshot_path=path)
    assert res.cycles == SPLIT and not os.path.exists(path + ".tmp")
    snap = Snapshot.load(path)
    assert snap.done == SPLIT and snap.reset_ran and snap == first.state(done=SPLIT, reset_ran=True)
    got, res = _every_clock(sysm, req, (make_second or make)(), cycles=CLOCKS, resume=path if through_file else snap)
    assert res.same_content(got[-1]) and len(got) == CLOCKS - SPLIT
    return got


def _equal(want, got):
    return all(w.same_content(g) and w.ram == g.ram for w, g in zip(want[SPLIT:], got))


# ---- 1. a split run equals the straight run ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("read_early", [False, True])
def test_staged_bits_engine_split_equals_straight(systems, straight, tmp_path, read_early):
    sysm, _ = systems
    for seed in SEEDS:
        got = _split_run(sysm, request(seed), lambda: runner.StagedBitsEngine(sysm, read_early=read_early), str(tmp_path / "s.npz"),
                         through_file=bool(seed & 1))
        assert _equal(straight[seed], got), seed


def test_plain_engine_on_the_lowered_form_split_equals_straight(systems, straight, tmp_path):
    _, lowered = systems
    for seed in SEEDS:
        assert _equal(straight[seed], _split_run(lowered, request(seed), lambda: runner.PlainEngine(lowered.nl), str(tmp_path / "p.npz"))), seed


def test_state_and_load_state_by_hand(systems):
    """without the runners: clock an engine, state(), a new engine, load_state, and both go on in step"""
    sysm, _ = systems
    a = runner.StagedBitsEngine(sysm)
    runner.run_packet(sysm, request(2), cycles=2, engine=a)
    b = runner.StagedBitsEngine(sysm)
    b.load_state(a.state())
    for _ in range(3):
        for eng in (a, b):
            eng.tick()
            eng.run()
        assert a.state() == b.state() and a.ram_image("ram") == b.ram_image("ram")


def _lanes_split(sysm, make, reqs, path, make_second=None):
    runner.run_packets(sysm, reqs, cycles=SPLIT, engine=make(), snapshot_path=path, snapshot_every=2)   # saved after clock 2, then after the last
    assert Snapshot.load(path).done == SPLIT and Snapshot.load(path).lanes == len(reqs)
    return runner.run_packets(sysm, reqs, cycles=CLOCKS, engine=(make_second or make)(), resume=path)


@pytest.mark.parametrize("which", ["staged", "plain"])
def test_three_lanes_through_run_packets(systems, straight, tmp_path, which):
    sysm, lowered = systems
    reqs = [request(seed) for seed in (0, 1, 2)]
    if which == "staged":
        got = _lanes_split(sysm, lambda: runner.StagedBitsEngine(sysm, lanes=3), reqs, str(tmp_path / "l.npz"))
    else:
        got = _lanes_split(lowered, lambda: runner.PlainEngine(lowered.nl, lanes=3), reqs, str(tmp_path / "l.npz"))
    for seed, g in zip((0, 1, 2), got):                                             # each lane: that request run alone, no snapshot
        assert straight[seed][-1].same_content(g), (seed, straight[seed][-1].diff(g))
    assert not got[0].same_content(got[1])


# ---- 2. until @finflag, from a resume ----------------------------------------------------------------------------------------------------

def finflag_netlist():
    """a 3-bit counter behind @reset that raises @finflag when it holds 4: after clock 5"""
    nl = netlist.Netlist()
    reset = nl.add("INPUT")
    nl.inputs[("reset", 0)] = reset
    cnt = [nl.add("DFF", [0]) for _ in range(3)]
    nxt = [nl.add("NOT", [cnt[0]]), nl.add("XOR", [cnt[0], cnt[1]]), nl.add("XOR", [cnt[2], nl.add("AND", [cnt[0], cnt[1]])])]
    for d, x in zip(cnt, nxt):
        nl.ins[d] = [nl.add("ANDNOT", [x, reset])]
    fin = nl.add("ANDNOT", [nl.add("ANDNOT", [cnt[2], cnt[1]]), cnt[0]])
    nl.outputs[("finflag", 0)] = nl.add("OUTPUT", [fin])
    for i in range(3):
        nl.outputs[("cnt", i)] = nl.add("OUTPUT", [cnt[i]])
    nl.validate()
    return nl


def test_run_until_finflag_from_a_resume(tmp_path):
    nl, path = finflag_netlist(), str(tmp_path / "f.npz")
    want = runner.run_packet(nl, PlainPacket(), cycles=-1)
    assert want.cycles == 5 and want.bits["cnt"] == [0, 0, 1]
    runner.run_packet(nl, PlainPacket(), cycles=2, snapshot_path=path)
    got = runner.run_packet(nl, PlainPacket(), cycles=-1, resume=path)
    assert got.cycles == 5 and want.same_content(got)
    # snapshot_every on the way: the file after the run is the last clock's, and a resume from it has nothing left to do
    runner.run_packet(nl, PlainPacket(), cycles=-1, resume=path, snapshot_path=path, snapshot_every=2)
    assert Snapshot.load(path).done == 5
    again = runner.run_packet(nl, PlainPacket(), cycles=-1, resume=path)
    assert again.cycles == 5 and want.same_content(again)


# ---- 3. mutants: each has to give other packets than the straight run -----------------------------------------------------------------------

class _NoRamCells(runner.StagedBitsEngine):
    """a state without the RAM cells: what comes back is the fresh engine's zeros"""

    def _write_mem(self, pt, lane, image):
        if pt.kind != "ram":
            super()._write_mem(pt, lane, image)


class _NoDffSlots(runner.StagedBitsEngine):
    def _state_slots(self):
        plan = self.ex.plan
        dffs = {plan.slot[i] for i in plan.dffs}
        return [s for s in super()._state_slots() if s not in dffs]


class _ResetAgain(runner.StagedBitsEngine):
    def load_state(self, snap):
        super().load_state(snap)
        reset = [self.nl.inputs[("reset", 0)]]
        self.set_nodes(reset, [1])
        self.run()
        self.set_nodes(reset, [0])


class _LaneOneIntoLaneZero(runner.StagedBitsEngine):
    def load_state(self, snap):
        arena = snap.arena.copy()
        arena[0] = arena[1]
        mems = [{n: np.concatenate([a[1:2], a[1:]]) for n, a in m.items()} for m in (snap.ram, snap.rom)]
        super().load_state(Snapshot(snap.meta, snap.slots, arena, *mems))


@pytest.mark.parametrize("mutant", [_NoRamCells, _NoDffSlots, _ResetAgain])
def test_each_mistake_in_the_state_is_caught(systems, straight, tmp_path, mutant):
    sysm, _ = systems
    ok = [_equal(straight[seed], _split_run(sysm, request(seed), lambda: mutant(sysm), str(tmp_path / "m.npz"))) for seed in SEEDS]
    assert not all(ok), mutant.__name__


def test_input_streams_restarted_at_zero_are_caught(systems, straight, tmp_path, monkeypatch):
    sysm, _ = systems
    real = runner._set_inputs
    resumed = []
    monkeypatch.setattr(runner, "_set_inputs", lambda s, e, r, done: real(s, e, r, done - SPLIT if resumed else done))

    def second():
        resumed.append(True)
        return runner.StagedBitsEngine(sysm)

    ok = []
    for seed in SEEDS:
        del resumed[:]
        ok.append(_equal(straight[seed], _split_run(sysm, request(seed), lambda: runner.StagedBitsEngine(sysm), str(tmp_path / "i.npz"), second)))
    assert not all(ok)


def test_a_lane_restored_into_another_is_caught(systems, straight, tmp_path):
    sysm, _ = systems
    reqs = [request(seed) for seed in (0, 1, 2)]
    got = _lanes_split(sysm, lambda: runner.StagedBitsEngine(sysm, lanes=3), reqs, str(tmp_path / "x.npz"),
                       lambda: _LaneOneIntoLaneZero(sysm, lanes=3))
    assert not straight[0][-1].same_content(got[0]) and straight[1][-1].same_content(got[1]) and straight[2][-1].same_content(got[2])


# ---- 4. refusals: each names what disagrees and leaves the target as it was ---------------------------------------------------------------

class _P128(runner.StagedBitsEngine):
    _state_params = lambda self: dict(n=636, N=1024, k=1, l=3, Bgbit=6, t=7, basebit=2)


class _P80(runner.StagedBitsEngine):
    _state_params = lambda self: dict(n=500, N=1024, k=1, l=2, Bgbit=10, t=8, basebit=2)


class _Cipher(runner.StagedBitsEngine):
    state_kind = "cipher"


def _ran(sysm, cls=runner.StagedBitsEngine, clocks=2, seed=4, **kw):
    eng = cls(sysm.nl if cls is runner.PlainEngine else sysm, **{k: v for k, v in kw.items() if k == "lanes"})
    run_kw = {k: v for k, v in kw.items() if k != "lanes"}
    if kw.get("lanes", 1) > 1:
        runner.run_packets(sysm, [request(seed + r) for r in range(kw["lanes"])], cycles=clocks, engine=eng, **run_kw)
    else:
        runner.run_packet(sysm, request(seed), cycles=clocks, engine=eng, **run_kw)
    return eng


def test_refusals_leave_the_engine_as_it_was(systems, tmp_path):
    sysm, lowered = systems
    other = load_blueprint(read_early_cases.write_blueprint(str(tmp_path)), cmux_memories=True)   # the same memories behind another core
    good = _ran(sysm, clocks=3).state(done=3, reset_ran=True)
    short = Snapshot(good.meta, good.slots, good.arena, {"ram": good.ram["ram"][:, :-1]}, good.rom)
    thin = Snapshot(good.meta, good.slots, good.arena, good.ram, {"rom": good.rom["rom"][:, :-4]})
    no_ram = Snapshot(good.meta, good.slots, good.arena, {}, good.rom)
    cases = [
        (sysm, _ran(sysm, _P80), _ran(sysm, _P128).state(done=2, reset_ran=True), "parameter set"),
        (other, _ran(other), good, "system digest"),
        (lowered, _ran(lowered, runner.PlainEngine), good, "system digest"),
        (sysm, _ran(sysm, lanes=2), good, "1 lanes, this engine has 2"),
        (sysm, _ran(sysm), _ran(sysm, _Cipher).state(done=2, reset_ran=True), "cipher engine"),
        (sysm, _ran(sysm), short, "RAM 'ram'"),
        (sysm, _ran(sysm), thin, "ROM 'rom'"),
        (sysm, _ran(sysm), no_ram, "lacks RAM 'ram'"),
    ]
    for system, eng, snap, text in cases:
        before = eng.state()
        with pytest.raises(ValueError, match=text):
            eng.load_state(snap)
        assert eng.state() == before, text
        with pytest.raises(ValueError, match=text):                                  # ... and through the runners
            if eng.lanes == 1:
                runner.run_packet(system, request(4), cycles=6, engine=eng, resume=snap)
            else:
                runner.run_packets(system, [request(4), request(5)], cycles=6, engine=eng, resume=snap)
        assert eng.state() == before, text
    eng = _ran(sysm)
    before = eng.state()
    path = str(tmp_path / "never.npz")
    with pytest.raises(ValueError, match="cycles = 2 is the total"):
        runner.run_packet(sysm, request(4), cycles=2, engine=eng, resume=good, snapshot_path=path)
    no_reset = _ran(sysm, skip_reset=True).state(done=2, reset_ran=False)
    with pytest.raises(ValueError, match="reset cycle never ran"):
        runner.run_packet(sysm, request(4), cycles=6, engine=eng, resume=no_reset, snapshot_path=path)
    with pytest.raises(ValueError, match="snapshot_every without snapshot_path"):
        runner.run_packet(sysm, request(4), cycles=6, engine=eng, snapshot_every=2)
    with pytest.raises(ValueError, match="snapshot_every without snapshot_path"):
        runner.run_packets(sysm, [request(4)], cycles=6, engine=eng, snapshot_every=2)
    with pytest.raises(ValueError, match="at least 1"):
        runner.run_packet(sysm, request(4), cycles=6, engine=eng, snapshot_path=path, snapshot_every=0)
    with pytest.raises(ValueError, match="holds 1 lanes"):
        runner.run_packets(sysm, [request(4), request(5)], cycles=6, engine=runner.StagedBitsEngine(sysm, lanes=2), resume=good, snapshot_path=path)
    assert eng.state() == before and not os.path.exists(path) and not os.path.exists(path + ".tmp")
    # what the snapshot allows: the reset skipped on both sides
    runner.run_packet(sysm, request(4), cycles=4, engine=runner.StagedBitsEngine(sysm), resume=no_reset, skip_reset=True)


# ---- 5. the file ---------------------------------------------------------------------------------------------------------------------------

def test_the_file(systems, tmp_path, monkeypatch):
    sysm, _ = systems
    eng = _ran(sysm, clocks=3)
    snap, path = eng.state(done=3, reset_ran=True), str(tmp_path / "run.snapshot")
    snap.save(path)
    assert sorted(os.listdir(tmp_path)) == ["run.snapshot"]                         # no .tmp, no .npz appended
    with np.load(path, allow_pickle=False) as z:
        assert z.files[0] == "version" and list(z["version"]) == [snapshot.VERSION]
        assert set(z.files) == {"version", "meta", "slots", "arena", "ram.ram", "rom.rom"} and z["meta"].dtype == np.uint8
        meta = json.loads(bytes(z["meta"]).decode("utf-8"))
        arrays = {k: z[k] for k in z.files}
    assert meta["done"] == 3 and meta["lanes"] == 1 and meta["engine"] == "StagedBitsEngine" and meta["kind"] == "bits" and len(meta["digest"]) == 64
    assert not any("key" in k.lower() for k in list(meta) + list(arrays))
    assert Snapshot.load(path) == snap
    raw = open(path, "rb").read()
    for cut in (len(raw) // 2, len(raw) - 7, 10):
        with open(tmp_path / "cut", "wb") as f:
            f.write(raw[:cut])
        with pytest.raises(ValueError, match="not a complete snapshot"):
            Snapshot.load(str(tmp_path / "cut"))
    with open(tmp_path / "v2", "wb") as f:
        np.savez(f, **dict(arrays, version=np.array([snapshot.VERSION + 1], dtype=np.uint32)))
    with pytest.raises(ValueError, match=f"version {snapshot.VERSION + 1}"):
        Snapshot.load(str(tmp_path / "v2"))
    for gone in ("version", "arena", "ram.ram"):
        with open(tmp_path / "gone", "wb") as f:
            np.savez(f, **{k: v for k, v in arrays.items() if k != gone})
        with pytest.raises(ValueError, match="no version" if gone == "version" else "lacks the array"):
            Snapshot.load(str(tmp_path / "gone"))
    with pytest.raises(ValueError, match="version"):                                 # a resume from such a file touches nothing
        runner.run_packet(sysm, request(4), cycles=6, engine=eng, resume=str(tmp_path / "v2"))
    assert eng.state(done=3, reset_ran=True) == snap
    # a save whose os.replace fails leaves the previous file and no .tmp
    keep = str(tmp_path / "keep")
    shutil.copy(path, keep)
    later = _ran(sysm, clocks=4).state(done=4, reset_ran=True)

    def refuse(src, dst):
        raise OSError("no replace today")

    monkeypatch.setattr(os, "replace", refuse)
    with pytest.raises(OSError, match="no replace today"):
        later.save(path)
    monkeypatch.undo()
    assert open(path, "rb").read() == raw and sorted(os.listdir(tmp_path)) == sorted(["run.snapshot", "cut", "v2", "gone", "keep"])
    later.save(path)
    assert Snapshot.load(path) == later and Snapshot.load(path) != snap


# ---- 6. the cipher engines on recording streams ---------------------------------------------------------------------------------------------

FLAGS = dict(refresh_aside=True, read_early=True, stage_cb=True)


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    return load_blueprint(stage_cases.write_blueprint(str(tmp_path_factory.mktemp("snapshot_four"))), cmux_memories=True)


def _touches(rig, store):
    """the calls that write `store`, as positions in the recording"""
    return [j for j, c in enumerate(rig.log) if ("store", store.serial) in early._access(rig, None, c)[1]]


@pytest.mark.parametrize("cls,lanes", [(runner.CmuxCipherEngine, 1), (runner.CmuxLaneEngine, 2)])
def test_state_is_ordered_behind_the_refresh_and_the_join(monkeypatch, four, cls, lanes):
    eng, rig = early._engine(monkeypatch, four, cls=cls, lanes=lanes, **FLAGS)
    early._clocks(eng, four, rig, n=2)
    eng.tick()
    eng.run()                                                                       # the clock edge: run() done, the next tick() to come
    mark = len(rig.log)
    snap = eng.state(done=3, reset_ran=True)
    assert not [c for c in rig.log[mark:] if c[1] == "sync"]                        # no host synchronisation of its own
    bad = early._races(rig, eng.arena)
    assert not bad, early._show(rig, bad)
    before = rigs._before(rig.log)
    rams = [pt for pt in four.ports if pt.kind == "ram"]
    for pt in four.ports:
        store = eng.mem[pt.name].trlwe
        loads = [j for j in range(mark, len(rig.log)) if rig.log[j][1] == "store_download" and rig.log[j][2][0] is store]
        assert len(loads) == lanes
        for j in loads:                                                             # every writer of the rows, the refresh aside among them
            assert all((before[j] >> i) & 1 for i in _touches(rig, store) if i < j), pt.name
        if pt.kind == "ram":
            assert [i for i in _touches(rig, store) if rig.log[i][0] == eng.refresh_stream.sid]
    assert snap.lanes == lanes and snap.meta["kind"] == "cipher" and snap.meta["params"]["n"] == 636 and sorted(snap.ram) == [pt.name for pt in rams]
    assert snap.arena.shape == (lanes, len(snap.slots), 637) and snap.rom["rom"].shape == (lanes, 1, 2 * rigs.N)
    # a state taken while a refresh is in flight holds the refreshed rows: cells() orders itself behind it
    eng.tick()
    assert all(eng.mem[pt.name].pending_refresh is not None for pt in rams)
    mark = len(rig.log)
    eng.state()
    assert [c[:3] for c in rig.log[mark:] if c[1] == "wait_stream"] == [(eng.port_stream.sid, "wait_stream", [eng.refresh_stream.sid])] * len(rams)
    bad = early._races(rig, eng.arena)
    assert not bad, early._show(rig, bad)
    eng.free()


class _CellsWithoutWait(cmux.Ram):
    def cells(self, lane=0):
        return self.trlwe.download(self.stream, lane * self.row_stride, self.ncells).reshape(self.data_width, self.cells_per_plane, 2 * self.N)


def test_a_state_that_skips_order_refresh_is_caught(monkeypatch, four):
    monkeypatch.setattr(cmux, "Ram", _CellsWithoutWait)
    eng, rig = early._engine(monkeypatch, four, **FLAGS)
    runs = early._clocks(eng, four, rig, n=1)
    del runs
    rig.log[:] = [c for c in rig.log if c[1] != "store_download"]                    # _clocks read the cells, without the wait: not the subject
    assert not early._races(rig, eng.arena)
    eng.tick()
    eng.state()
    bad = early._races(rig, eng.arena)
    assert bad and all(rig.log[j][1] == "store_download" for _, j, _ in bad)


@pytest.mark.parametrize("cls,lanes", [(runner.CmuxCipherEngine, 1), (runner.CmuxLaneEngine, 2)])
@pytest.mark.parametrize("flags", [FLAGS, dict()], ids=["all", "off"])
def test_load_state_is_ordered_in_front_of_the_next_tick(monkeypatch, four, cls, lanes, flags):
    src, _ = early._engine(monkeypatch, four, cls=cls, lanes=lanes, early=bool(flags), **flags)
    snap = src.state(done=2, reset_ran=True)
    eng, rig = early._engine(monkeypatch, four, cls=cls, lanes=lanes, early=bool(flags), **flags)   # a fresh engine, a recording of its own
    built = len(rig.log)
    eng.load_state(snap)
    mark = len(rig.log)
    loaded = [j for j in range(built, mark) if rig.log[j][1] != "wait_stream"]
    names = [rig.log[j][1] for j in loaded]
    rams = [pt for pt in four.ports if pt.kind == "ram"]
    stages = len({pt.stage for pt in rams})
    assert names.count("upload_slots") == lanes and names.count("store_upload") == lanes * len(four.ports)
    assert names.count("circuit_bootstrap_batch") == (stages if flags else len(rams))   # the selectors the write-back will read
    assert names.index("circuit_bootstrap_batch") > max(j for j, n in enumerate(names) if n in ("upload_slots", "store_upload"))
    eng.tick()
    eng.run()
    before = rigs._before(rig.log)
    for j in range(mark, len(rig.log)):
        if rig.log[j][1] != "wait_stream":
            assert all((before[j] >> i) & 1 for i in loaded), rig.log[j][:2]
    bad = early._races(rig, eng.arena)
    assert not bad, early._show(rig, bad)
    # the write-back of that tick names selector slots the rebuild wrote
    chain = next(c for c in rig.log[mark:] if c[1] == "cmux_chain_batch")
    assert chain[2][0] is (eng.trgsw if flags else eng.mem[rams[0].name].trgsw)
    # a refused snapshot enqueues nothing
    mark = len(rig.log)
    other = Snapshot(dict(snap.meta, lanes=lanes + 1), snap.slots, snap.arena, snap.ram, snap.rom)
    with pytest.raises(ValueError, match="lanes"):
        eng.load_state(other)
    assert len(rig.log) == mark
    eng.free()
    src.free()


def test_flags_off_and_no_snapshot_enqueue_the_recorded_calls(monkeypatch, four):
    """the split of _port_read / _stage_read into selectors and tree moved no call: the default engine's recording is the parent's"""
    eng, rig = early._engine(monkeypatch, four, early=False)
    rigs._clocks(eng, four)
    eng.free()
    assert rigs._digest(rig.log) == rigs.PARENT_DIGEST
