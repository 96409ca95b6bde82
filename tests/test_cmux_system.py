"""CPU: blueprints whose rom / ram builtins stay CMUX memory ports (system.load_blueprint(cmux_memories=True)) — stage assignment, the
staged FrontierPlan, the bits-only twin of the staged engine against PlainEngine on the lowered MUX form, and Ram.read_port +
Ram.write_port against Ram.clock.  The defaults must give the systems and plans recorded from the commit before the feature
(tests/golden/cmux_system_parent_plans.json)."""
import json
import os

import numpy as np
import pytest

import cmux_system_cases as cases
from iyokan_amd import cmux, runner
from iyokan_amd.frontier import FrontierPlan
from iyokan_amd.netlist import BINARY
from iyokan_amd.system import load_blueprint
from netlist_util import gold

HERE = os.path.dirname(os.path.abspath(__file__))
REFTEST = os.path.join(HERE, "golden", "reftest", "config-toml")


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = cases.write_blueprint(str(tmp_path_factory.mktemp("cmux_system")))
    return load_blueprint(path), load_blueprint(path, cmux_memories=True)


# ---- stages ------------------------------------------------------------------------------------------------------------------------------


def test_stage_assignment(small):
    lowered, sysm = small
    assert not lowered.ports and lowered.stages is None and lowered.num_stages == 1
    rom, ram = sysm.ports
    assert (rom.kind, rom.name, rom.addr_width, rom.data_width, rom.stage) == ("rom", "rom", 3, 4, 0)
    assert (ram.kind, ram.name, ram.addr_width, ram.data_width, ram.stage) == ("ram", "ram", 2, 2, 1)
    assert (len(rom.addr), len(rom.wren), len(rom.wdata), len(rom.rdata)) == (3, 0, 0, 4)
    assert (len(ram.addr), len(ram.wren), len(ram.wdata), len(ram.rdata)) == (2, 1, 2, 2)
    st, nl = sysm.stages, sysm.nl
    assert sysm.num_stages == 3 and not sysm.rom and not sysm.ram
    assert [st[i] for i in rom.addr] == [0, 0, 0] and [st[i] for i in rom.rdata] == [1] * 4
    assert [st[i] for i in ram.addr] == [1, 1] and [st[i] for i in ram.rdata] == [2, 2]
    assert st[ram.wren[0]] == 0 and [st[i] for i in ram.wdata] == [2, 2]          # wren straight from a DFF, wdata from its own rdata
    assert all(nl.kinds[i] == "INPUT" for i in rom.rdata + ram.rdata)               # sources that own arena slots
    gates = [i for i, k in enumerate(nl.kinds) if k in BINARY or k in ("MUX", "NOT")]
    by_stage = {s: sum(1 for i in gates if st[i] == s) for s in range(3)}
    assert by_stage == {0: 8, 1: 2, 2: 2}                                           # counter + out[1]; the RAM address; wdata
    assert [st[nl.outputs[("out", b)]] for b in range(4)] == [0, 0, 2, 1]
    assert all(st[i] == 0 for i, k in enumerate(nl.kinds) if k == "DFF")


def test_address_loop_is_refused(tmp_path):
    path = cases.write_blueprint(str(tmp_path), loop=True)
    load_blueprint(path)                                                            # the lowered form is an ordinary netlist
    with pytest.raises(ValueError, match=r"combinational loop.*'ram'"):
        load_blueprint(path, cmux_memories=True)


def _check_staged(sysm, plan):
    st, nl = sysm.stages, sysm.nl
    assert len(plan.stage_levels) == sysm.num_stages
    seen, expect_start = [], 0
    for s, rng in enumerate(plan.stage_levels):
        assert rng.start == expect_start
        expect_start = rng.stop
        for L in plan.levels[rng.start:rng.stop]:
            assert L["boot"] or L["ew"]
            for i in L["boot"] + L["ew"]:
                assert st[i] == s, (i, nl.kinds[i], st[i], s)
                seen.append(i)
    assert expect_start == len(plan.levels)
    placed = [i for i, k in enumerate(nl.kinds) if k not in ("INPUT", "DFF", "OUTPUT")]
    assert sorted(seen) == placed
    level_of = {i: k for k, L in enumerate(plan.levels) for i in L["boot"] + L["ew"]}
    root = nl.roots()
    for i in placed:                                                                # and inside a stage every gate after its drivers
        for j in nl.ins[i]:
            if root[j] in level_of:
                assert level_of[root[j]] < level_of[i]


@pytest.mark.parametrize("balance,spread", [(False, True), (True, True), (True, False)])
def test_staged_plan_keeps_every_gate_in_its_stage(small, balance, spread):
    _check_staged(small[1], FrontierPlan(small[1].nl, 1, balance, spread=spread, stages=small[1].stages))


def test_staged_plan_of_a_processor(tmp_path):
    """cahp-ruby with its rom / ram as ports: 4 k gates with slack on both sides of two ports, through the slack-moving planners"""
    sysm = load_blueprint(os.path.join(REFTEST, "cahp-ruby.toml"), cmux_memories=True)
    assert sorted((pt.kind, pt.stage) for pt in sysm.ports)[0][0] == "ram" and sysm.num_stages >= 2
    for pt in sysm.ports:
        assert all(sysm.stages[r] == pt.stage + 1 for r in pt.rdata)
    plan = FrontierPlan(sysm.nl, 1, True, stages=sysm.stages)
    _check_staged(sysm, plan)
    unstaged = FrontierPlan(sysm.nl, 1, True)                                       # what the planners do when nobody tells them
    level_of = {i: k for k, L in enumerate(unstaged.levels) for i in L["boot"] + L["ew"]}
    first_behind = min(k for i, k in level_of.items() if sysm.stages[i] > 0)
    assert first_behind < max(k for i, k in level_of.items() if sysm.stages[i] == 0)  # ... gates behind a port among those in front of it


# ---- the defaults give the parent's systems and plans --------------------------------------------------------------------------------------


def test_defaults_give_the_recorded_systems_and_plans():
    with open(os.path.join(HERE, "golden", "cmux_system_parent_plans.json")) as f:
        want = json.load(f)
    for core in ("ruby", "pearl"):
        sysm = load_blueprint(gold(f"cahp-{core}-mux.toml"))
        assert not sysm.ports and sysm.stages is None
        assert cases.system_digest(sysm) == want[core]["system"], core
        assert cases.system_digest(load_blueprint(gold(f"cahp-{core}-mux.toml"), cmux_memories=True)) == want[core]["system"]   # mux-* stay MUX
        assert cases.plan_digest(FrontierPlan(sysm.nl, 1, balance=False)) == want[core]["asap"], core
        if core == "ruby":                                                          # the planners take a while: once
            plan = FrontierPlan(sysm.nl, 1)
            assert cases.plan_digest(plan) == want[core]["balanced"]
            assert [len(plan.stage_levels), plan.stage_levels[0]] == [1, range(len(plan.levels))]


# ---- the bits twin against the lowered system ----------------------------------------------------------------------------------------------
CLOCKS = 8


def _trace(sysm, engine, req):
    out = []
    res = runner.run_packet(sysm, req, engine=engine, on_cycle=lambda done, eng: out.append(runner.result_packet(sysm, eng, done)))
    assert res.same_content(out[-1]) and len(out) == CLOCKS
    return out


class _Mutant(runner.StagedBitsEngine):
    """the twin with ONE mistake in the order: write-back after the DFF commit, rdata one stage early, or read after write"""

    def __init__(self, sysm, mutant):
        super().__init__(sysm)
        self.mutant = mutant

    def run(self):
        if self.mutant != "early_rdata":
            return super().run()
        self._reads(0)
        self.ex.run(after_stage=lambda s: self._reads(s + 1))

    def tick(self):
        if self.mutant == "early_rdata":
            return super().tick()
        if self.mutant == "commit_first":
            self.ex.tick()
        for pt in self.ports:
            if pt.kind == "ram":
                self._port_write(pt)
                if self.mutant == "read_after_write":
                    self._port_read(pt)
        if self.mutant != "commit_first":
            self.ex.tick()


def _first_difference(small, seed, mutant=None):
    lowered, sysm = small
    req = cases.request(seed, CLOCKS)
    want = _trace(lowered, runner.PlainEngine(lowered.nl), req)
    eng = (_Mutant(sysm, mutant) if mutant else runner.StagedBitsEngine(sysm))
    got = _trace(sysm, eng, req)
    return next((c for c in range(CLOCKS) if not want[c].same_content(got[c])), None), want


SEEDS = range(6)


def test_bits_twin_equals_plain_engine_on_the_lowered_form(small):
    changes = 0
    for seed in SEEDS:
        bad, want = _first_difference(small, seed)
        assert bad is None, (seed, bad)
        changes += sum(want[c].ram["ram"] != want[c + 1].ram["ram"] for c in range(CLOCKS - 1))
        assert set(want[-1].bits) == {"out"} and set(want[-1].ram) == {"ram"} and len(want[-1].ram["ram"]) == 8
    assert changes >= 6                                                             # the programs do write


@pytest.mark.parametrize("mutant", ["commit_first", "early_rdata", "read_after_write"])
def test_each_order_mistake_is_caught(small, mutant):
    """write-back after the DFF commit, rdata one stage early, read after write: each differs from the lowered form at some clock"""
    assert any(_first_difference(small, seed, mutant)[0] is not None for seed in SEEDS), mutant


def test_a_system_with_ports_needs_a_staged_engine(small):
    with pytest.raises(ValueError, match="staged engine"):
        runner.run_packet(small[1], cases.request(0, 1))


# ---- Ram.read_port + Ram.write_port against Ram.clock --------------------------------------------------------------------------------------


class _Recorder:
    """a stream that writes down what is enqueued"""

    gpu_index = 0

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            flat = [a if isinstance(a, (_Store, int)) or a is None else np.asarray(a).tolist() for a in args]
            self.calls.append((name, flat, sorted((k, np.asarray(v).tolist()) for k, v in kw.items())))
        return call


class _Store:
    def __init__(self, slots, *_):
        self.slots, self.ptr, self.words = int(slots), id(self), 0

    def upload(self, *a):
        pass

    def __eq__(self, other):
        return isinstance(other, _Store) and self.slots == other.slots


def _ram(monkeypatch, keys, addr_width, data_width):
    from iyokan_amd import hip

    for name in ("Trlwe", "Trgsw", "Arena"):
        monkeypatch.setattr(hip, name, _Store)
    monkeypatch.setattr(hip, "current_params", lambda: keys.params)
    st = _Recorder()
    N = keys.params.N
    return cmux.Ram(st, np.zeros((data_width << addr_width, 2 * N), dtype=np.uint32), addr_width, data_width), st


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 1)])
@pytest.mark.parametrize("fused", [True, False])
def test_the_two_halves_enqueue_what_clock_enqueues(monkeypatch, keys128, shape, fused):
    a, w = shape
    whole, st_whole = _ram(monkeypatch, keys128, a, w)
    halves, st_halves = _ram(monkeypatch, keys128, a, w)
    arena = _Store(64)
    wdata, rdata = list(range(10, 10 + w)), list(range(20, 20 + w))
    whole.clock(None, arena, 5, wdata, rdata, fused=fused, resident=True)
    halves.read_port(arena, rdata)
    split = len(st_halves.calls)
    halves.write_port(arena, 5, wdata, rdata, fused=fused)
    ptr = lambda calls: [(n, [x.slots if isinstance(x, _Store) else "ptr" if n == "bootstrap_trlwe_batch" and i == 6 else x for i, x in enumerate(args)], kw)
                         for n, args, kw in calls]
    assert ptr(st_whole.calls) == ptr(st_halves.calls)
    assert [c[0] for c in st_halves.calls[:split]] == ["cmux_batch"] * a + ["sample_extract_index_keyswitch_batch"]
    tail = ["bootstrap_trlwe_batch", "trlwe_add_batch"] + (["cmux_chain_batch"] if fused else ["cmux_batch"] * a)
    assert [c[0] for c in st_halves.calls[split:]] == tail + ["sample_extract_index_keyswitch_batch", "bootstrap_trlwe_batch"]
    with pytest.raises(ValueError):
        halves.read_port(arena, rdata + [0])
    with pytest.raises(ValueError):
        halves.write_port(arena, 5, wdata[:-1], rdata)
    assert len(st_halves.calls) == len(st_whole.calls)                              # a refusal enqueues nothing


def test_the_two_halves_give_the_cells_of_clock(monkeypatch, keys128, built):
    """the write chain each way enqueues, through the kernel's emulation on two copies of a RAM: the same cell words"""
    import cmux_ref
    import ram_ref
    from iyokan_amd import client

    em, p = ram_ref.emul(), keys128.params
    a, w = 2, 1
    trgsw = client.encrypt_trgsw(keys128, [1, 0], seed=5)
    spec = cmux_ref.spectra(em, p, trgsw)
    rows = None
    results = []
    for use_halves in (False, True):
        ram, st = _ram(monkeypatch, keys128, a, w)
        if rows is None:
            bits = [1, 1, 0, 1] + [1] + [0] * (ram.trlwe.slots - 5)                  # four cells, the written TRLWE's row somewhere behind
            rows = client.encrypt_ram_trlwe(keys128, bits, seed=6)
            rows[ram.mux_rows(0)[0]] = client.encrypt_ram_trlwe(keys128, [0], seed=7)[0]
        if use_halves:
            ram.read_port(_Store(8), [0])
            ram.write_port(_Store(8), 1, [2], [0])
        else:
            ram.clock(None, _Store(8), 1, [2], [0], resident=True)
        (chain,) = [c for c in st.calls if c[0] == "cmux_chain_batch"]
        jobs = list(zip(*chain[1][2:]))
        results.append(ram_ref.emu_chain_run(em, p, rows, spec, a, jobs)[:ram.ncells])
    assert np.array_equal(results[0], results[1])
    got = client.decrypt_ram_trlwe(keys128, results[0])
    assert list(got) == [1, 0, 0, 1]                                                # cell 1 (address bits 1, 0) took the written 0
