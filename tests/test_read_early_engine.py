"""CPU: the engines that read a memory port as soon as its address is ready (read_early=True).

The bits twin (runner.StagedBitsEngine): the program order alone — every clock's result packet against PlainEngine on the lowered
form of tests/read_early_cases.py's system; two mutants show that the order is what the test checks.

The cipher engines (runner.CmuxCipherEngine / CmuxLaneEngine) on the recording rig of tests/test_cmux_stage_cb.py: a wait_stream is an
ordering edge, the executor's arena is attributed per SLOT from the descriptor and slot arrays of every call, every other store whole.
Every pair of calls on different streams that touch a common slot or store, one of them writing, has to be ordered by program order
plus the edges; the circuit bootstrapping of a stage and the stage's last gate level have to be unordered — the overlap the flag is
for; four mutants, each without one of the waits, are caught."""
import numpy as np
import pytest

import cmux_stage_cases as stage_cases
import read_early_cases as cases
import test_cmux_lanes_system as lane_rigs
import test_cmux_stage_cb as rigs
from iyokan_amd import frontier, runner
from iyokan_amd.frontier import FrontierExecutor, FrontierPlan
from iyokan_amd.system import load_blueprint

CLOCKS, PROGRAMS = 8, 6


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    path = cases.write_blueprint(str(tmp_path_factory.mktemp("read_early_engine")))
    return load_blueprint(path, cmux_memories=True), load_blueprint(path)


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    return load_blueprint(stage_cases.write_blueprint(str(tmp_path_factory.mktemp("read_early_four"))), cmux_memories=True)


# ---- the bits twin ------------------------------------------------------------------------------------------------------------------------

def _every_clock(sysm, req, engine=None):
    out = []
    runner.run_packet(sysm, req, engine=engine, on_cycle=lambda done, eng: out.append(runner.result_packet(sysm, eng, done)))
    return out


@pytest.fixture(scope="module")
def wanted(hand):
    """PlainEngine on the lowered form: the result packet after every clock of every program, computed once"""
    reqs = cases.programs(PROGRAMS, CLOCKS)
    want = [_every_clock(hand[1], r) for r in reqs]
    assert all(len(w) == CLOCKS for w in want)
    assert any(not want[0][c].same_content(want[0][c + 1]) for c in range(CLOCKS - 1))
    return reqs, want


def _agrees(sysm, reqs, want, make):
    """per program: whether every clock's result packet of make()'s engine equals the wanted one"""
    return [all(w.same_content(g) for w, g in zip(want[k], _every_clock(sysm, r, engine=make()))) for k, r in enumerate(reqs)]


@pytest.mark.parametrize("balance", [True, False], ids=["balance", "asap"])
def test_bits_twin_reads_early_and_gives_the_lowered_forms_packets(hand, wanted, balance):
    sysm, _ = hand
    reqs, want = wanted
    assert all(_agrees(sysm, reqs, want, lambda: runner.StagedBitsEngine(sysm, balance=balance, read_early=True)))
    eng = runner.StagedBitsEngine(sysm, balance=balance, read_early=True)
    assert eng.ex.plan.port_ready == {"rom": 1, "ram": 0}
    assert not hasattr(runner.StagedBitsEngine(sysm, balance=balance).ex.plan, "port_ready")       # the default plan is the one of before


def test_bits_twin_reads_where_port_ready_says(hand):
    """the order of one run(): the RAM's read in front of level 0, the ROM's behind it, both in front of level 1"""
    sysm, _ = hand
    eng = runner.StagedBitsEngine(sysm, read_early=True)
    log = []
    be, read = eng.ex.be, eng._port_read
    gate = be.gate_batch
    be.gate_batch = lambda *a: (log.append("batch") if len(a[0]) else None, gate(*a))[1]
    eng._port_read = lambda pt: (log.append(pt.name), read(pt))[1]
    eng.run()
    plan = eng.ex.plan
    per_level = [sum(1 for part in (L["ew"], L["boot"]) if part) for L in plan.levels]
    assert log == ["ram"] + ["batch"] * per_level[0] + ["rom"] + ["batch"] * sum(per_level[1:])
    off = runner.StagedBitsEngine(sysm)
    log2 = []
    gate2, read2 = off.ex.be.gate_batch, off._port_read
    off.ex.be.gate_batch = lambda *a: (log2.append("batch") if len(a[0]) else None, gate2(*a))[1]
    off._port_read = lambda pt: (log2.append(pt.name), read2(pt))[1]
    off.run()
    n0 = sum(per_level[:len(plan.stage_levels[0])])
    assert log2 == ["batch"] * n0 + ["rom", "ram"] + ["batch"] * (sum(per_level) - n0)


def test_bits_twin_with_three_lanes_through_run_packets(hand):
    sysm, low = hand
    reqs = cases.programs(3, CLOCKS, first=300)
    want = [runner.run_packet(low, r) for r in reqs]
    got = runner.run_packets(sysm, reqs, engine=runner.StagedBitsEngine(sysm, lanes=3, read_early=True))
    assert all(w.same_content(g) for w, g in zip(want, got)), [w.diff(g) for w, g in zip(want, got)]
    assert not want[0].same_content(want[1])


class _OneLevelTooSoon(runner.StagedBitsEngine):
    """a port whose address has a cone is read one level before port_ready"""

    def _ready_level(self, pt):
        ready = self.ex.plan.port_ready[pt.name]
        return max(self.ex.plan.stage_levels[pt.stage].start, ready - 1)


def _not_hoisted(sysm):
    """an engine that trusts port_ready over a plan whose cone gates stayed where the planner put them"""
    eng = runner.StagedBitsEngine(sysm, read_early=True)
    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    plan.port_ready = dict(eng.ex.plan.port_ready)
    eng.ex = FrontierExecutor(plan, frontier.PlainBitBackend(plan.num_slots))
    return eng


def test_each_mistake_of_the_order_gives_other_packets(hand, wanted, monkeypatch):
    sysm, _ = hand
    reqs, want = wanted
    assert not all(_agrees(sysm, reqs, want, lambda: _OneLevelTooSoon(sysm, read_early=True)))
    # a planner that pushes gates with slack late, as the balancer does on the committed blueprints (tests/test_read_early_plan.py)
    monkeypatch.setattr(frontier, "plan_levels", cases.late_levels)
    late = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    at = cases.level_of(late)
    assert min(at[i] for i in cases.cone_depths(sysm, sysm.ports[0])) > 0           # the ROM's cone did leave level 0
    assert not all(_agrees(sysm, reqs, want, lambda: _not_hoisted(sysm)))
    assert all(_agrees(sysm, reqs, want, lambda: runner.StagedBitsEngine(sysm, read_early=True)))   # hoisted, the same planner is fine
    assert all(_agrees(sysm, reqs, want, lambda: runner.StagedBitsEngine(sysm)))


# ---- the cipher engines on recording streams -----------------------------------------------------------------------------------------------

def _engine(monkeypatch, sysm, cls=runner.CmuxCipherEngine, lanes=1, early=True, **kw):
    rig = rigs._Rig(monkeypatch)
    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages, **({"early": sysm.ports} if early else {}))
    be = lane_rigs._LaneBackend(rig, plan.num_slots, lanes) if lanes > 1 else rigs._Backend(rig, plan.num_slots)
    n1 = int(rigs.P.n) + 1
    packets = [rigs._Packet(sysm) for _ in range(lanes)]
    images = dict(packets=packets) if cls is runner.CmuxLaneEngine else dict(packet=packets[0])
    eng = cls(sysm, FrontierExecutor(plan, be), lambda bits: np.zeros((len(bits), n1), dtype=np.uint32), lambda rows: [0] * len(rows),
              np.zeros(n1, dtype=np.uint32), rigs._Key("bk2", int(rigs.P.n)), rigs._Key("pk"), decrypt_ram=lambda rows: [0] * len(rows),
              **images, **kw)
    return eng, rig


def _clocks(eng, sysm, rig, n=3):
    """rigs._clocks, with the recording's length noted around every run(): [(first call, one past the last)]"""
    runs = []

    def run():
        first = len(rig.log)
        eng.run()
        runs.append((first, len(rig.log)))

    for lane in range(eng.lanes):
        for pt in sysm.ports:
            (eng.load_rom if pt.kind == "rom" else eng.load_ram)(pt.name, None, **({"lane": lane} if lane else {}))
    run()
    for _ in range(n):
        eng.tick()
        run()
    for pt in sysm.ports:
        if pt.kind == "ram":
            eng.ram_rows(pt.name)
    return runs


def _access(rig, main, call):
    """(what a recorded call reads, what it writes): ("slot", s) of the executor's arena, ("store", serial) of every other store"""
    _, name, args, kw = call
    kw = dict(kw)
    R, W = set(), set()
    whole = lambda st: ("store", st.serial)

    def slots(store, idx, into):
        if store is main:
            into.update(("slot", int(s)) for s in idx if s >= 0)
        else:
            into.add(whole(store))

    if name == "gate_batch":
        for r in range(kw.get("lanes", 1)):
            off = r * (kw.get("lane_stride") or 0)
            for col in args[2:5]:
                slots(args[0], [s + off for s in col if s >= 0], R)
            slots(args[0], [s + off for s in args[5]], W)
    elif name == "upload_slots":
        slots(args[0], args[1], W)
    elif name == "circuit_bootstrap_batch":
        slots(args[2], args[3], R)
        W |= {whole(args[5]), whole(args[7]), whole(args[8])}
    elif name in rigs.SEL_POS:
        R.add(whole(args[0]))
        W.add(whole(args[1]))
    elif name == "sample_extract_index_keyswitch_batch":
        R.add(whole(args[0]))
        slots(args[4], args[3], W)
    elif name == "bootstrap_trlwe_batch":
        slots(args[0], args[1], R)
        slots(args[0], args[2], R)
        W.add(whole(rig.stores[args[6]]))
    elif name in ("trlwe_add_batch", "store_upload"):
        W.add(whole(args[0]))
    elif name == "store_download":
        R.add(whole(args[0]))
    else:
        assert name in ("wait_stream", "sync"), name
    return R, W


def _races(rig, main):
    """the pairs of calls on different streams that touch a common slot or store, one of them writing, and are not ordered"""
    before = rigs._before(rig.log)
    touched = {}
    for j, call in enumerate(rig.log):
        R, W = _access(rig, main, call)
        for res in R | W:
            touched.setdefault(res, []).append((j, res in W))
    bad = []
    for res, calls in touched.items():
        for b, (j, wj) in enumerate(calls):
            for i, wi in calls[:b]:
                if (wi or wj) and rig.log[i][0] != rig.log[j][0] and not (before[j] >> i) & 1:
                    bad.append((i, j, res))
    return bad


def _show(rig, bad):
    return [(rig.log[i][:2], rig.log[j][:2], res) for i, j, res in bad[:4]]


def _overlaps(eng, rig, sysm, runs):
    """per run() and stage with ports and at least two levels behind its batch: (the circuit bootstrapping batches, the stage's last
    gate batch) as positions in the recording"""
    plan = eng.ex.plan
    out = []
    for first, last in runs:
        for s in sorted({pt.stage for pt in sysm.ports}):
            rng = plan.stage_levels[s]
            addr = {plan.slot[a] for pt in sysm.ports if pt.stage == s for a in pt.addr}
            cbs = [j for j in range(first, last) if rig.log[j][1] == "circuit_bootstrap_batch" and set(rig.log[j][2][3]) & addr]
            final = plan.levels[rng.stop - 1] if len(rng) else None
            if final is None or not final["boot"]:
                continue
            want = [plan.slot[i] for i in final["boot"]]
            gates = [j for j in range(first, last) if rig.log[j][1] == "gate_batch" and rig.log[j][2][5] == want]
            assert len(gates) == 1 and cbs
            out.append((cbs, gates[0]))
    return out


CONFIGS = [dict(), dict(stage_cb=True), dict(refresh_aside=True), dict(stage_cb=True, refresh_aside=True),
           dict(stage_cb=True, refresh_aside=True, rom_fused=True, tree_fused=True)]
CONFIG_IDS = ["alone", "stage_cb", "refresh_aside", "stage_cb+refresh_aside", "all+fused"]


@pytest.mark.parametrize("flags", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("which", ["hand", "four"])
def test_read_early_orders_every_shared_slot_and_store_and_nothing_more(monkeypatch, hand, four, which, flags):
    sysm = hand[0] if which == "hand" else four
    eng, rig = _engine(monkeypatch, sysm, read_early=True, **flags)
    runs = _clocks(eng, sysm, rig)
    assert len(rig.streams) == 2 + bool(flags.get("refresh_aside"))                 # M, P and at most R
    assert all(eng.mem[pt.name].stream is eng.port_stream for pt in sysm.ports) and eng.port_stream is not eng.stream
    bad = _races(rig, eng.arena)
    assert not bad, _show(rig, bad)
    P = eng.port_stream.sid
    batches = [c for c in rig.log if c[1] == "circuit_bootstrap_batch"]
    stages = {pt.stage for pt in sysm.ports}
    assert len(batches) == 4 * (len(stages) if flags.get("stage_cb") else len(sysm.ports)) and all(c[0] == P for c in batches)
    assert all(c[0] == 0 for c in rig.log if c[1] in ("gate_batch", "upload_slots"))
    assert all(c[0] != 0 for c in rig.log if c[1] in rigs.SEL_POS or c[1] in ("sample_extract_index_keyswitch_batch", "bootstrap_trlwe_batch"))
    # after every run() M is ordered behind everything P holds
    before = rigs._before(rig.log)
    for first, last in runs:
        on_p = [j for j in range(first, last) if rig.log[j][0] == P and rig.log[j][1] != "wait_stream"]
        tail = max(j for j in range(first, last) if rig.log[j][0] == 0)
        assert on_p and all((before[tail] >> j) & 1 for j in on_p)
    if which == "hand":
        # nothing more: the batches of stage 0 and the stage's last gate level are unordered, either way round
        pairs = _overlaps(eng, rig, sysm, runs)
        assert len(pairs) == 4
        for cbs, gate in pairs:
            assert len(cbs) == (1 if flags.get("stage_cb") else 2)
            for j in cbs:
                assert j < gate and not (before[gate] >> j) & 1, (j, gate)
        # ... and the batch goes out where port_ready says: the RAM's in front of the first gate batch, the ROM's (and the stage's) behind level 0
        plan = eng.ex.plan
        for first, last in runs:
            seq = [(c[1], c[2][3] if c[1] == "circuit_bootstrap_batch" else c[2][5]) for c in rig.log[first:last]
                   if c[1] in ("circuit_bootstrap_batch", "gate_batch")]
            level0 = [plan.slot[i] for i in plan.levels[0]["boot"]]
            rom, ram = ([plan.slot[a] for a in pt.addr] for pt in sysm.ports)
            k0 = seq.index(("gate_batch", level0))
            if flags.get("stage_cb"):
                assert seq[k0 + 1] == ("circuit_bootstrap_batch", rom + ram)
            else:
                assert seq[0] == ("circuit_bootstrap_batch", ram) and seq[k0 + 1] == ("circuit_bootstrap_batch", rom)
    eng.free()
    assert eng.port_stream is None and rig.streams[P].destroyed


def test_lane_engine_with_two_lanes(monkeypatch, hand):
    sysm = hand[0]
    eng, rig = _engine(monkeypatch, sysm, cls=runner.CmuxLaneEngine, lanes=2, read_early=True, stage_cb=True, refresh_aside=True)
    runs = _clocks(eng, sysm, rig)
    assert len(rig.streams) == 3
    bad = _races(rig, eng.arena)
    assert not bad, _show(rig, bad)
    plan, S = eng.ex.plan, eng.ex.plan.num_slots
    one = [plan.slot[a] for pt in sysm.ports for a in pt.addr]
    batches = [c for c in rig.log if c[1] == "circuit_bootstrap_batch"]
    assert len(batches) == 4 and all(c[2][3] == [s + r * S for r in range(2) for s in one] for c in batches)
    before = rigs._before(rig.log)
    for first, last in runs:                                                        # the overlap: the stage's last level carries both lanes
        final = plan.levels[plan.stage_levels[0].stop - 1]
        gate, = [j for j in range(first, last) if rig.log[j][1] == "gate_batch" and rig.log[j][2][5] == [plan.slot[i] for i in final["boot"]]]
        cb, = [j for j in range(first, last) if rig.log[j][1] == "circuit_bootstrap_batch"]
        assert cb < gate and not (before[gate] >> cb) & 1
    eng.free()


class _NoForkWait(runner.CmuxCipherEngine):
    def _fork(self):
        self._reads_pending = True


class _NoJoinBeforeTheNextStage(runner.CmuxCipherEngine):
    """joins at the end of run() only"""

    def _early_stage(self, s):
        self._stage = s + 1
        self._read_ready()


class _WriteWithoutWait(runner.CmuxCipherEngine):
    def tick(self):
        self._write_ports()
        self.stream.wait_stream(self.port_stream)
        self.ex.tick()


class _CommitWithoutWait(runner.CmuxCipherEngine):
    def tick(self):
        self.port_stream.wait_stream(self.stream)
        self._write_ports()
        self.ex.tick()


@pytest.mark.parametrize("mutant,which", [(_NoForkWait, "hand"), (_NoForkWait, "four"), (_NoJoinBeforeTheNextStage, "hand"),
                                          (_NoJoinBeforeTheNextStage, "four"), (_WriteWithoutWait, "four"), (_CommitWithoutWait, "hand"),
                                          (_CommitWithoutWait, "four")])
@pytest.mark.parametrize("flags", [dict(), dict(stage_cb=True, refresh_aside=True)], ids=["alone", "stage_cb+refresh_aside"])
def test_each_missing_wait_is_caught(monkeypatch, hand, four, mutant, which, flags):
    sysm = hand[0] if which == "hand" else four
    eng, rig = _engine(monkeypatch, sysm, cls=mutant, read_early=True, **flags)
    _clocks(eng, sysm, rig)
    assert _races(rig, eng.arena), mutant.__name__


# ---- flag off ---------------------------------------------------------------------------------------------------------------------------------

def test_flag_off_enqueues_the_default_engines_calls(monkeypatch, four, hand):
    for sysm in (four, hand[0]):
        digests = []
        for kw in ({}, {"read_early": False}):
            eng, rig = _engine(monkeypatch, sysm, early=False, **kw)
            rigs._clocks(eng, sysm)
            eng.free()
            assert len(rig.streams) == 1 and eng.port_stream is None and not [c for c in rig.log if c[1] in ("wait_stream", "sync")]
            digests.append(rigs._digest(rig.log))
        assert digests[0] == digests[1]
        if sysm is four:
            assert digests[0] == rigs.PARENT_DIGEST                                 # the recording of the commit before CMUX memories had lanes


@pytest.mark.parametrize("flags", [dict(), dict(stage_cb=True, refresh_aside=True)], ids=["alone", "stage_cb+refresh_aside"])
def test_read_early_moves_calls_and_changes_none(monkeypatch, hand, flags):
    """over the same plan, without the waits and whatever the stream: the calls of the flag-off engine, every one once"""
    canon = []
    for early in (False, True):
        eng, rig = _engine(monkeypatch, hand[0], read_early=early, **flags)
        _clocks(eng, hand[0], rig)
        canon.append(sorted(repr((name, [repr(a) if isinstance(a, (rigs._Store, rigs._Key)) else a for a in args], k))
                            for _, name, args, k in rig.log if name not in ("wait_stream", "sync")))
        eng.free()
    assert canon[0] == canon[1] and len(canon[0]) > 40


def test_read_early_needs_the_plan_that_knows(monkeypatch, hand):
    with pytest.raises(ValueError, match="early=system.ports"):
        _engine(monkeypatch, hand[0], early=False, read_early=True)
