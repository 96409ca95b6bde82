"""CPU: the plan that knows when a port's address is ready (frontier.FrontierPlan(stages=, early=ports): address cones hoisted,
plan.port_ready) and the executor's call after every level (FrontierExecutor.run(after_level=)).  Systems: the hand-built one of
tests/read_early_cases.py and the committed cahp-ruby / cahp-diamond blueprints behind CMUX memories; where a cone belongs is computed
here (read_early_cases.cone_depths), apart from the planner."""
import numpy as np
import pytest

import cmux_system_cases as small
import read_early_cases as cases
from iyokan_amd.frontier import FrontierExecutor, FrontierPlan
from iyokan_amd.netlist import BINARY
from iyokan_amd.system import load_blueprint
from netlist_util import gold

MODES = [dict(balance=True, spread=True), dict(balance=True, spread=False), dict(balance=False)]
MODE_IDS = ["balance+spread", "balance", "asap"]


@pytest.fixture(scope="module")
def systems(tmp_path_factory):
    out = {"hand": load_blueprint(cases.write_blueprint(str(tmp_path_factory.mktemp("read_early"))), cmux_memories=True)}
    for name in ("cahp-ruby", "cahp-diamond"):
        out[name] = load_blueprint(gold(name + ".toml"), cmux_memories=True)
    return out


_plans = {}


def _plan(systems, name, mode, early):
    key = (name, MODES.index(mode), early)
    if key not in _plans:
        sysm = systems[name]
        _plans[key] = FrontierPlan(sysm.nl, 1, stages=sysm.stages, **mode, **({"early": sysm.ports} if early else {}))
    return _plans[key]


def _same_descs(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_hand_system_is_what_its_docstring_says(systems):
    sysm = systems["hand"]
    assert [(pt.kind, pt.name, pt.addr_width, pt.data_width, pt.stage) for pt in sysm.ports] == [("rom", "rom", 3, 4, 0), ("ram", "ram", 2, 2, 0)]
    assert sysm.num_stages == 2
    rom, ram = sysm.ports
    assert sorted(cases.cone_depths(sysm, rom).values()) == [1, 1, 1] and cases.cone_depths(sysm, ram) == {}
    root = sysm.nl.roots()
    assert all(sysm.nl.kinds[root[a]] == "DFF" for a in ram.addr + ram.wren)
    assert {root[w] for w in ram.wdata} <= {root[r] for r in rom.rdata}
    plan = _plan(systems, "hand", MODES[2], False)
    assert len(plan.stage_levels[0]) == cases.SIDE_CHAIN and len(plan.stage_levels[1]) >= 1


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["hand", "cahp-ruby", "cahp-diamond"])
def test_without_early_the_plan_is_the_staged_plan(systems, name, mode):
    """early=None spelled out against the call of before the argument: levels, slots, descriptors"""
    sysm = systems[name]
    a = _plan(systems, name, mode, False)
    b = FrontierPlan(sysm.nl, 1, stages=sysm.stages, early=None, **mode)
    assert small.plan_digest(a) == small.plan_digest(b) and a.stage_levels == b.stage_levels and not hasattr(a, "port_ready")
    for La, Lb in zip(a.levels, b.levels):
        assert _same_descs(La["ew_desc"], Lb["ew_desc"]) and _same_descs(La["rank_desc"][0], Lb["rank_desc"][0])
    assert _same_descs(a.latch_desc, b.latch_desc) and _same_descs(a.commit_desc, b.commit_desc)


def test_early_needs_stages(systems):
    with pytest.raises(ValueError, match="stages="):
        FrontierPlan(systems["hand"].nl, 1, early=systems["hand"].ports)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["hand", "cahp-ruby", "cahp-diamond"])
def test_early_hoists_the_cones_and_knows_when_a_port_is_ready(systems, name, mode):
    sysm = systems[name]
    nl, root = sysm.nl, sysm.nl.roots()
    base, plan = _plan(systems, name, mode, False), _plan(systems, name, mode, True)
    at, at0 = cases.level_of(plan), cases.level_of(base)
    # the same gates in the same number of levels per stage, every gate in its own stage's range and exactly once
    assert sorted(at) == sorted(at0) and [len(r) for r in plan.stage_levels] == [len(r) for r in base.stage_levels]
    assert sum(len(L["boot"]) + len(L["ew"]) for L in plan.levels) == len(at)
    assert all(at[i] in plan.stage_levels[sysm.stages[i]] for i in at)
    assert plan.num_slots == base.num_slots and plan.shadow_base == base.shadow_base
    # every gate's inputs lie in earlier levels; a bootstrapped gate may also read an elementwise gate of its own level, which the
    # executor runs first (an elementwise gate may not: one batch never reads a slot it writes)
    ew = {i for L in plan.levels for i in L["ew"]}
    for i, k in at.items():
        for j in nl.ins[i]:
            j = root[j]
            if j in at:
                assert at[j] < k or (at[j] == k and j in ew and i not in ew), (i, j)
    # the descriptors name the slots of the gates of their level
    for L in plan.levels:
        assert list(L["rank_desc"][0][4]) == [plan.slot[i] for i in L["boot"]] and list(L["ew_desc"][4]) == [plan.slot[i] for i in L["ew"]]
        assert all(nl.kinds[i] in BINARY or nl.kinds[i] == "MUX" for i in L["boot"])
    # every cone gate at the level of the longest path that ends in it, and port_ready behind the deepest of them
    cone_gates = set()
    for pt in sysm.ports:
        start = plan.stage_levels[pt.stage].start
        depth = cases.cone_depths(sysm, pt)
        cone_gates |= set(depth)
        for i, d in depth.items():
            assert at[i] == start + d - 1, (pt.name, i, at[i], start, d)
        assert plan.port_ready[pt.name] == start + max(depth.values(), default=0), pt.name
    assert set(plan.port_ready) == {pt.name for pt in sysm.ports}
    # and nothing else moved
    assert all(at[i] == at0[i] for i in at if i not in cone_gates)


def test_port_ready_of_the_three_systems(systems):
    hand, ruby, diamond = (_plan(systems, n, MODES[0], True) for n in ("hand", "cahp-ruby", "cahp-diamond"))
    assert hand.port_ready == {"rom": hand.stage_levels[0].start + 1, "ram": hand.stage_levels[0].start}
    start, levels = ruby.stage_levels[0].start, len(ruby.stage_levels[0])
    assert ruby.port_ready["ram"] == start and 0 < ruby.port_ready["rom"] - start <= levels // 4      # about 6 of about 40
    print("cahp-ruby: rom ready after", ruby.port_ready["rom"] - start, "of", levels, "levels")
    assert diamond.port_ready["ramA"] == diamond.port_ready["ramB"] == diamond.stage_levels[0].start
    assert diamond.stage_levels[0].start < diamond.port_ready["rom"] <= diamond.stage_levels[0].stop
    # the balancer does push cone gates late on the committed blueprint: without the hoist port_ready would be a lie
    at0 = cases.level_of(_plan(systems, "cahp-ruby", MODES[0], False))
    rom = systems["cahp-ruby"].ports[0]
    assert max(at0[i] for i in cases.cone_depths(systems["cahp-ruby"], rom)) >= ruby.port_ready["rom"]


# ---- the executor's calls ------------------------------------------------------------------------------------------------------------------

class _Recorder:
    """a backend that writes down its gate batches by their output slots"""

    def __init__(self, log):
        self.log = log

    def gate_batch(self, ops, in0, in1, in2, out):
        if len(ops):
            self.log.append(("batch", tuple(int(s) for s in out)))


def _expected(plan, stage=False, level=False):
    want = [("level", 0)] if level else []
    for s, rng in enumerate(plan.stage_levels):
        for k in rng:
            L = plan.levels[k]
            want += [("batch", tuple(plan.slot[i] for i in part)) for part in (L["ew"], L["boot"]) if part]
            if level:
                want.append(("level", k + 1))
        if stage:
            want.append(("stage", s))
    return want


@pytest.mark.parametrize("name", ["hand", "cahp-ruby"])
def test_after_level_is_called_behind_every_level_and_in_front_of_after_stage(systems, name):
    plan = _plan(systems, name, MODES[0], True)
    log = []
    ex = FrontierExecutor(plan, _Recorder(log))
    hooks = dict(after_stage=lambda s: log.append(("stage", s)), after_level=lambda i: log.append(("level", i)))
    ex.run(**hooks)
    assert log == _expected(plan, stage=True, level=True)
    assert [e[1] for e in log if e[0] == "level"] == list(range(len(plan.levels) + 1))
    for s, rng in enumerate(plan.stage_levels):                                     # a boundary: the level's call, then the stage's
        assert log.index(("stage", s)) == log.index(("level", rng.stop)) + 1
    del log[:]
    ex.run(after_level=hooks["after_level"])
    assert log == _expected(plan, level=True)
    # without the argument: the sequence of before it
    del log[:]
    ex.run(after_stage=hooks["after_stage"])
    assert log == _expected(plan, stage=True)
    del log[:]
    ex.run()
    assert log == _expected(plan)


def test_a_stage_without_levels_calls_after_stage_alone(tmp_path):
    """tests/cmux_system_cases.py's system has a stage of no gates in front (the ROM is addressed by DFFs): one call per level index"""
    sysm = load_blueprint(small.write_blueprint(str(tmp_path)), cmux_memories=True)
    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages, early=sysm.ports)
    log = []
    FrontierExecutor(plan, _Recorder(log)).run(after_stage=lambda s: log.append(("stage", s)), after_level=lambda i: log.append(("level", i)))
    assert log == _expected(plan, stage=True, level=True)
    assert [e[1] for e in log if e[0] == "level"] == list(range(len(plan.levels) + 1))
    assert [e[1] for e in log if e[0] == "stage"] == list(range(sysm.num_stages))
    assert plan.port_ready["rom"] == 0 and plan.stage_levels[sysm.ports[1].stage].start <= plan.port_ready["ram"]
