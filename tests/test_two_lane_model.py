"""The two-lane model (frontier.two_lane_*): lane tables rescaled to a CU subset, the list-scheduling
simulation with its clock penalty, and the plans it prices — every gate once, antichains, every read ordered by its lane or a
wait edge, and the same bits as the plaintext simulator in any interleaving of the lanes that respects those edges.  The committed
profiles/r07_two_lane_model.txt must follow from the committed inputs."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from iyokan_amd import frontier as F  # noqa: E402
from iyokan_amd import netlist as N  # noqa: E402
from iyokan_amd.params import OPS  # noqa: E402
from netlist_util import gold  # noqa: E402


def _table():
    with open(os.path.join(ROOT, "profiles", "r06_final_model_inputs.json")) as f:
        return json.load(f)["128bit"]["cost_table"]


def _net(name):
    if name == "cahp-system":
        from iyokan_amd.system import load_blueprint

        return load_blueprint(gold("cahp-ruby-mux.toml")).nl
    if name == "cahp-core":
        return N.load_yosys_json(gold("cahp-ruby-core-yosys.json"))
    return N.load_iyokanl1_json(gold({"counter": "counter-4bit-iyokanl1.json", "mux-ram": "mux-ram-8-16-16.min.json"}[name]))


def test_lane_table_sees_a_narrow_level_grow_on_a_cu_subset():
    t = _table()
    whole, lane = F.make_level_cost(t), F.make_level_cost(F.lane_table(t, 64))
    assert lane.quanta == (512, 64)
    assert whole(511) == pytest.approx(t["pass_ms"][1])                 # 2 passes on 256 CUs
    assert lane(511) == pytest.approx(t["round_ms"])                    # 8 passes' worth on 64: one round of 512
    assert lane(64) == pytest.approx(t["pass_ms"][0]) and lane(65) == pytest.approx(t["pass_ms"][1])


def test_simulation_orders_lanes_by_their_edges_and_charges_the_penalty_only_while_lane_b_runs():
    # no lane B: the levels back to back
    assert F.simulate_lanes([(0.0, 2.0), (10.0, 0.0), (0.0, 3.0)], [], [], [], penalty=2.0) == pytest.approx(15.0)
    # B (4 ms) starts after A's level 0 and is needed by level 2; A's passes run at half speed beside it
    t = F.simulate_lanes([(0.0, 2.0), (0.0, 1.0), (0.0, 1.0)], [4.0], [0], [2], penalty=2.0)
    assert t == pytest.approx(2.0 + 4.0 + 1.0)          # level 1 takes 2 ms beside B, level 2 waits for B to end at 6
    # rounds are not penalised
    assert F.simulate_lanes([(1.0, 0.0), (3.0, 0.0)], [5.0], [-1], [2], penalty=2.0) == pytest.approx(5.0)
    with pytest.raises(ValueError):
        F.simulate_lanes([(0.0, 1.0), (0.0, 1.0)], [1.0], [1], [1])     # B after level 1, level 1 waits for B


def test_a_whole_device_lane_without_lane_b_prices_as_the_one_lane_plan():
    t = _table()
    nl = _net("mux-ram")
    levels = F.plan_levels(nl, 1, F.make_level_cost(t))
    one = sum(F.with_sub_pass_shape(F.make_level_cost(t))(r) for r in F.level_rotations(nl, levels))
    assert F.two_lane_price(nl, levels, [], t, 32) == pytest.approx(one)


def _check_plan(nl, levels, a_levels, sets):
    placed = [i for lv in a_levels for i in lv] + [i for s in sets for i in s["nodes"]]
    assert sorted(placed) == sorted(i for lv in levels for i in lv)     # every gate exactly once
    root = nl.roots()
    src = lambda j: root[j] if nl.kinds[j] == "OUTPUT" else j
    where = {}
    for k, lv in enumerate(a_levels):
        for i in lv:
            where[i] = ("A", k)
    for j, s in enumerate(sets):
        assert s["after"] < s["level"] < s["before"]
        for i in s["nodes"]:
            where[i] = ("B", j)
    for i, (lane, x) in where.items():
        for d in nl.ins[i]:
            d = src(d)
            if d not in where:
                continue                                                 # source: ready from the start
            dl, dx = where[d]
            if lane == "A" and dl == "A":
                assert dx < x                                            # earlier level (so never the same batch)
            elif lane == "A":
                assert sets[dx]["before"] <= x                           # a wait edge before lane A's level
            elif dl == "A":
                assert dx <= sets[x]["after"]                            # the set waits for that level
            else:
                assert dx < x                                            # an earlier set of lane B


def _desc(nl, slot, nodes):
    ops = np.array([OPS[nl.kinds[i]] for i in nodes], dtype=np.int32)
    cols = [np.array([slot[nl.ins[i][c]] if len(nl.ins[i]) > c else -1 for i in nodes], dtype=np.int32) for c in range(3)]
    return ops, cols[0], cols[1], cols[2], np.array([slot[i] for i in nodes], dtype=np.int32)


def _run_interleaved(nl, a_levels, sets, seed, clocks=3):
    """Both lanes on PlainBitBackend, one batch at a time, the next lane picked at random among those whose edges allow it"""
    plan = F.FrontierPlan(nl, 1, balance=False)                          # slots, latch and commit
    be = F.PlainBitBackend(plan.num_slots)
    sim = N.PlainSimulator(nl)
    for i, v in nl.dff_init.items():
        be.write(plan.slot[i], v)
    rng = np.random.default_rng(seed)
    gates = [i for lv in a_levels for i in lv] + [i for s in sets for i in s["nodes"]]
    for _ in range(clocks):
        be.gate_batch(*plan.latch_desc)
        be.gate_batch(*plan.commit_desc)
        sim.tick()
        for (port, bit) in sorted(nl.inputs):
            v = int(rng.integers(0, 2))
            be.write(plan.slot[nl.inputs[(port, bit)]], v)
            sim.set_input(port, bit, v)
        ka = jb = 0
        while ka < len(a_levels) or jb < len(sets):
            can_a = ka < len(a_levels) and all(j < jb for j, s in enumerate(sets) if s["before"] <= ka)
            can_b = jb < len(sets) and sets[jb]["after"] < ka
            assert can_a or can_b
            if can_a and (not can_b or rng.integers(0, 2)):
                be.gate_batch(*_desc(nl, plan.slot, a_levels[ka]))
                ka += 1
            else:
                be.gate_batch(*_desc(nl, plan.slot, sets[jb]["nodes"]))
                jb += 1
        sim.evaluate()
        assert [be.read(plan.slot[i]) for i in gates] == [sim.node_value(i) for i in gates]
        for key in sorted(nl.outputs):
            assert be.read(plan.slot[nl.outputs[key]]) == sim.get_output(*key)


@pytest.mark.parametrize("name", ["counter", "mux-ram", "cahp-core", "cahp-system"])
def test_two_lane_plans_are_ordered_and_compute_the_plaintext_bits(name):
    t = _table()
    nl = _net(name)
    levels = F.plan_levels(nl, 1, F.make_level_cost(t))
    depth = len(levels)
    shapes = [(8, 0, 1, 0), (8, depth // 2, 4, 0), (4, 0, 1 << 30, 0), (16, depth // 2, 2, depth // 2)]
    for n, (a, horizon, slack, head) in enumerate(shapes):
        a_levels, sets = F.two_lane_levels(nl, levels, t, a, horizon, slack, head)
        assert len(a_levels) == depth
        _check_plan(nl, levels, a_levels, sets)
        for seed in range(3 if name in ("counter", "mux-ram") else 1):
            _run_interleaved(nl, a_levels, sets, seed=100 * n + seed)


def test_the_best_two_lane_plan_is_the_cheapest_candidate_and_is_ordered():
    t = _table()
    nl = _net("mux-ram")
    levels = F.plan_levels(nl, 1, F.make_level_cost(t))
    best, = F.two_lane_bound(nl, t, 8, levels=levels)
    _check_plan(nl, levels, best["a_levels"], best["sets"])
    for horizon in (0, len(levels) // 2):
        a_levels, sets = F.two_lane_levels(nl, levels, t, 8, horizon, 4)
        assert best["ms"] <= F.two_lane_price(nl, a_levels, sets, t, 8) + 1e-9


def test_committed_two_lane_report_follows_from_the_committed_inputs():
    import scale_model

    with open(os.path.join(ROOT, "profiles", "r07_two_lane_model.txt")) as f:
        recorded = [json.loads(line) for line in f if line.startswith("{")]
    with open(os.path.join(ROOT, "profiles", "r06_final_model_inputs.json")) as f:
        inputs = json.load(f)
    with open(os.path.join(ROOT, "profiles", "r06_scale_model.json")) as f:
        one_gpu = {c: r["by_gpus"]["1"]["s_per_clock"] for c, r in json.load(f)["configs"].items() if "s_per_clock" in r["by_gpus"]["1"]}
    again = []
    for line in scale_model.two_lane(inputs, lane_cus=(8,)):
        again.append(line)
        if line["config"] != "3_mux_ram_8_16_16" and line["lanes"] == 2 and line["mode"] == "whole_head":
            break                                                        # config #4's two-lane lines at a = 8 are enough here
    for line in again:
        assert line in recorded, line
        if line["lanes"] == 1:
            assert line["ms_per_clock"] / 1e3 == pytest.approx(one_gpu[line["config"]], rel=1e-5)
    # the finding: no two-lane plan at the loaded clock comes within reach of the issue's 8 % gate
    for line in recorded:
        if line["lanes"] == 2 and line["penalty"] == "loaded":
            assert line["vs_one_lane"] > -0.08
