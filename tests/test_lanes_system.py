"""CPU: K request packets of one system in one run (runner.run_packets) on the bits twin of the GPU path — a FrontierExecutor on
PlainBitBackend(lanes=K), every level one gate batch over all lanes — and on PlainEngine(lanes=K).  Result r must be the packet
run_packet(system, requests[r]) returns alone, and what the reference recorded for the vector."""
import copy

import numpy as np
import pytest

from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, PlainBitBackend
from iyokan_amd.packet import PlainPacket
from iyokan_amd.runner import CipherEngine, CmuxCipherEngine, PlainEngine, run_packet, run_packets
from iyokan_amd.system import load_blueprint
from netlist_util import gold

K = 3
# blueprint, request, recorded result, cycles (tests/test_reference_vectors.py's)
VECTORS = {
    "counter-4bit": ("counter-4bit.toml", "test13.in", "test13.out", 3),
    "dff-reset": ("dff-reset.toml", "test23.in", "test23.out", 1),
    "mux-ram-8-16-16": ("mux-ram-8-16-16.toml", "test08.in", "test08.out", 8),
}


def bits_engine(nl, lanes, stride_extra=0):
    plan = FrontierPlan(nl, 1)
    be = PlainBitBackend(plan.num_slots + stride_extra, lanes=lanes)
    return CipherEngine(FrontierExecutor(plan, be), lambda bits: np.array(bits, dtype=np.uint8).reshape(-1, 1), lambda rows: np.asarray(rows).reshape(-1),
                        np.zeros(1, dtype=np.uint8), lanes=lanes)


def requests_of(name):
    """K requests: the vector's own first.  A system without inputs but @reset (counter-4bit, dff-reset) has nothing a request could
    differ in; the RAM system's second request rotates every input stream by one clock and its third has another RAM image."""
    base = PlainPacket.load(gold(VECTORS[name][1]))
    second, third = copy.deepcopy(base), copy.deepcopy(base)
    for port, stream in second.bits.items():
        width = len(stream) // 8
        second.bits[port] = stream[width:] + stream[:width]
    for ram, image in third.ram.items():
        third.ram[ram] = [1 - b for b in image]
    return [base, second, third]


@pytest.fixture(scope="module", params=list(VECTORS))
def run(request):
    """everything a vector's tests share: the system, the requests, each request's result alone, the laned results"""
    blueprint, _, want, cycles = VECTORS[request.param]
    sysm = load_blueprint(gold(blueprint))
    reqs = requests_of(request.param)
    alone = [run_packet(sysm, r, cycles=cycles, engine=bits_engine(sysm.nl, 1)) for r in reqs]
    eng = bits_engine(sysm.nl, K, stride_extra=5)          # a stride larger than the plan's slots
    arena0 = eng.ex.be.arena.clone()
    together = run_packets(sysm, reqs, cycles=cycles, engine=eng)
    return dict(name=request.param, sysm=sysm, reqs=reqs, alone=alone, together=together, cycles=cycles, want=PlainPacket.load(gold(want)), eng=eng, arena0=arena0)


def test_result_r_is_the_packet_of_request_r_alone(run):
    assert len(run["together"]) == K
    for got, want in zip(run["together"], run["alone"]):
        assert got.same_content(want), got.diff(want)
    assert run["together"][0].same_content(run["want"]), run["together"][0].diff(run["want"])
    if run["name"] == "mux-ram-8-16-16":      # the requests do differ, and so do their results
        assert not run["together"][1].same_content(run["together"][0]) and not run["together"][2].same_content(run["together"][0])


def test_plain_engine_lanes_agree(run):
    got = run_packets(run["sysm"], run["reqs"], cycles=run["cycles"])          # PlainEngine(lanes=K)
    for g, want in zip(got, run["alone"]):
        assert g.same_content(want), g.diff(want)


def test_slots_behind_a_lane_s_plan_are_never_written(run):
    be = run["eng"].ex.be
    a = be.arena.numpy().reshape(K, be.lane_stride)
    assert not a[:, -5:].any()


def test_one_input_bit_changes_its_own_lane_only():
    blueprint, req, _, cycles = VECTORS["mux-ram-8-16-16"]
    sysm = load_blueprint(gold(blueprint))
    base = PlainPacket.load(gold(req))
    other = copy.deepcopy(base)
    at = next(i for i, b in enumerate(base.bits["wren"]) if b == 1)           # one write becomes no write
    other.bits["wren"][at] = 0
    same = run_packets(sysm, [base, base, base], cycles=cycles, engine=bits_engine(sysm.nl, K))
    for middle in range(K):
        reqs = [other if r == middle else base for r in range(K)]
        got = run_packets(sysm, reqs, cycles=cycles, engine=bits_engine(sysm.nl, K))
        for r in range(K):
            assert got[r].same_content(same[r]) == (r != middle), (middle, r)


def test_requests_that_disagree_are_refused_before_anything_runs():
    sysm = load_blueprint(gold("counter-4bit.toml"))

    class Untouched:
        lanes = 2

        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was reached")

    with pytest.raises(ValueError, match="disagree on the number of cycles"):
        run_packets(sysm, [PlainPacket(cycles=3), PlainPacket(cycles=4)], engine=Untouched())
    with pytest.raises(ValueError, match="@reset cannot be set"):
        run_packets(sysm, [PlainPacket(cycles=3), PlainPacket(cycles=3, bits={"reset": [1]})], engine=Untouched())
    with pytest.raises(ValueError, match="needs a number of cycles"):
        run_packets(sysm, [PlainPacket(), PlainPacket()], engine=Untouched())
    with pytest.raises(ValueError, match="no request"):
        run_packets(sysm, [], engine=Untouched())
    with pytest.raises(ValueError, match="3 request packets for an engine with 2 lanes"):
        run_packets(sysm, [PlainPacket(cycles=1)] * 3, engine=Untouched())
    ram = load_blueprint(gold("mux-ram-8-16-16.toml"))
    with pytest.raises(ValueError, match="wrong length of RAM"):
        run_packets(ram, [PlainPacket(cycles=1), PlainPacket(cycles=1, ram={"target": [0, 1]})], engine=Untouched())


def test_engine_refusals():
    sysm = load_blueprint(gold("counter-4bit.toml"))
    plan2 = FrontierPlan(sysm.nl, 2)
    with pytest.raises(ValueError, match="lanes > 1 with world > 1"):
        FrontierExecutor(plan2, PlainBitBackend(plan2.num_slots, lanes=2), rank=0, world=2)
    FrontierExecutor(plan2, PlainBitBackend(plan2.num_slots), rank=0, world=2)              # one lane: as before
    plan = FrontierPlan(sysm.nl, 1)
    ex = FrontierExecutor(plan, PlainBitBackend(plan.num_slots, lanes=2))
    with pytest.raises(ValueError, match="CMUX memories have no lanes"):
        CmuxCipherEngine(sysm, ex, None, None, None, None, None, lanes=2)
    with pytest.raises(ValueError, match="CMUX memories have no lanes"):
        CmuxCipherEngine(sysm, ex, None, None, None, None, None)                            # the backend's lanes count, too
    with pytest.raises(ValueError, match="backend holds 2"):
        CipherEngine(ex, None, None, np.zeros(1, dtype=np.uint8), lanes=3)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            PlainBitBackend(4, lanes=bad)
        with pytest.raises(ValueError):
            PlainEngine(sysm.nl, lanes=bad)
    be = PlainBitBackend(4, lanes=2)
    with pytest.raises(ValueError, match="lane 2"):
        be.write(0, 1, lane=2)
    with pytest.raises(ValueError, match="outside the lane"):
        be.read(4, lane=0)


def test_executor_ports_take_a_lane():
    sysm = load_blueprint(gold("mux-ram-8-16-16.toml"))
    plan = FrontierPlan(sysm.nl, 1)
    ex = FrontierExecutor(plan, PlainBitBackend(plan.num_slots, lanes=2))
    ex.set_input("wren", 0, 1, lane=1)
    node = sysm.nl.inputs[("wren", 0)]
    assert ex.get_node(node, lane=1) == 1 and ex.get_node(node) == 0
    ex.set_node(node, 1)
    ex.set_node(node, 0, lane=1)
    assert ex.get_node(node, lane=0) == 1 and ex.get_node(node, lane=1) == 0
    ex.run()
    assert ex.get_output("rdata", 0, lane=1) in (0, 1)
