"""The hand-built system of the read_early tests (test_read_early_plan / test_read_early_engine / test_gpu_read_early), one Iyokan-L1
core behind the builtins of tests/cmux_system_cases.py (a ROM 3 x 4, a RAM 2 x 2):

    a 3-bit counter in DFFs; the ROM's address is the counter behind ONE level of XORs   -> its cone is three gates of stage 0, level 0
    the RAM's address comes straight from two DFFs                                      -> its cone is empty: ready at the stage's start
    a side chain of four dependent gates of stage 0 outside every cone                  -> stage 0 has four levels, the cones slack
    wren from a DFF (fed by ROM bit 3), wdata from the ROM's rdata bits 1, 2
    stage-1 gates mix both rdata into the DFFs that address the RAM and into @out

Both ports are stage 0, their rdata and everything behind it stage 1.  Also an independent longest-path computation of where an
address cone belongs, and a planner that pushes every gate as late as it can go (what the balancer does to slack-rich gates on the
committed blueprints, made certain here)."""
import json
import os

import numpy as np

import cmux_system_cases as small

ROM_SHAPE, RAM_SHAPE = small.ROM_SHAPE, small.RAM_SHAPE
BLUEPRINT = small.BLUEPRINT
SIDE_CHAIN = 4


def core_json():
    c = small._Core()
    reset = c.inp("reset", 0)
    romd = [c.inp("romd", i) for i in range(4)]
    ramr = [c.inp("ramr", i) for i in range(2)]
    cnt = [c.dff() for _ in range(3)]
    wq, a0, a1, q0, sq = (c.dff() for _ in range(5))
    nxt = [c.gate("NOT", A=cnt[0]), c.gate("XOR", A=cnt[0], B=cnt[1]), c.gate("XOR", A=cnt[2], B=c.gate("AND", A=cnt[0], B=cnt[1]))]
    for d, x in zip(cnt, nxt):
        c.feed(d, c.gate("ANDNOT", A=x, B=reset))
    for i in range(3):                                                              # the ROM's address cone: one level
        c.out("rom_addr", i, c.gate("XOR", A=cnt[i], B=cnt[(i + 1) % 3]))
    c.out("ram_addr", 0, a0)
    c.out("ram_addr", 1, a1)
    side = c.gate("AND", A=cnt[0], B=cnt[2])                                        # four dependent gates outside every cone
    side = c.gate("XOR", A=side, B=cnt[1])
    side = c.gate("OR", A=side, B=q0)
    side = c.gate("XNOR", A=side, B=cnt[2])
    c.feed(sq, side)
    c.feed(wq, romd[3])
    c.out("wren", 0, wq)
    c.out("wdata", 0, romd[1])
    c.out("wdata", 1, romd[2])
    m0 = c.gate("XOR", A=romd[0], B=ramr[0])                                        # stage 1: both rdata, into DFFs
    m1 = c.gate("XNOR", A=romd[2], B=ramr[1])
    c.feed(a0, c.gate("XOR", A=romd[1], B=ramr[1]))
    c.feed(a1, m1)
    c.feed(q0, m0)
    for i, drv in enumerate([q0, m1, sq, c.gate("XOR", A=m0, B=cnt[2])]):
        c.out("out", i, drv)
    return {"ports": c.ports, "cells": c.cells}


def write_blueprint(directory):
    """core.json and system.toml in `directory`; returns the blueprint's path."""
    with open(os.path.join(directory, "core.json"), "w") as f:
        json.dump(core_json(), f)
    path = os.path.join(directory, "system.toml")
    with open(path, "w") as f:
        f.write(BLUEPRINT)
    return path


request = small.request   # a random program (the ROM image), a random initial RAM, no @inputs


# ---- where a cone belongs, computed apart from iyokan_amd.frontier ------------------------------------------------------------------------

def cone_depths(sysm, pt):
    """{gate: the number of gates of stage pt.stage on the longest path that ends in it} over the address cone of `pt`, by a memoised
    walk backwards from the address pins (stops at DFFs, sources and other stages; OUTPUT wires stand for their driver)."""
    nl, stages = sysm.nl, sysm.stages
    depth = {}

    def walk(i):
        while nl.kinds[i] == "OUTPUT":
            i = nl.ins[i][0]
        if nl.kinds[i] in ("INPUT", "DFF") or stages[i] != pt.stage:
            return 0
        if i not in depth:
            depth[i] = 0                                                            # (the netlist has no combinational loop)
            depth[i] = 1 + max([walk(j) for j in nl.ins[i]], default=0)
        return depth[i]

    import sys

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 20000))
    try:
        for a in pt.addr:
            walk(a)
    finally:
        sys.setrecursionlimit(limit)
    return depth


def level_of(plan):
    """{gate: its index in plan.levels}"""
    return {i: k for k, L in enumerate(plan.levels) for i in L["boot"] + L["ew"]}


def late_levels(nl, world=1, cost=None, spread=True):
    """A stand-in for frontier.plan_levels that places every gate at its LATEST level (ALAP): the same number of levels as
    levelise(), every gate with slack as far back as its consumers allow."""
    asap = nl.levelise()
    depth = len(asap)
    root = nl.roots()
    level = {i: k for k, lv in enumerate(asap) for i in lv}
    alap = {i: depth - 1 for i in level}
    for lv in reversed(asap):
        for i in lv:
            for j in nl.ins[i]:
                j = root[j]
                if j in alap:
                    alap[j] = min(alap[j], alap[i] - 1)
    out = [[] for _ in range(depth)]
    for lv in asap:
        for i in lv:
            out[alap[i]].append(i)
    return out


def programs(count, cycles, first=100):
    return [request(first + k, cycles) for k in range(count)]


def rng_bits(seed, n):
    return [int(b) for b in np.random.default_rng(seed).integers(0, 2, size=n)]
