"""The four-port system of the stage tests (test_cmux_stage_cb / test_gpu_cmux_stage_cb), written as a blueprint with one Iyokan-L1 core:

    a 3-bit counter and a wren register in DFFs drive THREE ports of one stage, all of different widths:
        rom   3-bit address x 4 bits    address = the counter
        rama  1-bit address x 1 bit     address = counter bit 2
        ramb  2-bit address x 2 bits    address = (counter bit 2, the wren register)
    ramc      1-bit address x 1 bit     address = rama's rdata                      -> the next stage
    every wren is the one register (it keeps a 1 once it holds one); wdata comes from the port's own rdata: rama keeps its bit while
    wren is 1, ramb counts (b0' = NOT b0, b1' = b1 XOR b0), ramc toggles

With the counter at 4 .. 7 and the register at 1 every clock addresses rama cell 1 and ramb cell 3, so each clock reads back through ramb
— and through ramc, behind rama's rdata — what the clock before wrote and refreshed."""
import json
import os

import cmux_system_cases as small

PORTS = (("rom", "rom", 3, 4), ("ram", "rama", 1, 1), ("ram", "ramb", 2, 2), ("ram", "ramc", 1, 1))

BLUEPRINT = """
[[file]]
type = "iyokanl1-json"
path = "core.json"
name = "core"

[[builtin]]
type = "rom"
name = "rom"
in_addr_width = 3
out_rdata_width = 4

[[builtin]]
type = "ram"
name = "rama"
in_addr_width = 1
in_wdata_width = 1
out_rdata_width = 1

[[builtin]]
type = "ram"
name = "ramb"
in_addr_width = 2
in_wdata_width = 2
out_rdata_width = 2

[[builtin]]
type = "ram"
name = "ramc"
in_addr_width = 1
in_wdata_width = 1
out_rdata_width = 1

[connect]
"rom/addr[0:2]" = "core/rom_addr[0:2]"
"core/romd[0:3]" = "rom/rdata[0:3]"
"rama/addr[0]" = "core/a_addr[0]"
"rama/wren" = "core/a_wren"
"rama/wdata[0]" = "core/a_wdata[0]"
"core/ar[0]" = "rama/rdata[0]"
"ramb/addr[0:1]" = "core/b_addr[0:1]"
"ramb/wren" = "core/b_wren"
"ramb/wdata[0:1]" = "core/b_wdata[0:1]"
"core/br[0:1]" = "ramb/rdata[0:1]"
"ramc/addr[0]" = "core/c_addr[0]"
"ramc/wren" = "core/c_wren"
"ramc/wdata[0]" = "core/c_wdata[0]"
"core/cr[0]" = "ramc/rdata[0]"
"core/reset" = "@reset"
"@out[0:3]" = "core/out[0:3]"
"""


def core_json():
    c = small._Core()
    reset = c.inp("reset", 0)
    romd = [c.inp("romd", i) for i in range(4)]
    ar, br, cr = c.inp("ar", 0), [c.inp("br", i) for i in range(2)], c.inp("cr", 0)
    cnt = [c.dff() for _ in range(3)]
    wq = c.dff()
    nxt = [c.gate("NOT", A=cnt[0]), c.gate("XOR", A=cnt[0], B=cnt[1]), c.gate("XOR", A=cnt[2], B=c.gate("AND", A=cnt[0], B=cnt[1]))]
    for d, x in zip(cnt, nxt):
        c.feed(d, c.gate("ANDNOT", A=x, B=reset))
    c.feed(wq, c.gate("OR", A=wq, B=romd[3]))
    for i in range(3):
        c.out("rom_addr", i, cnt[i])
    c.out("a_addr", 0, cnt[2])
    c.out("b_addr", 0, cnt[2])
    c.out("b_addr", 1, wq)
    c.out("c_addr", 0, ar)
    for name in ("a_wren", "b_wren", "c_wren"):
        c.out(name, 0, wq)
    c.out("a_wdata", 0, c.gate("XNOR", A=ar, B=wq))
    c.out("b_wdata", 0, c.gate("NOT", A=br[0]))
    c.out("b_wdata", 1, c.gate("XOR", A=br[1], B=br[0]))
    c.out("c_wdata", 0, c.gate("NOT", A=cr))
    for i, drv in enumerate([cnt[0], c.gate("XOR", A=cr, B=romd[0]), c.gate("XOR", A=br[0], B=br[1]), c.gate("XOR", A=ar, B=romd[1])]):
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


def request(seed, cycles):
    """A random ROM image and random initial RAMs, no @inputs."""
    import numpy as np

    from iyokan_amd.packet import PlainPacket

    rng = np.random.default_rng(seed)
    image = lambda a, w: [int(b) for b in rng.integers(0, 2, size=w << a)]
    return PlainPacket(rom={"rom": image(3, 4)}, ram={n: image(a, w) for k, n, a, w in PORTS if k == "ram"}, cycles=cycles)
