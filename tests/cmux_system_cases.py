"""The small system of the CMUX-memory tests (test_cmux_system / test_gpu_cmux_system), written as a blueprint with one Iyokan-L1 core:

    a 3-bit counter in DFFs drives a ROM (3-bit address x 4 bits) directly            -> the ROM port is stage 0, its rdata stage 1
    ROM data and the counter drive the RAM's address (2-bit address x 2 bits)          -> the RAM port is stage 1, its rdata stage 2
    wren comes STRAIGHT from a DFF (fed by ROM bit 3), wdata from the RAM's own rdata  -> gates of stage 2
    the RAM's rdata is latched by two DFFs; @out reads DFFs and gates of stages 0, 1 and 2

loop=True feeds the RAM's address from its own rdata.  Also a digest of a system and of a plan, for comparing against recorded ones."""
import hashlib
import json
import os

import numpy as np

ROM_SHAPE, RAM_SHAPE = (3, 4), (2, 2)

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
name = "ram"
in_addr_width = 2
in_wdata_width = 2
out_rdata_width = 2

[connect]
"rom/addr[0:2]" = "core/rom_addr[0:2]"
"core/romd[0:3]" = "rom/rdata[0:3]"
"ram/addr[0:1]" = "core/ram_addr[0:1]"
"ram/wren" = "core/wren"
"ram/wdata[0:1]" = "core/wdata[0:1]"
"core/ramr[0:1]" = "ram/rdata[0:1]"
"core/reset" = "@reset"
"@out[0:3]" = "core/out[0:3]"
"""


class _Core:
    def __init__(self):
        self.ports, self.cells, self.n = [], [], 0

    def _id(self):
        self.n += 1
        return self.n

    def inp(self, name, bit):
        i = self._id()
        self.ports.append({"type": "input", "id": i, "portName": name, "portBit": bit, "bits": []})
        return i

    def out(self, name, bit, driver):
        self.ports.append({"type": "output", "id": self._id(), "portName": name, "portBit": bit, "bits": [driver]})

    def gate(self, kind, **inputs):
        i = self._id()
        self.cells.append({"type": kind, "id": i, "input": inputs})
        return i

    def dff(self):
        return self.gate("DFFP", D=None)

    def feed(self, dff, driver):
        next(c for c in self.cells if c["id"] == dff)["input"]["D"] = driver


def core_json(loop=False):
    c = _Core()
    reset = c.inp("reset", 0)
    romd = [c.inp("romd", i) for i in range(4)]
    ramr = [c.inp("ramr", i) for i in range(2)]
    cnt = [c.dff() for _ in range(3)]
    wq, q0, q1 = c.dff(), c.dff(), c.dff()
    nxt = [c.gate("NOT", A=cnt[0]), c.gate("XOR", A=cnt[0], B=cnt[1]), c.gate("XOR", A=cnt[2], B=c.gate("AND", A=cnt[0], B=cnt[1]))]
    for d, x in zip(cnt, nxt):
        c.feed(d, c.gate("ANDNOT", A=x, B=reset))
    for i in range(3):
        c.out("rom_addr", i, cnt[i])
    ra0 = c.gate("XOR", A=ramr[0] if loop else romd[0], B=cnt[0])
    ra1 = c.gate("XOR", A=romd[1], B=romd[2])
    c.out("ram_addr", 0, ra0)
    c.out("ram_addr", 1, ra1)
    c.feed(wq, romd[3])
    c.out("wren", 0, wq)
    wd0, wd1 = c.gate("XOR", A=ramr[0], B=romd[2]), c.gate("XNOR", A=ramr[1], B=romd[0])
    c.out("wdata", 0, wd0)
    c.out("wdata", 1, wd1)
    c.feed(q0, ramr[0])
    c.feed(q1, ramr[1])
    for i, drv in enumerate([q0, c.gate("XOR", A=q1, B=cnt[2]), wd0, ra0]):
        c.out("out", i, drv)
    return {"ports": c.ports, "cells": c.cells}


def write_blueprint(directory, loop=False):
    """core.json and system.toml in `directory`; returns the blueprint's path."""
    with open(os.path.join(directory, "core.json"), "w") as f:
        json.dump(core_json(loop), f)
    path = os.path.join(directory, "system.toml")
    with open(path, "w") as f:
        f.write(BLUEPRINT)
    return path


def request(seed, cycles):
    """A random program (the ROM image), a random initial RAM, no @inputs."""
    from iyokan_amd.packet import PlainPacket

    rng = np.random.default_rng(seed)
    rom = [int(b) for b in rng.integers(0, 2, size=ROM_SHAPE[1] << ROM_SHAPE[0])]
    ram = [int(b) for b in rng.integers(0, 2, size=RAM_SHAPE[1] << RAM_SHAPE[0])]
    return PlainPacket(rom={"rom": rom}, ram={"ram": ram}, cycles=cycles)


def _sha(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def system_digest(sysm):
    nl = sysm.nl
    table = lambda t: sorted([list(map(str, k)), v] for k, v in t.items())
    return _sha([nl.kinds, nl.ins, table(nl.inputs), table(nl.outputs), table(nl.ram), sorted(map(str, nl.dff_init.items())),
                 {n: sorted(c.items()) for n, c in sysm.rom.items()}, {n: sorted(c.items()) for n, c in sysm.ram.items()}])


def plan_digest(plan):
    return _sha([[[L["boot"], L["ew"], L["base"], L["B"]] for L in plan.levels], plan.slot, plan.num_slots, plan.shadow_base])


# ---- one clock on the GPU, every selector-derived word against the composed restatement ---------------------------------------------------


def gpu_engine(keys, sysm, bk2, pk, packet, **kw):
    """A CmuxCipherEngine on cuda:0 for `sysm` with fresh HipBackend; returns (engine, backend)."""
    import torch

    from iyokan_amd import client, runner
    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend

    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0))
    seed = {"v": 9000}

    def encrypt(bits):
        seed["v"] += 1
        return client.encrypt_bits(keys, bits, seed=seed["v"])

    try:
        eng = runner.CmuxCipherEngine(sysm, FrontierExecutor(plan, be), encrypt, lambda rows: client.decrypt_bits(keys, rows),
                                      client.trivial(keys.params, 0), bk2, pk, packet=packet,
                                      decrypt_ram=lambda rows: client.decrypt_ram_trlwe(keys, rows), **kw)
    except Exception:
        be.close()                                                                  # a refusal leaves no stream behind
        raise
    return eng, be


def restated_selectors(p, tlwes, ntt, K):
    """emul_rotate -> privks_ref of every address bit (uniform key K, t = 1, basebit = 1): u32 [bits][(k+1) l][k+1][N]"""
    from concurrent.futures import ThreadPoolExecutor

    import cb_rotate_cases
    import cb_rotate_ref
    import privks_ref

    l = int(p.l)
    jobs = [(t, cb_rotate_ref.mu_of(r, p.Bgbit)) for t in tlwes for r in range(l)]
    with ThreadPoolExecutor(max_workers=8) as pool:                                 # the emulation releases the GIL
        rot = list(pool.map(lambda j: cb_rotate_cases.emul_rotate(j[0], 1, 0, j[1], ntt), jobs))
    row_fn = privks_ref.key_rows_of(K)
    return np.stack([privks_ref.selector_rows(rot[b * l:(b + 1) * l], 1, 1, row_fn, l) for b in range(len(tlwes))])


def one_clock_words(keys, orc, sysm, bk_host, K, bk2, pk, **kw):
    """One run() + tick() of the small system from a chosen register state; asserts the ROM result row, the rdata TLWEs of both
    memories and the RAM cells after tick() word for word against emul_rotate -> privks_ref -> cmux_ref / ram_ref on the TLWEs that
    were in the arena's address / wren / wdata slots."""
    import cb_rotate_cases
    import cmux_ref
    import ram_ref
    from iyokan_amd.packet import TFHEPacket

    p = keys.params
    N = int(p.N)
    packet = TFHEPacket.encrypt(keys, request(3, 1), seed=500)
    eng, be = gpu_engine(keys, sysm, bk2, pk, packet, **kw)
    try:
        rom, ram = sysm.ports
        eng.load_rom("rom", None)
        eng.load_ram("ram", None)
        root, slot = sysm.nl.roots(), eng.ex.plan.slot
        regs = [root[a] for a in rom.addr] + [root[ram.wren[0]]]
        assert all(sysm.nl.kinds[i] == "DFF" for i in regs)
        eng.set_nodes(regs, [1, 0, 1, 1])                                            # counter = 5, wren = 1
        rom_mem, ram_mem = eng.mem["rom"], eng.mem["ram"]
        cells0 = ram_mem.cells()
        eng.run()
        read = lambda nodes: be.read_many([slot[i] for i in nodes])
        a_rom, d_rom, a_ram, d_ram, wren, wdata = (read(x) for x in (rom.addr, rom.rdata, ram.addr, ram.rdata, ram.wren, ram.wdata))
        rom_row = rom_mem.trlwe.download(eng.stream, rom_mem.row(0, rom_mem.layout.result), 1)[0]
        eng.tick()
        cells1 = ram_mem.cells()
        regs_after = read(regs[:3])
    finally:
        eng.free()
        be.close()
    ntt = cb_rotate_cases.key_ntt(bk_host)
    want_row = cmux_ref.rom_read(p, np.asarray(packet.rom["rom"], dtype=np.uint32).reshape(-1, 2 * N), restated_selectors(p, a_rom, ntt, K), 3, 2)
    assert np.array_equal(rom_row, want_row), np.flatnonzero(rom_row != want_row)[:8]
    for i in range(4):
        assert np.array_equal(d_rom[i], orc.keyswitch(cmux_ref.sample_extract_index(want_row, i, N))), i
    image = np.asarray(packet.ram["ram"], dtype=np.uint32).reshape(4, 2, 2 * N).transpose(1, 0, 2)
    assert np.array_equal(cells0, image)                                            # the packet's order became planes of cells
    rdata, _, cells = ram_ref.clock(p, orc, cells0, restated_selectors(p, a_ram, ntt, K), wren[0], wdata)
    assert np.array_equal(d_ram, rdata)
    bad = np.argwhere((cells1 != cells).any(axis=2))
    assert bad.size == 0, bad[:8]
    assert (cells1 != cells0).any(axis=2).all()                                     # every cell was refreshed
    assert not np.array_equal(regs_after, a_rom)                                    # the registers did latch (the ORDER is the bits twin's test)
