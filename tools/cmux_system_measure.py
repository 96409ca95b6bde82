"""Time per clock of a blueprint with rom / ram builtins, once as CMUX memories behind circuit bootstrapping (runner.CmuxCipherEngine) and
once lowered to the MUX form on the gate path (runner.CipherEngine), on the same GPU in one process.  Three systems: the small ROM + RAM
system of tests/cmux_system_cases.py, the 8-bit-address RAM of tests/golden/reftest/config-toml/ram-addr8bit.toml, and `three-port`, built
here: one ROM (7-bit address x 32 bits) and two RAMs (8 x 8) whose three ports are in ONE stage, all addressed by a counter in DFFs.

--stage-cb / --refresh-aside give the engine stage_cb=True / refresh_aside=True (runner.CmuxCipherEngine).  --ab compares: per system and
per flag set (each flag alone, both) three interleaved pairs of the flags-off engine and the flagged one, in this one process and build.

Keys have the real shapes (bk2 at n = 636; the private key-switching key n_in = 2048, t = 10, basebit = 3, 2.35 GB) and uniform content:
the kernels' time does not depend on the words.  Wall time per clock is tick() + run() over --clocks clocks between two stream
synchronisations.  The split is taken in a second pass that synchronises after every part of a port (rotation, private key switch +
selector assembly, read tree + extraction, write-back + refresh) and after the gate levels, so its parts add up to more than the wall time.

    python tools/cmux_system_measure.py [--clocks 3] [--rom-fused] > profiles/cmux_system_ab.txt
    python tools/cmux_system_measure.py --ab [--bk2-form fft] >> profiles/cmux_stage_ab.txt"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cmux_system_cases as cases  # noqa: E402
from iyokan_amd import client, cmux, hip, runner  # noqa: E402
from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend  # noqa: E402
from iyokan_amd.params import params_128bit  # noqa: E402
from iyokan_amd.system import load_blueprint  # noqa: E402


class SplitEngine(runner.CmuxCipherEngine):
    """the same launches, the circuit bootstrapping as its three calls, a synchronisation and a clock reading after every part"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ms = {"rotation": 0.0, "private key switch + selectors": 0.0, "read tree + extraction": 0.0, "write-back + refresh": 0.0, "gates": 0.0}
        self._t = None

    def _lap(self, what):
        self.stream.sync()
        now = time.perf_counter()
        self.ms[what] += (now - self._t) * 1e3
        self._t = now

    def run(self):
        self.stream.sync()
        self._t = time.perf_counter()
        super().run()
        self._lap("gates")

    def tick(self):
        self.stream.sync()
        self._t = time.perf_counter()
        super().tick()
        self._lap("gates")

    def _port_read(self, pt):
        self._lap("gates")
        p = hip.current_params()
        l, mem, slots = int(p.l), self.mem[pt.name], self._slots(pt.addr)
        in_ = np.repeat(slots, l)
        mu = np.tile(np.array([1 << (63 - (r + 1) * int(p.Bgbit)) for r in range(l)], dtype=np.uint64), len(slots))
        self.stream.cb_rotate_batch(self.bk2, self.arena, in_, [1] * len(in_), [0] * len(in_), mu, self.tlwe2, np.arange(len(in_)))
        self._lap("rotation")
        cmux.selectors_from_tlwe2(self.stream, self.privks_key, self.tlwe2, 0, pt.addr_width, self.scratch, mem.trgsw, 0)
        self._lap("private key switch + selectors")
        if pt.kind == "rom":
            mem.read(None, self.arena, self._slots(pt.rdata).reshape(1, -1), resident=True, fused=self.rom_fused)
        else:
            mem.read_port(self.arena, self._slots(pt.rdata))
        self._lap("read tree + extraction")

    def _port_write(self, pt):
        self._lap("gates")
        super()._port_write(pt)
        self._lap("write-back + refresh")


THREE_PORT = """
[[file]]
type = "iyokanl1-json"
path = "core.json"
name = "core"

[[builtin]]
type = "rom"
name = "rom"
in_addr_width = 7
out_rdata_width = 32

[[builtin]]
type = "ram"
name = "rama"
in_addr_width = 8
in_wdata_width = 8
out_rdata_width = 8

[[builtin]]
type = "ram"
name = "ramb"
in_addr_width = 8
in_wdata_width = 8
out_rdata_width = 8

[connect]
"rom/addr[0:6]" = "core/rom_addr[0:6]"
"core/romd[0:31]" = "rom/rdata[0:31]"
"rama/addr[0:7]" = "core/a_addr[0:7]"
"rama/wren" = "core/a_wren"
"rama/wdata[0:7]" = "core/a_wdata[0:7]"
"core/ar[0:7]" = "rama/rdata[0:7]"
"ramb/addr[0:7]" = "core/b_addr[0:7]"
"ramb/wren" = "core/b_wren"
"ramb/wdata[0:7]" = "core/b_wdata[0:7]"
"core/br[0:7]" = "ramb/rdata[0:7]"
"core/reset" = "@reset"
"@out[0:7]" = "core/out[0:7]"
"""


def write_three_port(directory):
    """config #4's shapes with every port in one stage: an 8-bit counter in DFFs is the address of the ROM (its low 7 bits) and of both
    RAMs, wren a DFF fed by ROM bit 31, wdata = rdata XOR ROM bits, @out = the two RAMs' rdata XORed"""
    c = cases._Core()
    reset = c.inp("reset", 0)
    romd = [c.inp("romd", i) for i in range(32)]
    ar, br = [c.inp("ar", i) for i in range(8)], [c.inp("br", i) for i in range(8)]
    cnt, wq = [c.dff() for _ in range(8)], c.dff()
    carry = None
    for i, d in enumerate(cnt):
        nxt = c.gate("NOT", A=d) if carry is None else c.gate("XOR", A=d, B=carry)
        carry = d if carry is None else c.gate("AND", A=d, B=carry)
        c.feed(d, c.gate("ANDNOT", A=nxt, B=reset))
    c.feed(wq, romd[31])
    for i in range(8):
        if i < 7:
            c.out("rom_addr", i, cnt[i])
        c.out("a_addr", i, cnt[i])
        c.out("b_addr", i, cnt[7 - i])
        c.out("a_wdata", i, c.gate("XOR", A=ar[i], B=romd[i]))
        c.out("b_wdata", i, c.gate("XOR", A=br[i], B=romd[8 + i]))
        c.out("out", i, c.gate("XOR", A=ar[i], B=br[i]))
    c.out("a_wren", 0, wq)
    c.out("b_wren", 0, wq)
    with open(os.path.join(directory, "core.json"), "w") as f:
        json.dump({"ports": c.ports, "cells": c.cells}, f)
    path = os.path.join(directory, "system.toml")
    with open(path, "w") as f:
        f.write(THREE_PORT)
    return path


def engine(keys, sysm, kind, bk2=None, pk=None, rom_fused=False, **flags):
    import torch

    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0))
    enc, dec, zero = (lambda bits: client.encrypt_bits(keys, bits, seed=5)), (lambda rows: client.decrypt_bits(keys, rows)), client.trivial(keys.params, 0)
    ex = FrontierExecutor(plan, be)
    if kind == "mux":
        return runner.CipherEngine(ex, enc, dec, zero), be, plan
    cls = SplitEngine if kind == "split" else runner.CmuxCipherEngine
    return cls(sysm, ex, enc, dec, zero, bk2, pk, rom_fused=rom_fused, **flags), be, plan


def clocks(eng, be, sysm, n):
    rng = np.random.default_rng(1)
    nids = list(sysm.nl.inputs.values())
    eng.set_nodes(nids, rng.integers(0, 2, size=len(nids)))
    eng.run()
    eng.tick()
    eng.run()                                                                       # one clock to warm up
    be.sync()
    gc.collect()                                                                    # no collection of the lowered netlists inside the timed clocks
    gc.disable()
    try:
        t = time.perf_counter()
        for _ in range(n):
            eng.tick()
            eng.run()
        be.sync()
        if getattr(eng, "refresh_stream", None) is not None:
            eng.refresh_stream.sync()                                               # the last clock's refresh counts
        return (time.perf_counter() - t) * 1e3 / max(n, 1)
    finally:
        gc.enable()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clocks", type=int, default=3)
    ap.add_argument("--bk2-form", choices=sorted(hip.Bk2Key.FORMS), default="ntt",
                    help="the lvl2 bootstrapping key's form: ntt = the integer key, fft = the FP64 key (cb_rotate_fft_kernel)")
    ap.add_argument("--rom-fused", action="store_true",
                    help="the rotate tail of every ROM read as ONE cmux_rotate_chain_batch (Rom.read(fused=True)) instead of one cmux_batch per step")
    ap.add_argument("--small-only", action="store_true", help="the small ROM + RAM system alone (the one with a ROM)")
    ap.add_argument("--stage-cb", action="store_true", help="one circuit bootstrapping batch per stage (CmuxCipherEngine(stage_cb=True))")
    ap.add_argument("--refresh-aside", action="store_true", help="the RAMs' refresh on a second stream (CmuxCipherEngine(refresh_aside=True))")
    ap.add_argument("--ab", action="store_true", help="per system: three interleaved pairs flags-off / flagged for each flag alone and both")
    args = ap.parse_args()
    flags = {k: True for k, on in (("stage_cb", args.stage_cb), ("refresh_aside", args.refresh_aside)) if on}
    keys = client.keygen(params_128bit(), seed=1)
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    rng = np.random.default_rng(2)
    bk2 = hip.Bk2Key(keys.params.n, form=args.bk2_form)
    for first in range(0, bk2.n, 100):
        count = min(100, bk2.n - first)
        bk2.upload(st, first, rng.integers(0, 1 << 63, size=(count, bk2.step_words), dtype=np.uint64))
    pk = hip.PrivKsKey(2048, 10, 3)
    window = rng.integers(0, 1 << 32, size=(8192, pk.words), dtype=np.uint64).astype(np.uint32)
    for first in range(0, pk.rows, 8192):
        pk.upload(st, first, window[:min(8192, pk.rows - first)])
    st.sync()
    print(f"build {hip.build_id()}; {args.clocks} clocks per figure; 128-bit set; bk2 n = {bk2.n} form {bk2.form}, private key n_in = 2048, t = 10, basebit = 3; "
          f"ROM rotate tail {'fused (one cmux_rotate_chain_batch)' if args.rom_fused else 'unfused (one cmux_batch per step)'}"
          f"; engine flags {flags or 'none'}")
    tmp = tempfile.mkdtemp()
    systems = [("small: ROM 3-bit address x 4 bits, RAM 2-bit address x 2 bits, 12 gates", cases.write_blueprint(tmp)),
               ("ram-addr8bit: RAM 8-bit address x 8 bits", os.path.join(ROOT, "tests", "golden", "reftest", "config-toml", "ram-addr8bit.toml")),
               ("three-port: ROM 7-bit address x 32 bits, two RAMs 8-bit address x 8 bits, all three ports in one stage", write_three_port(tempfile.mkdtemp()))]
    for title, path in systems[:1] if args.small_only else systems:
        print(f"\n== {title}")
        lowered, ported = load_blueprint(path), load_blueprint(path, cmux_memories=True)
        if args.ab:
            stages = sorted({pt.stage for pt in ported.ports})
            print(f"   {len(ported.ports)} ports in {len(stages)} stages with ports; ms per clock, pairs run off then on, three times")
            for name, fl in (("stage_cb", {"stage_cb": True}), ("refresh_aside", {"refresh_aside": True}),
                             ("stage_cb + refresh_aside", {"stage_cb": True, "refresh_aside": True})):
                pairs = []
                for _ in range(3):
                    pair = []
                    for f in ({}, fl):
                        eng, be, _ = engine(keys, ported, "cmux", bk2, pk, args.rom_fused, **f)
                        pair.append(clocks(eng, be, ported, args.clocks))
                        eng.free()
                        be.close()
                    pairs.append(pair)
                off, on = np.array(pairs).T
                print(f"   {name:26s} off {' '.join(f'{v:8.2f}' for v in off)}   on {' '.join(f'{v:8.2f}' for v in on)}   "
                      f"median off {np.median(off):8.2f}  on {np.median(on):8.2f}  on - off {np.median(on) - np.median(off):+8.2f}  "
                      f"(spread of off {off.max() - off.min():.2f})")
            continue
        eng, be, plan = engine(keys, lowered, "mux")
        ms = clocks(eng, be, lowered, args.clocks)
        print(f"lowered MUX form : {ms:9.2f} ms per clock   ({lowered.nl.rotations()} rotations, {len(plan.levels)} levels)")
        be.close()
        eng, be, plan = engine(keys, ported, "cmux", bk2, pk, args.rom_fused, **flags)
        ms = clocks(eng, be, ported, args.clocks)
        rot = sum(pt.addr_width for pt in ported.ports) * int(keys.params.l)
        print(f"CMUX memories    : {ms:9.2f} ms per clock   ({ported.nl.rotations()} gate rotations, {len(plan.levels)} levels, "
              f"{len(ported.ports)} ports, {rot} lvl2 rotations in {len(ported.ports)} batches)")
        eng.free()
        be.close()
        eng, be, _ = engine(keys, ported, "split", bk2, pk, args.rom_fused)
        clocks(eng, be, ported, 0)
        for k in eng.ms:
            eng.ms[k] = 0.0
        n = max(1, args.clocks - 1)
        for _ in range(n):
            eng.tick()
            eng.run()
        for k, v in eng.ms.items():
            print(f"    {k:32s} {v / n:9.2f} ms per clock (synchronised after every part)")
        eng.free()
        be.close()
    bk2.free()
    pk.free()
    st.destroy()
    hip.cleanup()


if __name__ == "__main__":
    main()
