"""What K lanes gain on a circuit behind CMUX memories ("CMUX memories per lane"): ms per clock and request-clocks
per second of runner.CmuxLaneEngine with K = 2, 4, 8 lanes, each against the one-lane runner.CmuxCipherEngine beside it.

Systems: ram-addr8bit, and cahp-ruby loaded with cmux_memories=True (the bare core behind its ROM and RAMs).  Keys: the integer and the
FP64 lvl2 key (--bk2-form).  Method: --pairs interleaved pairs (K = 1, then K lanes) per K in ONE process; a figure is tick() + run() over
--clocks clocks between two stream synchronisations, after one warm-up clock; median (min .. max) of the pairs.  Keys have the real
shapes and uniform content, as in tools/cmux_system_measure.py: the kernels' time does not depend on the words.  All flags off.

--defaults: the flags-off one-lane CmuxCipherEngine clock alone, --pairs figures, one line — for the comparison of two builds (run it
once per tree, alternating; --root names the tree whose package and library are used, so the same script measures both).

    python tools/cmux_lanes_measure.py --bk2-form ntt >> profiles/cmux_lanes_ab.txt
    python tools/cmux_lanes_measure.py --bk2-form fft >> profiles/cmux_lanes_ab.txt
    python tools/cmux_lanes_measure.py --defaults [--root OTHER_TREE] >> profiles/cmux_lanes_ab.txt"""
import argparse
import gc
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_plans = {}


def engine(m, keys, sysm, bk2, pk, lanes):
    import torch

    if id(sysm) not in _plans:   # the single-lane plan, made once per system: every engine of the system shares it
        _plans[id(sysm)] = m.FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    plan = _plans[id(sysm)]
    be = m.HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0), **({"lanes": lanes} if lanes > 1 else {}))
    common = (sysm, m.FrontierExecutor(plan, be), lambda bits: m.client.encrypt_bits(keys, bits, seed=5),
              lambda rows: m.client.decrypt_bits(keys, rows), m.client.trivial(keys.params, 0), bk2, pk)
    eng = m.runner.CmuxLaneEngine(*common) if lanes > 1 else m.runner.CmuxCipherEngine(*common)
    return eng, be


def clocks(eng, be, sysm, n, lanes):
    rng = np.random.default_rng(1)
    nids = list(sysm.nl.inputs.values())
    for lane in range(lanes):
        eng.set_nodes(nids, rng.integers(0, 2, size=len(nids)), **({"lane": lane} if lane else {}))
    eng.run()
    eng.tick()
    eng.run()                                                                       # one clock to warm up
    be.sync()
    gc.collect()
    gc.disable()
    try:
        t = time.perf_counter()
        for _ in range(n):
            eng.tick()
            eng.run()
        be.sync()
        return (time.perf_counter() - t) * 1e3 / max(n, 1)
    finally:
        gc.enable()


def one(m, keys, sysm, bk2, pk, lanes, n):
    eng, be = engine(m, keys, sysm, bk2, pk, lanes)
    try:
        return clocks(eng, be, sysm, n, lanes)
    finally:
        eng.free()
        be.close()


def fmt(v):
    return f"{np.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clocks", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--lanes", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--bk2-form", default="ntt", help="ntt = the integer lvl2 key, fft = the FP64 key")
    ap.add_argument("--systems", nargs="+", default=["ram-addr8bit", "cahp-ruby"])
    ap.add_argument("--defaults", action="store_true", help="the flags-off one-lane CmuxCipherEngine clock of ram-addr8bit alone")
    ap.add_argument("--root", default=HERE, help="the tree whose iyokan_amd package and library are measured")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)

    class m:   # the measured tree's modules
        from iyokan_amd import client, hip, runner
        from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend
        from iyokan_amd.params import params_128bit
        from iyokan_amd.system import load_blueprint

    keys = m.client.keygen(m.params_128bit(), seed=1)
    m.hip.initialize(keys, device_ids=(0,))
    st = m.hip.Stream(0)
    rng = np.random.default_rng(2)
    bk2 = m.hip.Bk2Key(keys.params.n, form=args.bk2_form)
    for first in range(0, bk2.n, 100):
        count = min(100, bk2.n - first)
        bk2.upload(st, first, rng.integers(0, 1 << 63, size=(count, bk2.step_words), dtype=np.uint64))
    pk = m.hip.PrivKsKey(2048, 10, 3)
    window = rng.integers(0, 1 << 32, size=(8192, pk.words), dtype=np.uint64).astype(np.uint32)
    for first in range(0, pk.rows, 8192):
        pk.upload(st, first, window[:min(8192, pk.rows - first)])
    st.sync()
    gold = os.path.join(root, "tests", "golden", "reftest", "config-toml")
    head = f"build {m.hip.build_id()}; bk2 form {bk2.form}; {args.clocks} clocks per figure; 128-bit set; flags off"
    if args.defaults:
        sysm = m.load_blueprint(os.path.join(gold, "ram-addr8bit.toml"), cmux_memories=True)
        v = [one(m, keys, sysm, bk2, pk, 1, args.clocks) for _ in range(args.pairs)]
        print(f"defaults  {head}; ram-addr8bit, CmuxCipherEngine, ms per clock: {' '.join(f'{x:.2f}' for x in v)}   median {fmt(v)}", flush=True)
    else:
        print(f"\n{head}; {args.pairs} interleaved pairs (K = 1, then K lanes) per K, median (min .. max)", flush=True)
        for name in args.systems:
            sysm = m.load_blueprint(os.path.join(gold, name + ".toml"), cmux_memories=True)
            bits = [pt.addr_width for pt in sysm.ports]
            print(f"== {name}: {len(sysm.ports)} ports, address bits {bits}, {sysm.nl.rotations()} gate rotations per clock", flush=True)
            print("   K | K = 1 beside it, ms per clock | K lanes, ms per clock | clock | request-clocks / s", flush=True)
            for K in args.lanes:
                a, b = [], []
                for _ in range(args.pairs):
                    a.append(one(m, keys, sysm, bk2, pk, 1, args.clocks))
                    b.append(one(m, keys, sysm, bk2, pk, K, args.clocks))
                ma, mb = float(np.median(a)), float(np.median(b))
                print(f"   {K} | {fmt(a)} | {fmt(b)} | x {mb / ma:.2f} | {1e3 / ma:.2f} -> {K * 1e3 / mb:.2f} (x {K * ma / mb:.2f})", flush=True)
    bk2.free()
    pk.free()
    st.destroy()
    m.hip.cleanup()


if __name__ == "__main__":
    main()
