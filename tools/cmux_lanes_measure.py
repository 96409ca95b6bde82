"""What K lanes gain on a circuit behind CMUX memories ("CMUX memories per lane"): ms per clock and request-clocks
per second of runner.CmuxLaneEngine with K = 2, 4, 8 lanes, each against the one-lane runner.CmuxCipherEngine beside it.

Systems: ram-addr8bit, and cahp-ruby loaded with cmux_memories=True (the bare core behind its ROM and RAMs).  Keys: the integer and the
FP64 lvl2 key (--bk2-form).  Method: --pairs interleaved pairs (K = 1, then K lanes) per K in ONE process; a figure is tick() + run() over
--clocks clocks between two stream synchronisations, after one warm-up clock; median (min .. max) of the pairs.  Keys have the real
shapes and uniform content, as in tools/cmux_system_measure.py: the kernels' time does not depend on the words.  All flags off.

--defaults: the flags-off one-lane CmuxCipherEngine clock alone, --pairs figures, one line — for the comparison of two builds (run it
once per tree, alternating; --root names the tree whose package and library are used, so the same script measures both).

--read-early: what reading a port as soon as its address is ready gains ("Ports read early"): per system — cahp-ruby
behind CMUX memories, section 6e's small system (tests/cmux_system_cases.py) and ram-addr8bit, which has no gate and is the control where
nothing can move — per K in --lanes (default 1 and 8) and per flag set (none, stage_cb, refresh_aside, both, the fused read forms
rom_fused + tree_fused, all four; --sets picks), --pairs interleaved pairs of the engine with those flags and the same engine with
read_early=True, in ONE process; a figure as above, the refresh stream included.  The flag-off engine runs the plan of before the flag,
the flagged one FrontierPlan(early=ports); the model price of both plans is printed.

--snapshot: what saving and resuming a run costs ("Snapshot and resume"): per system (ram-addr8bit, cahp-ruby behind
CMUX memories) and K in --lanes (default 1 and 8), flags off: the ms per clock of that engine as above, then --pairs times state() +
Snapshot.save() of it into a temporary directory and Snapshot.load() + load_state() into a second, fresh engine of the same shape (up to
the synchronisation of its streams, the rebuilt selectors included); median (min .. max), and the file's size.

--cb-many: what one lvl2 rotation per address bit gains on a clock (the many-digit form): per system — ram-addr8bit
and the three-port system of tools/cmux_system_measure.py (23 address bits in one stage) — and K in --lanes (default 1 and 8), flags off
but for stage_cb on the three-port system (its one batch per stage is the 23 x K x l rotations the form divides by l): --pairs
interleaved pairs of the engine with cb_many off and on, in ONE process; a figure as above.

    python tools/cmux_lanes_measure.py --cb-many --pairs 3 >> profiles/cb_many_ab.txt
    python tools/cmux_lanes_measure.py --snapshot --pairs 3 >> profiles/snapshot_cost.txt
    python tools/cmux_lanes_measure.py --bk2-form ntt >> profiles/cmux_lanes_ab.txt
    python tools/cmux_lanes_measure.py --bk2-form fft >> profiles/cmux_lanes_ab.txt
    python tools/cmux_lanes_measure.py --defaults [--root OTHER_TREE] >> profiles/cmux_lanes_ab.txt
    python tools/cmux_lanes_measure.py --read-early --bk2-form ntt >> profiles/cmux_read_early_ab.txt
    python tools/cmux_lanes_measure.py --defaults --systems cahp-ruby ram-addr8bit [--root OTHER_TREE] >> profiles/cmux_read_early_ab.txt"""
import argparse
import gc
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_plans = {}


def plan_of(m, sysm, early=False):
    """the single-lane plan, made once per system (and once more with the address cones hoisted): every engine of the system shares it"""
    if (id(sysm), early) not in _plans:
        _plans[(id(sysm), early)] = m.FrontierPlan(sysm.nl, 1, stages=sysm.stages, **({"early": sysm.ports} if early else {}))
    return _plans[(id(sysm), early)]


def engine(m, keys, sysm, bk2, pk, lanes, **flags):
    import torch

    plan = plan_of(m, sysm, bool(flags.get("read_early")))
    be = m.HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0), **({"lanes": lanes} if lanes > 1 else {}))
    common = (sysm, m.FrontierExecutor(plan, be), lambda bits: m.client.encrypt_bits(keys, bits, seed=5),
              lambda rows: m.client.decrypt_bits(keys, rows), m.client.trivial(keys.params, 0), bk2, pk)
    eng = m.runner.CmuxLaneEngine(*common, **flags) if lanes > 1 else m.runner.CmuxCipherEngine(*common, **flags)
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
        be.sync()                                                                   # run() ends with the executor's stream behind every read
        if getattr(eng, "refresh_stream", None) is not None:
            eng.refresh_stream.sync()                                               # the last clock's refresh counts
        return (time.perf_counter() - t) * 1e3 / max(n, 1)
    finally:
        gc.enable()


def one(m, keys, sysm, bk2, pk, lanes, n, **flags):
    eng, be = engine(m, keys, sysm, bk2, pk, lanes, **flags)
    try:
        return clocks(eng, be, sysm, n, lanes)
    finally:
        eng.free()
        be.close()


def fmt(v):
    return f"{np.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


def model_ms(m, sysm, plan):
    """the level-cost model's price of a plan's gate levels (frontier.with_sub_pass_shape of the compiled-in table), ms per clock"""
    from iyokan_amd import frontier

    price = frontier.with_sub_pass_shape(frontier.mi355x_level_cost)
    return sum(price(r) for r in frontier.level_rotations(sysm.nl, [L["boot"] + L["ew"] for L in plan.levels]))


FLAG_SETS = (("no other flag", {}), ("stage_cb", {"stage_cb": True}), ("refresh_aside", {"refresh_aside": True}),
             ("stage_cb + refresh_aside", {"stage_cb": True, "refresh_aside": True}),
             # a read in few calls: with the unfused trees a port of 7 or 8 address bits is more than the eight calls a stream stages ahead
             ("rom_fused + tree_fused", {"rom_fused": True, "tree_fused": True}),
             ("all four", {"stage_cb": True, "refresh_aside": True, "rom_fused": True, "tree_fused": True}))


def read_early_leg(m, args, keys, bk2, pk, head, gold):
    import tempfile

    sys.path.insert(0, os.path.join(HERE, "tests"))
    import cmux_system_cases

    paths = {"small": cmux_system_cases.write_blueprint(tempfile.mkdtemp())}
    print(f"\n{head.replace('; flags off', '')}; read_early: {args.pairs} interleaved pairs (flag off, then on) per line, ms per clock, "
          f"median (min .. max)", flush=True)
    for name in args.systems or ["cahp-ruby", "small", "ram-addr8bit"]:
        sysm = m.load_blueprint(paths.get(name) or os.path.join(gold, name + ".toml"), cmux_memories=True)
        base, early = plan_of(m, sysm), plan_of(m, sysm, True)
        ready = {pt.name: early.port_ready[pt.name] - early.stage_levels[pt.stage].start for pt in sysm.ports}
        print(f"== {name}: {len(sysm.ports)} ports, address bits {[pt.addr_width for pt in sysm.ports]}, {sysm.nl.rotations()} gate rotations per clock, "
              f"levels per stage {[len(r) for r in early.stage_levels]}; levels of its stage a port's address needs: {ready}", flush=True)
        print(f"   model price of the gate levels: {model_ms(m, sysm, base):.2f} ms as planned, {model_ms(m, sysm, early):.2f} ms with the cones hoisted", flush=True)
        print("   K | flags beside read_early   | off                         | on                          | on - off (medians) | every pair outside the larger spread", flush=True)
        for K in args.lanes or [1, 8]:
            for title, flags in (FLAG_SETS if args.sets is None else [FLAG_SETS[i] for i in args.sets]):
                off, on = [], []
                for _ in range(args.pairs):
                    off.append(one(m, keys, sysm, bk2, pk, K, args.clocks, **flags))
                    on.append(one(m, keys, sysm, bk2, pk, K, args.clocks, read_early=True, **flags))
                spread = max(max(off) - min(off), max(on) - min(on))
                clear = all(abs(a - b) > spread for a, b in zip(off, on)) and len({a > b for a, b in zip(off, on)}) == 1
                print(f"   {K} | {title:25s} | {fmt(off)} | {fmt(on)} | {np.median(on) - np.median(off):+9.2f} | {'yes' if clear else 'no'}", flush=True)


def cb_many_leg(m, args, keys, bk2, pk, head, gold):
    import tempfile

    sys.path.insert(0, os.path.join(HERE, "tools"))
    import cmux_system_measure

    l = int(keys.params.l)
    systems = {"ram-addr8bit": (os.path.join(gold, "ram-addr8bit.toml"), {}),
               "three-port": (cmux_system_measure.write_three_port(tempfile.mkdtemp()), {"stage_cb": True})}
    print(f"\n{head.replace('; flags off', '')}; cb_many: {args.pairs} interleaved pairs (off, then on) per line, ms per clock, median (min .. max)",
          flush=True)
    print("   system | flags | K | lvl2 rotations of the widest batch, off -> on | off | on | on / off | every pair outside the larger spread", flush=True)
    for name in args.systems or ["ram-addr8bit", "three-port"]:
        path, flags = systems[name]
        sysm = m.load_blueprint(path, cmux_memories=True)
        for K in args.lanes or [1, 8]:
            off, on = [], []
            for _ in range(args.pairs):
                off.append(one(m, keys, sysm, bk2, pk, K, args.clocks, **flags))
                on.append(one(m, keys, sysm, bk2, pk, K, args.clocks, cb_many=True, **flags))
            bits = K * (sum(pt.addr_width for pt in sysm.ports) if flags else max(pt.addr_width for pt in sysm.ports))
            spread = max(max(off) - min(off), max(on) - min(on))
            clear = all(abs(a - b) > spread for a, b in zip(off, on)) and len({a > b for a, b in zip(off, on)}) == 1
            print(f"   {name} | {' + '.join(flags) or 'none'} | {K} | {bits * l} -> {bits} | {fmt(off)} | {fmt(on)} | "
                  f"{np.median(on) / np.median(off):.2f} | {'yes' if clear else 'no'}", flush=True)


def snapshot_leg(m, args, keys, bk2, pk, head, gold):
    import shutil
    import tempfile

    from iyokan_amd.snapshot import Snapshot

    print(f"\n{head}; snapshot: state() + save() and load() + load_state(), {args.pairs} times each, ms, median (min .. max)", flush=True)
    print("   system | K | ms per clock | state() + save() | load() + load_state() | file, MB", flush=True)
    where = tempfile.mkdtemp()
    path = os.path.join(where, "run.snapshot")
    try:
        for name in args.systems or ["ram-addr8bit", "cahp-ruby"]:
            sysm = m.load_blueprint(os.path.join(gold, name + ".toml"), cmux_memories=True)
            for K in args.lanes or [1, 8]:
                eng, be = engine(m, keys, sysm, bk2, pk, K)
                fresh, fresh_be = engine(m, keys, sysm, bk2, pk, K)
                try:
                    clock = clocks(eng, be, sysm, args.clocks, K)
                    save, load = [], []
                    for _ in range(args.pairs):
                        t = time.perf_counter()
                        eng.state(done=args.clocks + 1).save(path)
                        save.append((time.perf_counter() - t) * 1e3)
                        t = time.perf_counter()
                        fresh.load_state(Snapshot.load(path))
                        fresh_be.sync()
                        fresh.mem_stream.sync()
                        load.append((time.perf_counter() - t) * 1e3)
                    print(f"   {name} | {K} | {clock:9.2f} | {fmt(save)} | {fmt(load)} | {os.path.getsize(path) / 1e6:.1f}", flush=True)
                finally:
                    for e, b in ((eng, be), (fresh, fresh_be)):
                        e.free()
                        b.close()
    finally:
        shutil.rmtree(where)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clocks", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--lanes", type=int, nargs="+", default=None, help="default 2 4 8; with --read-early 1 8")
    ap.add_argument("--bk2-form", default="ntt", help="ntt = the integer lvl2 key, fft = the FP64 key")
    ap.add_argument("--systems", nargs="+", default=None, help="default ram-addr8bit cahp-ruby; --defaults: ram-addr8bit; --read-early: cahp-ruby small ram-addr8bit")
    ap.add_argument("--defaults", action="store_true", help="the flags-off one-lane CmuxCipherEngine clock alone (of ram-addr8bit, or of --systems)")
    ap.add_argument("--read-early", action="store_true", help="read_early=True against the same engine without it, per system, K and flag set")
    ap.add_argument("--snapshot", action="store_true", help="state() + save() and load() + load_state() per system and K, beside the ms per clock")
    ap.add_argument("--cb-many", action="store_true", help="cb_many=True against the same engine without it, per system and K")
    ap.add_argument("--sets", type=int, nargs="+", default=None, help="--read-early: which of the six flag sets (0 .. 5), default all")
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
        for name in args.systems or ["ram-addr8bit"]:
            sysm = m.load_blueprint(os.path.join(gold, name + ".toml"), cmux_memories=True)
            v = [one(m, keys, sysm, bk2, pk, 1, args.clocks) for _ in range(args.pairs)]
            print(f"defaults  {head}; {name}, CmuxCipherEngine, ms per clock: {' '.join(f'{x:.2f}' for x in v)}   median {fmt(v)}", flush=True)
    elif args.read_early:
        read_early_leg(m, args, keys, bk2, pk, head, gold)
    elif args.snapshot:
        snapshot_leg(m, args, keys, bk2, pk, head, gold)
    elif args.cb_many:
        cb_many_leg(m, args, keys, bk2, pk, head, gold)
    else:
        print(f"\n{head}; {args.pairs} interleaved pairs (K = 1, then K lanes) per K, median (min .. max)", flush=True)
        for name in args.systems or ["ram-addr8bit", "cahp-ruby"]:
            sysm = m.load_blueprint(os.path.join(gold, name + ".toml"), cmux_memories=True)
            bits = [pt.addr_width for pt in sysm.ports]
            print(f"== {name}: {len(sysm.ports)} ports, address bits {bits}, {sysm.nl.rotations()} gate rotations per clock", flush=True)
            print("   K | K = 1 beside it, ms per clock | K lanes, ms per clock | clock | request-clocks / s", flush=True)
            for K in args.lanes or [2, 4, 8]:
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
