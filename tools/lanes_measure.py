#!/usr/bin/env python3
"""What K lanes cost and gain: ms per clock and request-clocks per second of one CAHP core (tests/golden/reftest: cahp-ruby-mux.toml, the
lowered form — every rom / ram a MUX tree of gates) with K = 1, 2, 4, 8 request packets in one widened clock (HipBackend(lanes=K):
every level ONE iyk_hip_gate_batch_lanes of count x K gates).

    python tools/lanes_measure.py [--lanes 1,2,4,8] [--pairs 5] [--parent-lib PATH] [--out profiles/lanes_ab.txt]

Part 1, in one process: for every K > 1, `pairs` times a clock of the K = 1 executor, then a clock of the K-lane executor, alternating —
a clock is run() + tick(), timed on the host around a stream synchronise.  Medians with min .. max.
Part 2, only with --parent-lib (a libiyokan_hip.so built from the parent commit): K = 1 clocks of this library and of the parent's,
each in a fresh process (a process loads one library), alternating, `pairs` times: the default path must not move.
Times are data independent, so the arenas hold trivial ciphertexts.  Needs a GPU; every raw line goes to --out as well."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLUEPRINT = os.path.join(ROOT, "tests", "golden", "reftest", "config-toml", "cahp-ruby-mux.toml")


def executors(lane_counts, lib_path=None):
    import numpy as np
    import torch

    from iyokan_amd import client, hip
    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend
    from iyokan_amd.params import params_128bit
    from iyokan_amd.system import load_blueprint

    if lib_path:
        hip.LIB_PATH = os.path.abspath(lib_path)
    assert torch.cuda.is_available(), "lanes_measure.py needs a GPU"
    keys = client.keygen(params_128bit(), seed=1)
    hip.initialize(keys, device_ids=(0,))
    sysm = load_blueprint(BLUEPRINT)
    plan = FrontierPlan(sysm.nl, 1)
    zero = client.trivial(keys.params, 0)
    exs = {}
    for k in lane_counts:
        be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0), lanes=k)
        for lane in range(k):
            be.write_many(list(range(plan.num_slots)), np.tile(zero, (plan.num_slots, 1)), **({"lane": lane} if lane else {}))
        exs[k] = FrontierExecutor(plan, be)
    info = {"gates_per_clock": int(sum(len(L["ew_desc"][0]) + len(L["rank_desc"][0][0]) for L in plan.levels)), "rotations_per_clock": int(plan.nl.rotations()),
            "levels": len(plan.levels), "slots": int(plan.num_slots), "build_id": hip.build_id()}
    return hip, exs, info


def clock_ms(ex):
    ex.sync()
    t0 = time.perf_counter()
    ex.run()
    ex.tick()
    ex.sync()
    return (time.perf_counter() - t0) * 1e3


def spread(xs):
    return f"{statistics.median(xs):.2f} ({min(xs):.2f} .. {max(xs):.2f})"


def write_out(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def worker(args):
    """K = 1 clocks of the library at --lib, one JSON line"""
    hip, exs, info = executors([1], args.lib)
    for _ in range(args.warmup):
        clock_ms(exs[1])
    ms = [clock_ms(exs[1]) for _ in range(args.clocks)]
    print(json.dumps({"lib": args.lib, "build_id": info["build_id"], "ms": ms}), flush=True)
    exs[1].be.close()
    hip.cleanup()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lanes", default="1,2,4,8")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--clocks", type=int, default=5, help="clocks per process in part 2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanes_ab.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.pairs < 3:
        ap.error("at least three pairs")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    counts = sorted({int(k) for k in args.lanes.split(",")} | {1})
    hip, exs, info = executors(counts)
    say(f"# lanes_measure: cahp-ruby-mux, 128-bit set, {json.dumps(info)}")
    say(f"# part 1: {args.pairs} interleaved pairs per K, one process; ms per clock, median (min .. max)")
    for ex in exs.values():
        for _ in range(args.warmup):
            clock_ms(ex)
    for k in counts:
        if k == 1:
            continue
        one, many = [], []
        for i in range(args.pairs):
            one.append(clock_ms(exs[1]))
            many.append(clock_ms(exs[k]))
            say(f"pair K={k} #{i}: K=1 {one[-1]:.2f} ms   K={k} {many[-1]:.2f} ms")
        m1, mk = statistics.median(one), statistics.median(many)
        say(f"K={k}: K=1 {spread(one)} ms   K={k} {spread(many)} ms   clock x{mk / m1:.2f}   request-clocks/s {1e3 / m1:.2f} -> {k * 1e3 / mk:.2f}"
            f" (x{k * m1 / mk:.2f})")
    for ex in exs.values():
        ex.be.close()
    hip.cleanup()
    if args.parent_lib:
        say(f"# part 2: K = 1, this library against {args.parent_lib}, {args.pairs} alternating pairs of fresh processes, {args.clocks} clocks each")
        this_lib = os.path.join(ROOT, "iyokan_amd", "lib", "libiyokan_hip.so")
        got = {"this": [], "parent": []}
        for i in range(args.pairs):
            for name, lib in (("this", this_lib), ("parent", args.parent_lib)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--clocks", str(args.clocks), "--warmup",
                                      str(args.warmup)], capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    say(f"worker {name} #{i} failed ({out.returncode}): {out.stderr[-400:]}")
                    write_out(args.out, lines)
                    return 1
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                got[name].append(statistics.median(rec["ms"]))
                say(f"pair #{i} {name} ({rec['build_id']}): median of {len(rec['ms'])} clocks {got[name][-1]:.2f} ms   all {[round(x, 2) for x in rec['ms']]}")
        a, b = statistics.median(got["this"]), statistics.median(got["parent"])
        say(f"K=1: this {spread(got['this'])} ms   parent {spread(got['parent'])} ms   this / parent {a / b:.4f}")
    write_out(args.out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
