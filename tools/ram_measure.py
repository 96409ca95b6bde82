#!/usr/bin/env python3
"""Workloads and report of profiles/ram_ab.txt (128-bit set).

chain:  cmux_chain_kernel against the same work as `steps` cmux_batch launches, at 2048 jobs x 8 steps (every cell of an addr_width 8,
        data_width 8 RAM) and 128 jobs x 4 steps; selectors shared by all jobs, every job in place on its own cell, one written row
        per 2^steps cells — the shape of Ram.clock.  Per shape 1 + REPS fused launches, then 1 + REPS unfused sequences.
clock:  1 + CLOCKS clocks of cmux.Ram at addr_width 8, data_width 8, fused; the report lists the kernels of the last one.

  rocprofv3 --kernel-trace --stats -d DIR -o ram -- python tools/ram_measure.py run-chain SIDE.json   (no counters in the same run)
  rocprofv3 --kernel-trace --stats -d DIR2 -o ram -- python tools/ram_measure.py run-clock SIDE2.json
  python tools/ram_measure.py report-chain DIR/<...>_results.db SIDE.json
  python tools/ram_measure.py report-clock DIR2/<...>_results.db SIDE2.json"""
import json
import os
import re
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES, REPS = [(2048, 8), (128, 4)], 5
ADDR_WIDTH, DATA_WIDTH, CLOCKS = 8, 8, 2


def _init():
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_128bit

    keys = client.keygen(params_128bit(), seed=1)
    hip.initialize(keys, device_ids=(0,))
    return client, hip, keys


def run_chain(side_path):
    from iyokan_amd import cmux

    client, hip, keys = _init()
    rng = np.random.default_rng(1)
    try:
        st = hip.Stream(0)
        for jobs_n, steps in SHAPES:
            cells, planes = 1 << steps, jobs_n >> steps
            sel, trl = hip.Trgsw(steps), hip.Trlwe(2 * jobs_n + planes)   # cells, accumulators of the unfused form, written rows
            sel.upload(st, 0, rng.integers(0, 1 << 32, size=(steps, sel.words), dtype=np.uint64).astype(np.uint32))
            rows = rng.integers(0, 1 << 32, size=(min(256, trl.slots), trl.words), dtype=np.uint64).astype(np.uint32)
            for first in range(0, trl.slots, rows.shape[0]):   # arbitrary words: the kernels' time does not depend on them
                trl.upload(st, first, rows[: trl.slots - first])
            jobs = [j for d in range(planes) for j in cmux.ram_write_jobs(steps, 2 * jobs_n + d, d * cells)]
            unfused = [cmux.chain_steps(j, jobs_n + g) for g, j in enumerate(jobs)]
            for _ in range(1 + REPS):
                st.cmux_chain_batch(sel, trl, *zip(*jobs))
                st.sync()
            for _ in range(1 + REPS):
                for s in range(steps):
                    st.cmux_batch(sel, trl, *zip(*(c[s] for c in unfused)))
                st.sync()
            sel.free()
            trl.free()
        with open(side_path, "w") as f:
            json.dump({"build_id": hip.build_id(), "shapes": SHAPES, "reps": REPS}, f)
        st.destroy()
    finally:
        hip.cleanup()


def run_clock(side_path):
    from iyokan_amd import cmux

    client, hip, keys = _init()
    p = keys.params
    rng = np.random.default_rng(2)
    try:
        st = hip.Stream(0)
        C = 1 << ADDR_WIDTH
        cells = client.encrypt_ram_trlwe(keys, rng.integers(0, 2, size=DATA_WIDTH * C), seed=3)
        ram = cmux.Ram(st, cells, ADDR_WIDTH, DATA_WIDTH)
        arena = hip.Arena(1 + 2 * DATA_WIDTH)
        st.upload(arena, 0, client.encrypt_bits(keys, [1] + [1, 0] * (DATA_WIDTH // 2) + [0] * DATA_WIDTH, seed=4))
        addr = 0b10010110
        trgsw = client.encrypt_trgsw(keys, [(addr >> k) & 1 for k in range(ADDR_WIDTH)], seed=5)
        for _ in range(1 + CLOCKS):
            ram.clock(trgsw, arena, 0, np.arange(1, 1 + DATA_WIDTH), np.arange(1 + DATA_WIDTH, 1 + 2 * DATA_WIDTH))
            st.sync()
        word = client.decrypt_ram_trlwe(keys, ram.cells()[:, addr])
        assert list(word) == [1, 0] * (DATA_WIDTH // 2), word   # the run computed a RAM write
        with open(side_path, "w") as f:
            json.dump({"build_id": hip.build_id(), "addr_width": ADDR_WIDTH, "data_width": DATA_WIDTH, "clocks": CLOCKS}, f)
        arena.free()
        ram.free()
        st.destroy()
    finally:
        hip.cleanup()


def _kernels(db_path):
    cur = sqlite3.connect(db_path).cursor()
    cols = [d[0] for d in cur.execute("select * from kernels limit 1").description]
    pick = lambda *c: next(x for x in c if x in cols)
    rows = cur.execute(f"select {pick('name', 'kernel_name')}, {pick('start', 'start_timestamp')}, {pick('end', 'end_timestamp')} "
                       "from kernels order by 2").fetchall()
    return [(n, (e - s) / 1e6) for n, s, e in rows]


def report_chain(db_path, side_path):
    side = json.load(open(side_path))
    k = [(n, d) for n, d in _kernels(db_path) if "cmux_chain_kernel" in n or "cmux_fft_kernel" in n]
    print(f"build id {side['build_id']}; 128-bit set; rocprofv3 --kernel-trace --stats, no counters in the run; selectors shared by all jobs, "
          "every job in place on its own cell (the write-back of Ram.clock)")
    at = 0
    for jobs_n, steps in side["shapes"]:
        reps = side["reps"]
        fused = k[at:at + 1 + reps]
        at += 1 + reps
        un = k[at:at + (1 + reps) * steps]
        at += (1 + reps) * steps
        assert all("cmux_chain_kernel" in n for n, _ in fused) and all("cmux_fft_kernel" in n for n, _ in un), (jobs_n, steps)
        f = [d for _, d in fused[1:]]
        u = [sum(d for _, d in un[r * steps:(r + 1) * steps]) for r in range(1, 1 + reps)]
        print(f"{jobs_n} jobs x {steps} steps: cmux_chain_kernel median {np.median(f):.4f} ms (min {min(f):.4f}, max {max(f):.4f}); "
              f"{steps} cmux_fft_kernel launches, summed kernel time, median {np.median(u):.4f} ms (min {min(u):.4f}, max {max(u):.4f}); "
              f"{reps} runs each after one warm-up; fused / unfused = {np.median(f) / np.median(u):.3f}")
    assert at == len(k), (at, len(k))
    print("(kernel durations only: the unfused form also pays steps - 1 further launch gaps on the stream, which a kernel trace does not show)")


def report_clock(db_path, side_path):
    side = json.load(open(side_path))
    k = _kernels(db_path)
    chains = [i for i, (n, _) in enumerate(k) if "cmux_chain_kernel" in n]
    assert len(chains) == 1 + side["clocks"], len(chains)
    # one period of the stream, from the last-but-one write-back chain to the last: the tail of one clock (chain, extraction + key switch,
    # refresh) and the head of the next (selector transform, read tree, extraction + key switch, MUXwoSE) — every kernel of a clock once
    period = k[chains[-2]:chains[-1]]
    short = lambda n: re.sub(r"\(.*", "", re.sub(r"^void ", "", re.sub(r"<.*", "", n.replace("iyk::", ""))))
    order, agg = [], {}
    for n, d in period:
        s = short(n)
        if s not in agg:
            order.append(s)
            agg[s] = [0, 0.0]
        agg[s][0] += 1
        agg[s][1] += d
    total = sum(d for _, d in period)
    print(f"build id {side['build_id']}; 128-bit set; one Ram.clock at addr_width {side['addr_width']}, data_width {side['data_width']}, fused "
          f"({(1 << side['addr_width']) * side['data_width']} cells); kernel trace, the kernels of one clock in stream order")
    for s in order:
        print(f"  {s:40s} {agg[s][0]:3d} launch(es) {agg[s][1]:9.4f} ms  {100 * agg[s][1] / total:5.1f} %")
    print(f"  {'all kernels of the clock':40s} {len(period):3d} launch(es) {total:9.4f} ms")


if __name__ == "__main__":
    if sys.argv[1] in ("run-chain", "run-clock"):
        (run_chain if sys.argv[1] == "run-chain" else run_clock)(sys.argv[2])
    else:
        (report_chain if sys.argv[1] == "report-chain" else report_clock)(sys.argv[2], sys.argv[3])
