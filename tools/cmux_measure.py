#!/usr/bin/env python3
"""Workload and report of profiles/cmux_ab.txt: cmux_fft_kernel at 2048 jobs (one level of a 4096-row tree) with one shared selector
and with 2048 distinct selectors, against the calibrated cost of one step of a full blind-rotation round on the same GPU.

  rocprofv3 --kernel-trace --stats -d DIR -o cmux -- python tools/cmux_measure.py run SIDE.json     (no counters in the same run)
  python tools/cmux_measure.py report DIR/<...>_results.db SIDE.json                                (reads the durations, prints the file)

SIDE.json carries the calibrated cost table and the build id from the run to the report.

`run` launches 1 + REPS shared-selector batches, then 1 + REPS distinct-selector batches; `report` takes them in that order."""
import json
import os
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JOBS, REPS = 2048, 5


def run(side_path):
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_128bit

    p = params_128bit()
    keys = client.keygen(p, seed=1)
    rng = np.random.default_rng(1)
    hip.initialize(keys, device_ids=(0,))
    try:
        cost = hip.calibrate(0)
        st = hip.Stream(0)
        sel, trl = hip.Trgsw(JOBS), hip.Trlwe(3 * JOBS)
        block = rng.integers(0, 1 << 32, size=(64, sel.words), dtype=np.uint64).astype(np.uint32)
        for first in range(0, JOBS, 64):   # arbitrary selector words: the kernel's time does not depend on them
            sel.upload(st, first, block)
        rows = rng.integers(0, 1 << 32, size=(256, trl.words), dtype=np.uint64).astype(np.uint32)
        for first in range(0, 2 * JOBS, 256):
            trl.upload(st, first, rows)
        g = np.arange(JOBS)
        zero = np.zeros(JOBS, dtype=np.int32)
        for s in (zero, g):
            for _ in range(1 + REPS):
                st.cmux_batch(sel, trl, s, 2 * g, 2 * g + 1, zero, 2 * JOBS + g)
                st.sync()
        with open(side_path, "w") as f:
            json.dump({"cost": cost, "n": int(p.n), "build_id": hip.build_id(), "jobs": JOBS, "reps": REPS}, f)
        sel.free()
        trl.free()
        st.destroy()
    finally:
        hip.cleanup()


def report(db_path, side_path):
    side = json.load(open(side_path))
    cur = sqlite3.connect(db_path).cursor()
    cols = [d[0] for d in cur.execute("select * from kernels limit 1").description]
    pick = lambda *c: next(x for x in c if x in cols)
    rows = cur.execute(f"select {pick('name', 'kernel_name')}, {pick('start', 'start_timestamp')}, {pick('end', 'end_timestamp')} "
                       "from kernels order by 2").fetchall()
    d = [(e - s) / 1e6 for n, s, e in rows if "cmux_fft_kernel" in n]
    assert len(d) == 2 * (1 + REPS), len(d)
    shared, distinct = d[1:1 + REPS], d[2 + REPS:]
    step = side["cost"]["round_ms"] / side["n"]
    print(f"build id {side['build_id']}; 128-bit set; {side['jobs']} jobs per launch; rocprofv3 --kernel-trace --stats, no counters in the run")
    for name, v in (("shared selector", shared), ("distinct selectors", distinct)):
        print(f"cmux_fft_kernel, {name}: median {np.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f}, {len(v)} launches after one warm-up)")
    print(f"blind-rotation step of a full round on the same GPU: iyk_hip_level_cost_table().round_ms / n = "
          f"{side['cost']['round_ms']:.3f} / {side['n']} = {step:.4f} ms (calibrated: {side['cost']['calibrated']}, round = {side['cost']['round']} rotations)")
    print(f"ratio shared / step = {np.median(shared) / step:.2f}; distinct / step = {np.median(distinct) / step:.2f}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        report(sys.argv[2], sys.argv[3])
