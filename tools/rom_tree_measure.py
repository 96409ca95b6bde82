#!/usr/bin/env python3
"""Kernel-only A/B behind profiles/rom_tree_ab.txt (128-bit set): the read tree of a CMUX memory as ONE cmux_tree_batch per four levels
against the same tree as one cmux_batch per level (the launches Ram.read_port / Rom.read send without fused_tree, whose kernel this
change leaves byte-identical): the 8-level trees of an 8 x 8 and an 8 x 16 RAM (addr_width 8; 8 and 16 bit planes: two tree launches
against eight), and the 2-level upper tree of the (12, 0) ROM at 1 and 64 simultaneous reads (one launch against two).  Selectors and
rows hold uniform words: the kernels' time does not depend on them.

The method of tools/rom_chain_measure.py: HIP events on the stream the library launches on; per shape three interleaved pairs (fused,
unfused, fused, ...), each side one warm-up and then REPS timed runs with a stream synchronisation between runs; a pair's figure is
the median.  Both sides have two figures: `sum`, the sum of the launches each between its own pair of events, and `span`, one pair of
events around the whole sequence (the launch gaps included).  No threshold is fixed in advance: per shape the report states whether
fused `sum` lies outside the spread (the larger max - min of the three medians of the two sides) of unfused `sum`, and on which side.

    python tools/rom_tree_measure.py > profiles/rom_tree_ab.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RAMS, ROMS, REPS, PAIRS = [(8, 8), (8, 16)], [((12, 0), 1), ((12, 0), 64)], 5, 3


def main():
    import torch

    from iyokan_amd import client, cmux, hip
    from iyokan_amd.params import params_128bit

    keys = client.keygen(params_128bit(), seed=1)
    hip.initialize(keys, device_ids=(0,))
    rng = np.random.default_rng(1)
    ts = torch.cuda.Stream(device=0)
    st = hip.Stream(0, ts.cuda_stream)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    N = int(keys.params.N)
    words = lambda *shape: rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)

    def timed(launches):
        """ms of every launch between its own events, and of the whole sequence"""
        marks = [ev() for _ in range(len(launches) + 1)]
        outer = (ev(), ev())
        outer[0].record(ts)
        for m, launch in zip(marks, launches):
            m.record(ts)
            launch()
        marks[-1].record(ts)
        outer[1].record(ts)
        st.sync()
        return sum(a.elapsed_time(b) for a, b in zip(marks, marks[1:])), outer[0].elapsed_time(outer[1])

    def shapes():
        for aw, dw in RAMS:
            ram = cmux.Ram(st, words(dw << aw, 2 * N), aw, dw)
            ram.trgsw.upload(st, 0, words(aw, ram.trgsw.words))
            yield f"RAM {aw} x {dw}", ram, ram.tree_launches(), ram.read_launches()
        for (aw, lw), reads in ROMS:
            rom = cmux.Rom(st, words(cmux.rom_layout(aw, lw, N).data_rows, 2 * N), aw, lw, max_reads=reads)
            rom.trgsw.upload(st, 0, words(reads * aw, rom.trgsw.words))
            trees = rom.tree_launches(reads)
            yield f"ROM ({aw}, {lw}) reads {reads}", rom, trees, rom.launches(reads)[: sum(t[1][0] for t in trees)]

    print(f"build {hip.build_id()}; 128-bit set; {torch.cuda.get_device_name(0)}; HIP events; {PAIRS} interleaved pairs, median of {REPS} after one warm-up each")
    try:
        for name, mem, trees, levels in shapes():
            fused = [(lambda a=a: st.cmux_tree_batch(mem.trgsw, mem.trlwe, *a)) for a in trees]
            unfused = [(lambda a=a: st.cmux_batch(mem.trgsw, mem.trlwe, *a)) for a in levels]
            med = {("fused", "sum"): [], ("fused", "span"): [], ("unfused", "sum"): [], ("unfused", "span"): []}
            for pair in range(PAIRS):
                for side, launches in (("fused", fused), ("unfused", unfused)):
                    timed(launches)
                    runs = [timed(launches) for _ in range(REPS)]
                    sums, spans = [r[0] for r in runs], [r[1] for r in runs]
                    print(f"{name} pair {pair} {side:8s} {len(launches):2d} launch(es): per-launch sum ms "
                          + " ".join(f"{x:.4f}" for x in sums) + " | span ms " + " ".join(f"{x:.4f}" for x in spans))
                    med[side, "sum"].append(float(np.median(sums)))
                    med[side, "span"].append(float(np.median(spans)))
            f, u, fs, us = (float(np.median(med[k])) for k in (("fused", "sum"), ("unfused", "sum"), ("fused", "span"), ("unfused", "span")))
            spread = max(max(med[k]) - min(med[k]) for k in (("fused", "sum"), ("unfused", "sum")))
            verdict = "inside the spread of unfused" if abs(f - u) <= spread else f"outside the spread of unfused: {'FASTER' if f < u else 'SLOWER'}"
            print(f"== {name}: {len(levels)} levels, {len(trees)} tree launch(es) of {[len(t[0]) for t in trees]} jobs; fused sum {f:.4f} ms, "
                  f"unfused sum {u:.4f} ms, fused / unfused = {f / u:.3f}; span {fs:.4f} against {us:.4f} ms ({fs / us:.3f}); "
                  f"larger spread of the pairs {spread:.4f} ms; fused is {verdict}")
            mem.free()
    finally:
        st.destroy()
        hip.cleanup()


if __name__ == "__main__":
    main()
