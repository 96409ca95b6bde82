#!/usr/bin/env python3
"""Kernel-only A/B behind profiles/rom_chain_ab.txt (128-bit set): the rotate tail of a ROM read as ONE cmux_rotate_chain_batch against the
same tail as one cmux_batch per step (the launches Rom.read(fused=False) sends, whose kernel this change leaves byte-identical), for the
(12, 0) and (8, 3) ROMs at 1, 8 and 64 simultaneous reads.  Selectors and rows hold uniform words: the kernels' time does not depend
on them.

Timed with HIP events on the stream the library launches on.  Per shape three interleaved pairs (fused, unfused, fused, ...), each side
one warm-up and then REPS timed runs with a stream synchronisation between runs; a pair's figure is the median.  The unfused side
has two figures: `sum`, the sum of its launches each between its own pair of events, and `span`, one pair of events around the whole
sequence (the launch gaps included).  The claim the report tests: fused is not slower than unfused `sum` by more than the larger
spread (max - min of the three medians) of the two sides.

    python tools/rom_chain_measure.py > profiles/rom_chain_ab.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES, READS, REPS, PAIRS = [(12, 0), (8, 3)], [1, 8, 64], 5, 3


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

    print(f"build {hip.build_id()}; 128-bit set; {torch.cuda.get_device_name(0)}; HIP events; {PAIRS} interleaved pairs, median of {REPS} after one warm-up each")
    verdicts = []
    try:
        for aw, lw in SHAPES:
            for reads in READS:
                data = rng.integers(0, 1 << 32, size=(cmux.rom_layout(aw, lw, keys.params.N).data_rows, 2 * keys.params.N), dtype=np.uint64)
                rom = cmux.Rom(st, data.astype(np.uint32), aw, lw, max_reads=reads)
                rom.trgsw.upload(st, 0, rng.integers(0, 1 << 32, size=(reads * aw, rom.trgsw.words), dtype=np.uint64).astype(np.uint32))
                upper, chain = rom.launches_fused(reads)
                tail = rom.launches(reads)[len(upper):]
                for args in upper:   # the rows the tail starts from
                    st.cmux_batch(rom.trgsw, rom.trlwe, *args)
                st.sync()
                fused = [lambda: st.cmux_rotate_chain_batch(rom.trgsw, rom.trlwe, *chain)]
                unfused = [(lambda a=a: st.cmux_batch(rom.trgsw, rom.trlwe, *a)) for a in tail]
                med = {"fused": [], "sum": [], "span": []}
                for pair in range(PAIRS):
                    for side, launches in (("fused", fused), ("unfused", unfused)):
                        timed(launches)
                        runs = [timed(launches) for _ in range(REPS)]
                        sums, spans = [r[0] for r in runs], [r[1] for r in runs]
                        print(f"({aw}, {lw}) reads {reads:3d} pair {pair} {side:8s} {len(launches):2d} launch(es): per-launch sum ms "
                              + " ".join(f"{x:.4f}" for x in sums) + " | span ms " + " ".join(f"{x:.4f}" for x in spans))
                        if side == "fused":
                            med["fused"].append(float(np.median(sums)))
                        else:
                            med["sum"].append(float(np.median(sums)))
                            med["span"].append(float(np.median(spans)))
                f, u, sp = (float(np.median(med[k])) for k in ("fused", "sum", "span"))
                spread = max(max(med[k]) - min(med[k]) for k in ("fused", "sum"))
                holds = f <= u + spread
                verdicts.append(holds)
                print(f"== ({aw}, {lw}) reads {reads:3d}: {len(tail)} steps; fused {f:.4f} ms, unfused sum {u:.4f} ms, span {sp:.4f} ms; "
                      f"fused / sum = {f / u:.3f}, fused / span = {f / sp:.3f}; larger spread of the pairs {spread:.4f} ms; "
                      f"not slower than the sum by more than the spread: {holds}")
                rom.free()
        print(f"claim 'the fused tail is not slower than the unfused one at any measured shape, by more than the larger spread of the pairs': "
              f"{'holds' if all(verdicts) else 'does NOT hold'} ({sum(verdicts)} of {len(verdicts)} shapes)")
    finally:
        st.destroy()
        hip.cleanup()


if __name__ == "__main__":
    main()
