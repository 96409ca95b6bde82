#!/usr/bin/env python3
"""A/B of the two forms of the lvl0 -> lvl2 rotation (cb_rotate_kernel: IYK_HIP_CB_KERNEL=wg, cb_rotate_lat_kernel: =lat) on one GPU.

Kernel-only time from the HIP events around the launch (Stream.last_batch_timing), median of 5 batches after one warm-up, uniform key
words, as profiles/cb_rotate_ab.txt was taken.  Per parameter set (n = 636, n = 500) and batch width (1, 8, 24, 86, 258 rotations) the
two forms run INTERLEAVED, three pairs; a form is called faster at a width when it won every pair by more than the larger spread
(max - min of a form's three medians).  Each parameter set is one child process under its own `timeout`; the first non-zero status
stops the run.  Output: profiles/cb_rotate_lat_ab.txt (or --out).

    python tools/cb_rotate_lat_measure.py [--out FILE] [--limit SECONDS]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTHS = (1, 8, 24, 86, 258)
PAIRS, REPS = 3, 5
KNOB = "IYK_HIP_CB_KERNEL"


def child(name):
    import numpy as np

    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name(name), seed=1)
    p = keys.params
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    key = hip.Bk2Key(p.n)
    rng = np.random.default_rng(7)
    for first in range(0, p.n, 64):
        c = min(64, p.n - first)
        key.upload(st, first, rng.integers(0, 1 << 64, size=(c, 8, 2, 2048), dtype=np.uint64))
    arena = hip.Arena(8)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1, 1, 0, 0, 1, 0], seed=2))
    store = hip.Tlwe2(2048, max(WIDTHS))
    st.sync()
    print(f"set {name} n {p.n}: kernel-only ms per batch (HIP events around the launch), median of {REPS} after one warm-up, {PAIRS} interleaved pairs")
    try:
        for width in WIDTHS:
            in_ = [g % 8 for g in range(width)]
            mu = [1 << (63 - (g % int(p.l) + 1) * int(p.Bgbit)) for g in range(width)]
            med = {"wg": [], "lat": []}
            for _ in range(PAIRS):
                for kind in ("wg", "lat"):
                    os.environ[KNOB] = kind
                    assert hip.cb_rotate_form(width) == (kind == "lat")
                    ms = []
                    for _ in range(REPS + 1):
                        st.cb_rotate_batch(key, arena, in_, [1] * width, [0] * width, mu, store, list(range(width)))
                        st.sync()
                        ms.append(st.last_batch_timing()[0])
                    med[kind].append(statistics.median(ms[1:]))
            spread = {k: max(v) - min(v) for k, v in med.items()}
            wins = all(w - l > max(spread.values()) for w, l in zip(med["wg"], med["lat"]))
            for kind in ("wg", "lat"):
                m = statistics.median(med[kind])
                print(f"set {name} n {p.n}: {width:3d} rotations {kind:3s}: ms per batch {['%.3f' % v for v in med[kind]]} median {m:.3f} "
                      f"us/step {1000 * m / p.n:.2f} spread {spread[kind]:.3f}")
            print(f"set {name} n {p.n}: {width:3d} rotations: lat faster in every pair by more than the larger spread: {'yes' if wins else 'no'}", flush=True)
    finally:
        os.environ.pop(KNOB, None)
        store.free()
        arena.free()
        key.free()
        st.destroy()
        hip.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cb_rotate_lat_ab.txt"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a parameter set's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    lines = ["# tools/cb_rotate_lat_measure.py: cb_rotate_kernel<4, 9> (wg) against cb_rotate_lat_kernel<4, 9> (lat), forced by IYK_HIP_CB_KERNEL,",
             "# one process per parameter set, one GPU, no profiler attached (the card is shared: other tenants not controlled)."]
    status = 0
    for name in ("128", "80"):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name],
                           capture_output=True, text=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            lines.append(f"# set {name}: the child ended with status {r.returncode}; stopped here")
            lines += ["# " + s for s in r.stderr.splitlines()[-12:]]
            status = r.returncode
            break
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return status


if __name__ == "__main__":
    sys.exit(main())
