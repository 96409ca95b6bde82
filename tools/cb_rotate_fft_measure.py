#!/usr/bin/env python3
"""A/B of the two FORMS of the lvl2 bootstrapping key on one GPU: the FP64 key (hip.Bk2Key(form="fft"), cb_rotate_fft_kernel) against the
integer key under the latency form (form="ntt", IYK_HIP_CB_KERNEL=lat, cb_rotate_lat_kernel).

Kernel-only time from the HIP events around the launch (Stream.last_batch_timing), median of 5 batches after one warm-up, uniform key
words, as profiles/cb_rotate_lat_ab.txt was taken.  Per parameter set (n = 636, n = 500) and batch width (1, 8, 24, 86, 258 rotations) the
two keys run INTERLEAVED, three pairs; a key is called faster at a width when it won every pair by more than the larger spread
(max - min of a form's three medians).  Before the pairs: the time from the first upload call to the stream's idle (host copy into the
page-locked ring, transfer and transform of all n steps) for either form, three interleaved pairs after one untimed upload of each.  Each parameter set is one child process under its own
`timeout`; the first non-zero status stops the run.  Output: profiles/cb_rotate_fft_ab.txt (or --out).

    python tools/cb_rotate_fft_measure.py [--out FILE] [--limit SECONDS]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTHS = (1, 8, 24, 86, 258)
PAIRS, REPS = 3, 5
KNOB = "IYK_HIP_CB_KERNEL"
FORMS = ("ntt", "fft")


def child(name):
    import numpy as np

    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name(name), seed=1)
    p = keys.params
    os.environ[KNOB] = "lat"                    # the integer key's kernel; the FP64 key has one kernel whatever this says
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    rng = np.random.default_rng(7)
    windows = [rng.integers(0, 1 << 64, size=(min(64, p.n - first), 8, 2, 2048), dtype=np.uint64) for first in range(0, p.n, 64)]
    key = {form: hip.Bk2Key(p.n, form=form) for form in FORMS}
    print(f"set {name} n {p.n}: {hip.bk2_key_bytes(0) / 1e6:.1f} MB of lvl2 keys resident (both forms)")
    # a key may be uploaded again: pass 0 is the warm-up (it carries the first use of the stream's page-locked ring and of the transform
    # kernels, and sends the tables); passes 1 .. PAIRS are timed, the two forms interleaved
    ms = {form: [] for form in FORMS}
    for rep in range(PAIRS + 1):
        for form in FORMS:
            st.sync()
            t = time.perf_counter()
            for i, w in enumerate(windows):
                key[form].upload(st, 64 * i, w)
            st.sync()
            if rep:
                ms[form].append((time.perf_counter() - t) * 1e3)
    for form in FORMS:
        print(f"set {name} n {p.n}: key upload + transform of all steps to the stream's idle, form {form}: ms {['%.1f' % v for v in ms[form]]} "
              f"median {statistics.median(ms[form]):.1f} (after one untimed upload of either form, {PAIRS} interleaved pairs)")
    arena = hip.Arena(8)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1, 1, 0, 0, 1, 0], seed=2))
    store = hip.Tlwe2(2048, max(WIDTHS))
    st.sync()
    print(f"set {name} n {p.n}: kernel-only ms per batch (HIP events around the launch), median of {REPS} after one warm-up, {PAIRS} interleaved pairs")
    try:
        for width in WIDTHS:
            in_ = [g % 8 for g in range(width)]
            mu = [1 << (63 - (g % int(p.l) + 1) * int(p.Bgbit)) for g in range(width)]
            med = {form: [] for form in FORMS}
            for _ in range(PAIRS):
                for form in FORMS:
                    ms = []
                    for _ in range(REPS + 1):
                        st.cb_rotate_batch(key[form], arena, in_, [1] * width, [0] * width, mu, store, list(range(width)))
                        st.sync()
                        ms.append(st.last_batch_timing()[0])
                    med[form].append(statistics.median(ms[1:]))
            spread = {k: max(v) - min(v) for k, v in med.items()}
            wins = all(a - b > max(spread.values()) for a, b in zip(med["ntt"], med["fft"]))
            loses = all(b - a > max(spread.values()) for a, b in zip(med["ntt"], med["fft"]))
            for form in FORMS:
                m = statistics.median(med[form])
                print(f"set {name} n {p.n}: {width:3d} rotations {form:3s}: ms per batch {['%.3f' % v for v in med[form]]} median {m:.3f} "
                      f"us/step {1000 * m / p.n:.2f} spread {spread[form]:.3f}")
            verdict = "fft faster" if wins else "ntt (lat) faster" if loses else "neither"
            print(f"set {name} n {p.n}: {width:3d} rotations: in every pair by more than the larger spread: {verdict}", flush=True)
    finally:
        os.environ.pop(KNOB, None)
        store.free()
        arena.free()
        for k in key.values():
            k.free()
        st.destroy()
        hip.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cb_rotate_fft_ab.txt"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a parameter set's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    lines = ["# tools/cb_rotate_fft_measure.py: cb_rotate_fft_kernel<4, 9> (lvl2 key of form fft) against cb_rotate_lat_kernel<4, 9> (form ntt,",
             "# IYK_HIP_CB_KERNEL=lat), one process per parameter set, one GPU, no profiler attached (the card is shared: other tenants not controlled)."]
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
