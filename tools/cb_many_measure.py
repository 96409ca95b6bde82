#!/usr/bin/env python3
"""A/B of the many-digit form of the lvl0 -> lvl2 rotation (Stream.cb_rotate_many_batch: one rotation per address bit, l outputs) against
the per-digit form (Stream.cb_rotate_batch: l rotations per bit) on one GPU, for the same address bits.

Kernel-only time from the HIP events around the launch (Stream.last_batch_timing), median of 5 batches after one warm-up, uniform key
words, as profiles/cb_rotate_fft_ab.txt was taken.  Per parameter set (n = 636, l = 3; n = 500, l = 2), key form (the integer key under
its default kernel form; the FP64 key) and width (8 and 86 address bits: 86 x 3 = 258 per-digit rotations are two rounds on 256 CUs)
the two forms run INTERLEAVED, three pairs; a form is called faster when it won every pair by more than the larger spread (max - min of
a form's three medians).  Each parameter set is one child process under its own `timeout`; the first non-zero status stops the run.
Output: profiles/cb_many_ab.txt (or --out).

    python tools/cb_many_measure.py [--out FILE] [--limit SECONDS]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BITS = (8, 86)
PAIRS, REPS = 3, 5
KEY_FORMS = ("ntt", "fft")


def child(name):
    import numpy as np

    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name(name), seed=1)
    p = keys.params
    l, bg = int(p.l), int(p.Bgbit)
    os.environ.pop("IYK_HIP_CB_KERNEL", None)   # the integer key's default form
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    rng = np.random.default_rng(7)
    key = {form: hip.Bk2Key(p.n, form=form) for form in KEY_FORMS}
    for first in range(0, p.n, 64):
        w = rng.integers(0, 1 << 64, size=(min(64, p.n - first), 8, 2, 2048), dtype=np.uint64)
        for k in key.values():
            k.upload(st, first, w)
    arena = hip.Arena(8)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1, 1, 0, 0, 1, 0], seed=2))
    store = hip.Tlwe2(2048, max(BITS) * l)
    st.sync()
    mus = [1 << (63 - (r + 1) * bg) for r in range(l)]
    print(f"set {name} n {p.n} l {l}: kernel-only ms per batch (HIP events around the launch), median of {REPS} after one warm-up, "
          f"{PAIRS} interleaved pairs; kernel form of the integer key at these widths: {hip.cb_rotate_form(max(BITS))}")

    def run(which, form, bits):
        if which == "many":
            st.cb_rotate_many_batch(key[form], arena, [b % 8 for b in range(bits)], [1] * bits, [0] * bits, mus, store, [b * l for b in range(bits)])
        else:
            n = bits * l
            st.cb_rotate_batch(key[form], arena, [(g // l) % 8 for g in range(n)], [1] * n, [0] * n, [mus[g % l] for g in range(n)], store, list(range(n)))
        st.sync()
        return st.last_batch_timing()[0]

    try:
        for form in KEY_FORMS:
            for bits in BITS:
                med = {"per-digit": [], "many": []}
                for _ in range(PAIRS):
                    for which in med:
                        ms = [run(which, form, bits) for _ in range(REPS + 1)]
                        med[which].append(statistics.median(ms[1:]))
                spread = max(max(v) - min(v) for v in med.values())
                for which, v in med.items():
                    rot = bits * (l if which == "per-digit" else 1)
                    print(f"set {name} key {form} {bits:2d} bits {which:9s} ({rot:3d} rotations): ms per batch {['%.3f' % x for x in v]} "
                          f"median {statistics.median(v):.3f} (min {min(v):.3f} .. max {max(v):.3f})")
                faster = all(a - b > spread for a, b in zip(med["per-digit"], med["many"]))
                slower = all(b - a > spread for a, b in zip(med["per-digit"], med["many"]))
                ratio = statistics.median(med["many"]) / statistics.median(med["per-digit"])
                verdict = "many faster" if faster else "MANY SLOWER" if slower else "equal within the spread"
                print(f"set {name} key {form} {bits:2d} bits: many / per-digit {ratio:.2f}; in every pair by more than the larger spread "
                      f"({spread:.3f} ms): {verdict}", flush=True)
    finally:
        store.free()
        arena.free()
        for k in key.values():
            k.free()
        st.destroy()
        hip.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cb_many_ab.txt"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a parameter set's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    lines = ["# tools/cb_many_measure.py: Stream.cb_rotate_many_batch (one rotation per address bit) against Stream.cb_rotate_batch (l per bit),",
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
