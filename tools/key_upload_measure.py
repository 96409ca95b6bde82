#!/usr/bin/env python3
"""A/B of the unseeded and the seeded upload of the two big evaluation keys on one GPU.

Keys: the full-size private key-switching key (n_in = 2048, t = 10, basebit = 3: 286 860 rows, 2.35 GB unseeded, half of it seeded) and
the lvl2 bootstrapping key at n = 636 (167 MB unseeded), integer form.  Both are real keys from the client library, made in windows by
at most client.MAX_THREADS threads; the time to make them is reported beside the upload times and is no part of them.

An upload is timed from the first enqueue to the stream idle: the host copy into the page-locked ring, the transfer, for a seeded
window key_mask_expand_kernel, for the lvl2 key the transform.  Per key one untimed upload of each kind, then three INTERLEAVED pairs
unseeded / seeded into the same key object.  The seeded upload is called not slower when its slowest run is under the unseeded upload's
slowest run plus the larger spread (max - min) of the two.  Output: profiles/key_seeded_ab.txt (or --out).

    python tools/key_upload_measure.py [--out FILE] [--rows N]      (--rows: a smaller private key, for a dry run)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = 3
N_IN, T, BB = 2048, 10, 3
WINDOW = 8192   # rows made per client call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_seeded_ab.txt"))
    ap.add_argument("--rows", type=int, default=None)
    a = ap.parse_args()

    import numpy as np

    from iyokan_amd import client, hip
    from iyokan_amd.params import params_128bit

    keys = client.keygen(params_128bit(), seed=1)
    p = keys.params
    s2 = client.keygen_lvl2(N_IN, seed=2)
    mask_seed = client.new_mask_seed()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    try:
        say(f"build {hip.build_id()}  PAIRS {PAIRS}")

        def timed(fn):
            st.sync()
            t0 = time.perf_counter()
            fn()
            st.sync()
            return (time.perf_counter() - t0) * 1e3

        def pairs(name, plain, seeded, plain_bytes, seeded_bytes):
            plain()
            seeded()   # untimed: the staging ring grows here
            tp, ts = [], []
            for _ in range(PAIRS):
                tp.append(timed(plain))
                ts.append(timed(seeded))
            spread = max(max(tp) - min(tp), max(ts) - min(ts))
            verdict = "not slower" if max(ts) <= max(tp) + spread else "SLOWER"
            say(f"{name}: unseeded ms {' '.join(f'{v:.1f}' for v in tp)}   seeded ms {' '.join(f'{v:.1f}' for v in ts)}   spread {spread:.1f}")
            say(f"{name}: unseeded {plain_bytes / min(tp) / 1e6:.2f} GB/s of host bytes, seeded {seeded_bytes / min(ts) / 1e6:.2f} GB/s of host bytes "
                f"= {plain_bytes / min(ts) / 1e6:.2f} GB/s of key bytes written; seeded is {verdict}")

        # ---- private key-switching key
        total = client.privks_key_total_rows(p, N_IN, T, BB) if a.rows is None else a.rows
        K = np.empty((total, 2 * p.N), dtype=np.uint32)
        B = np.empty((total, p.N), dtype=np.uint32)
        t0 = time.perf_counter()
        for f in range(0, total, WINDOW):
            K[f:f + WINDOW] = client.privks_key_rows(keys, s2, T, BB, f, min(WINDOW, total - f), seed=3)
        t1 = time.perf_counter()
        for f in range(0, total, WINDOW):
            B[f:f + WINDOW] = client.privks_key_rows(keys, s2, T, BB, f, min(WINDOW, total - f), seed=3, mask_seed=mask_seed)
        t2 = time.perf_counter()
        say(f"privks key: {total} rows, host bytes unseeded {K.nbytes} seeded {B.nbytes}; made in {t1 - t0:.1f} s / {t2 - t1:.1f} s (not timed below)")
        if a.rows is None:
            key = hip.PrivKsKey(N_IN, T, BB)
        else:   # a dry run: the smallest key that holds the rows
            key = hip.PrivKsKey(max(1, -(-total // (2 * T * ((1 << BB) - 1))) - 1), T, BB)
        try:
            assert key.rows >= total
            pairs("privks key", lambda: key.upload(st, 0, K), lambda: key.upload_seeded(st, mask_seed, 0, B), K.nbytes, B.nbytes)
        finally:
            key.free()
        del K, B

        # ---- lvl2 bootstrapping key
        t0 = time.perf_counter()
        K2 = client.bk2_rows(keys, s2, 4, 9, 2.0 ** -44, seed=4)
        t1 = time.perf_counter()
        B2 = client.bk2_rows(keys, s2, 4, 9, 2.0 ** -44, seed=4, mask_seed=mask_seed)
        t2 = time.perf_counter()
        say(f"bk2 key: n = {p.n}, host bytes unseeded {K2.nbytes} seeded {B2.nbytes}; made in {t1 - t0:.1f} s / {t2 - t1:.1f} s (not timed below)")
        bk = hip.Bk2Key(p.n)
        try:
            pairs("bk2 key", lambda: bk.upload(st, 0, K2), lambda: bk.upload_seeded(st, mask_seed, 0, B2), K2.nbytes, B2.nbytes)
        finally:
            bk.free()
    finally:
        st.destroy()
        hip.cleanup()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
