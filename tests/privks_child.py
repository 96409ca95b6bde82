"""Child process of tests/test_gpu_privks.py::test_off_the_fft_path: IYK_HIP_NTT=fp is read at init, which a fresh process has
whatever fixture of the parent holds the library.  iyk_hip_trgsw_from_rows answers the state error that names the missing spectra and
launches nothing; iyk_hip_privks_batch, integer only, gives the restatement's words.  Prints `ok refused` and exits 0, or raises."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import privks_ref as ref  # noqa: E402


def main():
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name("128"), seed=1)
    p = keys.params
    os.environ["IYK_HIP_NTT"] = "fp"
    hip.initialize(keys, device_ids=(0,))
    try:
        assert hip.ntt_path() == "fp50"
        st = hip.Stream(0)
        n_in, t, bb = 16, 10, 3
        key = hip.PrivKsKey(n_in, t, bb)
        rng = np.random.default_rng(5)
        K = rng.integers(0, 1 << 32, size=(key.rows, key.words), dtype=np.uint64).astype(np.uint32)
        tl = rng.integers(0, 1 << 64, size=(3, n_in + 1), dtype=np.uint64)
        store, trl, dummy = hip.Tlwe2(n_in, 3), hip.Trlwe(8), hip.Trlwe(64)   # dummy: larger than one selector slot
        try:
            key.upload(st, 0, K)
            store.upload(st, 0, tl)
            T = np.full((8, key.words), 0x5A5A5A5A, dtype=np.uint32)
            trl.upload(st, 0, T)
            filler = rng.integers(0, 1 << 32, size=(64, key.words), dtype=np.uint64).astype(np.uint32)
            dummy.upload(st, 0, filler)
            L = hip.lib()
            slot = np.zeros(1, dtype=np.int32)
            rows = np.arange(p.trgsw_rows, dtype=np.int32)
            rc = L.iyk_hip_trgsw_from_rows(st.h, dummy.ptr, 1, 1, slot.ctypes.data_as(hip._i32p), trl.ptr, trl.slots,
                                           rows.ctypes.data_as(hip._i32p))
            msg = L.iyk_hip_last_error().decode()
            assert rc == -2 and "iyk_hip_trgsw_from_rows" in msg and "needs the FFT key spectra" in msg, (rc, msg)
            st.sync()
            assert np.array_equal(dummy.download(st, 0, 64), filler) and np.array_equal(trl.download(st, 0, 8), T)
            jobs = [(0, 0, 7), (1, 1, 0), (2, 0, 3)]
            st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
            got = trl.download(st, 0, 8)
            assert np.array_equal(got, ref.run_jobs(T.copy(), tl, jobs, t, bb, ref.key_rows_of(K)))
        finally:
            key.free()
            store.free()
            trl.free()
            dummy.free()
            st.destroy()
    finally:
        hip.cleanup()
    print("ok refused")


if __name__ == "__main__":
    main()
