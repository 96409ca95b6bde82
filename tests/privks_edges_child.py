"""Child process of tests/test_gpu_privks_edges.py::test_second_replica_and_reinitialisation: an initialisation with two replicas and a
re-initialisation, which a fresh process has whatever fixture of the parent holds the library.  Two replicas aliased to device 0 (as
tests/cmux_edges_child.py does): a private key-switch key on replica 1 is refused with a stream of replica 0 and gives the
restatement's words with a stream of replica 1; iyk_hip_privks_key_bytes counts per replica; after cleanup + initialize with the keys
still alive the counters are 0, and freeing an old key leaves them at 0 (the generation check of iyk_hip_privks_key_free).
Prints `ok replica reinit` and exits 0.  A failed check raises at once: nothing is tidied up on the way out, so no further call
reaches the GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import privks_edge_cases as cases  # noqa: E402
import privks_ref as ref  # noqa: E402


def _refused(hip, call, what):
    try:
        call()
    except hip.IykHipError as e:
        assert f"{what} failed (-1): " in str(e) and "the stream and the key are on different GPUs" in str(e), e
    else:
        raise AssertionError(f"{what} with a stream of the other replica was not refused")


def main():
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name("128"), seed=1)
    tl, K = cases.plan_store()
    n_in, t, bb = cases.PLAN_N_IN, cases.PLAN_T, cases.PLAN_BB
    hip.initialize(keys, device_ids=(0, 0))
    assert hip.lib().iyk_hip_num_gpus() == 2
    assert hip.privks_key_bytes(0) == 0 and hip.privks_key_bytes(1) == 0
    key1 = hip.PrivKsKey(n_in, t, bb, gpu_index=1)
    bytes1 = key1.rows * key1.words * 4
    assert (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (0, bytes1)
    key0 = hip.PrivKsKey(3, 5, 3)
    bytes0 = key0.rows * key0.words * 4
    assert bytes0 != bytes1 and (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (bytes0, bytes1)

    s0, s1 = hip.Stream(0), hip.Stream(1)
    store, trl = hip.Tlwe2(n_in, len(tl), 1), hip.Trlwe(8, 1)
    T = np.full((8, cases.WORDS), 0x5A5A5A5A, dtype=np.uint32)
    jobs = [(41, 0, 7), (3, 1, 0), (52, 0, 3), (17, 1, 4), (41, 1, 5)]
    args = ([j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
    store.upload(s1, 0, tl)
    trl.upload(s1, 0, T)
    _refused(hip, lambda: key1.upload(s0, 0, K), "iyk_hip_privks_key_upload")
    key1.upload(s1, 0, K)
    _refused(hip, lambda: s0.privks_batch(key1, store, *args), "iyk_hip_privks_batch")
    s0.sync()
    assert np.array_equal(trl.download(s1, 0, 8), T)          # nothing was launched
    s1.privks_batch(key1, store, *args)
    got = trl.download(s1, 0, 8)
    want = ref.run_jobs(T.copy(), tl, jobs, t, bb, ref.key_rows_of(K))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
    assert not np.all(want[7] == T[7]) and np.array_equal(want[1], T[1])

    store.free()
    trl.free()
    s0.destroy()
    s1.destroy()
    hip.cleanup()                                             # key0 and key1 are still alive
    hip.initialize(keys, device_ids=(0, 0))
    assert (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (0, 0)
    key1.free()                                               # a key of the earlier initialisation: its bytes are not in the new counters
    assert (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (0, 0), "freeing an old key took its bytes off the new counter"
    new0 = hip.PrivKsKey(3, 5, 3)
    assert (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (bytes0, 0)
    key0.free()
    assert (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (bytes0, 0)
    new0.free()
    assert (hip.privks_key_bytes(0), hip.privks_key_bytes(1)) == (0, 0)
    hip.cleanup()
    print("ok replica reinit")


if __name__ == "__main__":
    main()
