"""Child process of tests/test_gpu_cmux_edges.py::test_second_replica and ::test_refused_without_fft_spectra: both need an
initialisation of their own (two replicas; IYK_HIP_NTT=fp, read at init), which a fresh process has whatever fixture of the parent
holds the library.  `python cmux_edges_child.py replica|refused` prints `ok <mode>` and exits 0, or raises."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cmux_cases  # noqa: E402
import cmux_ref  # noqa: E402
import ram_ref  # noqa: E402


def _rows(p, seed, count):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(count, 2 * p.N), dtype=np.uint64).astype(np.uint32)


def second_replica(keys128, oracle128):
    """Two replicas aliased to device 0 (as test_gpu_zz_debug.py does); the stores and the stream of replica 1 — its own copy of the
    transform constants — run one cmux_batch, one chain batch and one index extraction."""
    from iyokan_amd import hip

    keys, p = keys128, keys128.params
    sub = cmux_cases.selectors(keys)[cmux_cases.UNIFORM - 4 : cmux_cases.UNIFORM + 4]   # four worst-case words, four uniform
    T = _rows(p, 36, 10)
    jobs = [(5, 0, 1, 0, 6), (2, 2, -1, 1500, 2), (7, 3, 4, 0, 4)]
    chains = [(0, 8, 0xA5, 6, 5, 7), (3, 5, 0b10110, 0, 1, 8)]
    hip.initialize(keys, device_ids=(0, 0))
    try:
        assert hip.lib().iyk_hip_num_gpus() == 2
        st = hip.Stream(1)
        sel, trl, arena = hip.Trgsw(len(sub), 1), hip.Trlwe(T.shape[0], 1), hip.Arena(2, 1)
        try:
            sel.upload(st, 0, sub)
            trl.upload(st, 0, T)
            st.cmux_batch(sel, trl, *zip(*jobs))
            st.cmux_chain_batch(sel, trl, *zip(*chains))
            st.sample_extract_index_keyswitch_batch(trl, [7, 2], [p.N - 1, 3], [0, 1], arena)
            st.sync()
            got, got_tlwe = trl.download(st, 0, T.shape[0]), st.download(arena, 0, 2)
        finally:
            sel.free()
            trl.free()
            arena.free()
            st.destroy()
    finally:
        hip.cleanup()
    want = ram_ref.run_chains(p, cmux_ref.run_jobs(p, T.copy(), sub, jobs), sub, chains)
    assert np.array_equal(got, want)
    for g, (row, h) in enumerate(((7, p.N - 1), (2, 3))):
        assert np.array_equal(got_tlwe[g], oracle128.keyswitch(cmux_ref.sample_extract_index(want[row], h, p.N))), (row, h)


def refused_without_fft_spectra(keys128, oracle128):
    """IYK_HIP_NTT=fp at init: the selector store and both CMUX entry points answer the state error that names the missing spectra and
    launch nothing; the row add and the index extraction, which need no spectra, still work.  The dummy selector store handed to the
    direct calls is a TRLWE buffer larger than one selector slot."""
    from iyokan_amd import hip

    keys, p = keys128, keys128.params
    old = os.environ.get("IYK_HIP_NTT")
    os.environ["IYK_HIP_NTT"] = "fp"
    try:
        hip.initialize(keys, device_ids=(0,))
    finally:
        if old is None:
            os.environ.pop("IYK_HIP_NTT", None)
        else:
            os.environ["IYK_HIP_NTT"] = old
    try:
        assert hip.ntt_path() == "fp50"
        try:
            hip.Trgsw(1)
        except hip.IykHipError as e:
            assert "iyk_hip_trgsw_alloc failed (-2): " in str(e) and "needs the FFT key spectra" in str(e), e
        else:
            raise AssertionError("Trgsw(1) was not refused")
        st = hip.Stream(0)
        T = _rows(p, 37, 4)
        trl, dummy, arena = hip.Trlwe(4), hip.Trlwe(64), hip.Arena(1)
        try:
            filler = _rows(p, 38, 64)
            trl.upload(st, 0, T)
            dummy.upload(st, 0, filler)
            L = hip.lib()
            zero = np.zeros(4, dtype=np.int32)
            one = np.ones(1, dtype=np.int32)
            two = np.full(1, 2, dtype=np.int32)
            ip = lambda a: a.ctypes.data_as(hip._i32p)
            up = lambda a: a.view(np.uint32).ctypes.data_as(hip._u32p)
            host = np.zeros(p.trgsw_rows * (p.k + 1) * p.N, dtype=np.uint32)   # one torus-domain TRGSW
            calls = {
                "iyk_hip_trgsw_upload": lambda: L.iyk_hip_trgsw_upload(st.h, dummy.ptr, 1, 0, 1, up(host)),
                "iyk_hip_cmux_batch": lambda: L.iyk_hip_cmux_batch(st.h, dummy.ptr, 1, trl.ptr, trl.slots, 1, ip(zero), ip(zero), ip(one),
                                                                   ip(zero), ip(two)),
                "iyk_hip_cmux_chain_batch": lambda: L.iyk_hip_cmux_chain_batch(st.h, dummy.ptr, 1, trl.ptr, trl.slots, 1, ip(zero), ip(one),
                                                                               up(zero), ip(zero), ip(one), ip(two)),
            }
            for name, call in calls.items():
                assert call() == -2, name
                msg = L.iyk_hip_last_error().decode()
                assert name in msg and "needs the FFT key spectra" in msg, msg
            st.sync()
            assert np.array_equal(trl.download(st, 0, 4), T) and np.array_equal(dummy.download(st, 0, 64), filler)   # nothing was launched
            st.trlwe_add_batch(trl, [0], [1], [3], int(p.mu))
            st.sample_extract_index_keyswitch_batch(trl, [3], [p.N // 2], [0], arena)
            st.sync()
            row = (T[0] + T[1]).astype(np.uint32)
            row[p.N] = (int(row[p.N]) + int(p.mu)) & 0xFFFFFFFF
            assert np.array_equal(trl.download(st, 3, 1)[0], row)
            assert np.array_equal(st.download(arena, 0, 1)[0], oracle128.keyswitch(cmux_ref.sample_extract_index(row, p.N // 2, p.N)))
        finally:
            trl.free()
            dummy.free()
            arena.free()
            st.destroy()
    finally:
        hip.cleanup()


def main(mode):
    import oracle_lib
    from iyokan_amd import client
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name("128"), seed=1)
    orc = oracle_lib.Oracle(keys)
    try:
        {"replica": second_replica, "refused": refused_without_fft_spectra}[mode](keys, orc)
    finally:
        orc.close()
    print(f"ok {mode}")


if __name__ == "__main__":
    main(sys.argv[1])
