"""Child process of tests/test_gpu_ram.py::test_debug_round_error (IYK_HIP_DEBUG=1 is read at init): one batch of CMUX chains with
worst-case selector words and extreme digits, then iyk_hip_fft_round_error.  Prints `round_error <set> <value> <build id>`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(which):
    import cmux_ref
    import ram_ref
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    assert os.environ.get("IYK_HIP_DEBUG") == "1"
    p = params_by_name(which)
    keys = client.keygen(p, seed=1)
    rng = np.random.default_rng(3)
    trgsw = np.stack([cmux_ref.worst_case_trgsw(p, 0x7FFF7FFF)] * 5 + [cmux_ref.worst_case_trgsw(p, 0x80008000)] * 5)
    rows = list(cmux_ref.extreme_pair(p, rng, top=False)) + list(cmux_ref.extreme_pair(p, rng, top=True))
    T = np.stack(rows + [np.zeros(2 * p.N, dtype=np.uint32)] * 4)
    # (sel0, steps, pattern, src, mem, out): the first difference of every chain has extreme digits, in both orientations
    jobs = [(0, 5, 0b01010, 0, 1, 4), (5, 5, 0b10101, 1, 0, 5), (0, 2, 0, 2, 3, 6), (5, 1, 1, 3, 2, 7)]
    hip.initialize(keys, device_ids=(0,))
    try:
        st = hip.Stream(0)
        sel, trl = hip.Trgsw(10), hip.Trlwe(8)
        sel.upload(st, 0, trgsw)
        trl.upload(st, 0, T)
        st.cmux_chain_batch(sel, trl, *zip(*jobs))
        st.sync()
        got = trl.download(st, 0, 8)
        err = hip.fft_round_error(0)
        bid = hip.build_id()
        sel.free()
        trl.free()
        st.destroy()
    finally:
        hip.cleanup()
    assert np.array_equal(got, ram_ref.run_chains(p, T.copy(), trgsw, jobs)), "CHECK build of the chain kernel differs from the reference"
    print(f"round_error {which} {err:.6e} {bid}")


if __name__ == "__main__":
    main(sys.argv[1])
