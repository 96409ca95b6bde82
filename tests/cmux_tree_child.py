"""Child process of tests/test_gpu_cmux_tree.py for the two runs that need an initialisation of their own, which a fresh process has
whatever fixture of the parent holds the library:
    python cmux_tree_child.py 80bit   levels 1 .. 4 side by side and the nine jobs that share their leaves, at the 80-bit set
    python cmux_tree_child.py debug   IYK_HIP_DEBUG=1 (read at init): the nine jobs and the worst-case words at the 128-bit set, then
                                      iyk_hip_fft_round_error
Both compare word for word with the reference of tests/cmux_tree_cases.py.  Prints `round_error <value> <build id>` (debug) and
`ok <mode>`, or raises."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(which, names, debug):
    import cmux_tree_cases as cases
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name(which), seed=1)
    built = [{**cases.CPU_CASES, **cases.GPU_CASES}[n](keys) for n in names]
    got = []
    hip.initialize(keys, device_ids=(0,))
    try:
        st = hip.Stream(0)
        sel = hip.Trgsw(cases.SLOTS)
        sel.upload(st, 0, cases.selectors(keys))
        try:
            for _, T, batches in built:
                trl = hip.Trlwe(T.shape[0])
                try:
                    trl.upload(st, 0, T)
                    for jobs in batches:
                        st.cmux_tree_batch(sel, trl, *zip(*jobs))
                    st.sync()
                    got.append(trl.download(st, 0, T.shape[0]))
                finally:
                    trl.free()
            err, bid = hip.fft_round_error(0), hip.build_id()
        finally:
            sel.free()
            st.destroy()
    finally:
        hip.cleanup()
    for name, (trgsw, T, batches), rows in zip(names, built, got):
        assert np.array_equal(rows, cases.expected(keys.params, T, trgsw, batches)), f"{name} at the {which}-bit set differs from the reference"
    if debug:
        print(f"round_error {err:.6e} {bid}")


def main(mode):
    if mode == "debug":
        assert os.environ.get("IYK_HIP_DEBUG") == "1"
        run("128", ["nine", "alt"], True)
    else:
        assert mode == "80bit" and os.environ.get("IYK_HIP_DEBUG") != "1"
        run("80", ["side_by_side", "nine"], False)
    print(f"ok {mode}")


if __name__ == "__main__":
    main(sys.argv[1])
