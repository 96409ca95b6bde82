"""Child process of tests/test_gpu_cmux_stage_cb.py::test_wait_stream_refuses_a_second_replica: two replicas aliased to device 0 need an
initialisation of their own, which a fresh process has whatever fixture of the parent holds the library.  A stream of replica 0 and one
of replica 1 are refused either way round by iyk_hip_stream_wait_stream, both stay usable, and two streams of replica 1 are accepted.
`python cmux_stage_child.py` prints `ok replica` and exits 0, or raises."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_by_name

    keys = client.keygen(params_by_name("128"), seed=1)
    p = keys.params
    rows = np.random.default_rng(51).integers(0, 1 << 32, size=(3, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    hip.initialize(keys, device_ids=(0, 0))
    try:
        assert hip.lib().iyk_hip_num_gpus() == 2
        s0, s1, s1b = hip.Stream(0), hip.Stream(1), hip.Stream(1)
        trl = hip.Trlwe(3, 1)
        try:
            trl.upload(s1, 0, rows)
            for a, b in ((s0, s1), (s1, s0)):
                try:
                    a.wait_stream(b)
                except hip.IykHipError as e:
                    assert "iyk_hip_stream_wait_stream failed (-1): " in str(e) and "different replicas" in str(e), e
                else:
                    raise AssertionError("a stream of another replica was not refused")
            s1.trlwe_add_batch(trl, [0], [1], [2], 0)
            s1b.wait_stream(s1)                                                     # two streams of replica 1
            got = trl.download(s1b, 0, 3)
            s0.sync()
        finally:
            trl.free()
            for s in (s0, s1, s1b):
                s.destroy()
    finally:
        hip.cleanup()
    assert np.array_equal(got[:2], rows[:2]) and np.array_equal(got[2], (rows[0] + rows[1]).astype(np.uint32))
    print("ok replica")


if __name__ == "__main__":
    main()
