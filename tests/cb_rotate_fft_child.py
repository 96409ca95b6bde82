"""Child process of tests/test_gpu_cb_rotate_fft.py, started with IYK_HIP_DEBUG=1 (read at iyk_hip_init): the `quarters-min` case under a
lvl2 key of the FP64 form, word for word, and then the largest |z - rint(z)| that cb_rotate_fft_kernel recorded
(iyk_hip_fft_round_error).  Nothing else with a rounded transform runs in this process, so the figure is the rotation's own."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import cb_rotate_fft_cases as cases  # noqa: E402
from iyokan_amd import client, hip  # noqa: E402
from iyokan_amd.params import params_128bit  # noqa: E402

assert os.environ.get("IYK_HIP_DEBUG") == "1"
keys = client.keygen(params_128bit(), seed=1)
hip.initialize(keys, device_ids=(0,))
st = hip.Stream(0)
bk, jobs = cases.case("quarters-min")
want = cases.expected("quarters-min")
key = hip.Bk2Key(bk.shape[0], form="fft")
key.upload(st, 0, bk)
tl = np.stack([j[0] for j in jobs])
arena = hip.Arena.from_torch(torch.from_numpy(np.ascontiguousarray(tl).view(np.int32)).to("cuda:0"))
store = hip.Tlwe2(cases.N2, len(jobs))
torch.cuda.synchronize()
assert hip.fft_round_error(0) == 0.0
st.cb_rotate_batch(key, arena, list(range(len(jobs))), [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], store, list(range(len(jobs))))
got = store.download(st, 0, len(jobs))
err = hip.fft_round_error(0)
store.free()
key.free()
st.destroy()
hip.cleanup()
assert np.array_equal(got, want), np.argwhere(got != want)[:8]
print(f"round error {err!r}")
