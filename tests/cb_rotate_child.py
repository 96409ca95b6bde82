"""Child process of tests/test_gpu_cb_rotate.py: iyk_hip_cleanup followed by iyk_hip_init with a lvl2 bootstrapping key still alive —
the byte count starts at 0 again and freeing the old key leaves it at 0, as for the private key-switching keys."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iyokan_amd import client, hip  # noqa: E402
from iyokan_amd.params import params_128bit  # noqa: E402

keys = client.keygen(params_128bit(), seed=1)
hip.initialize(keys, device_ids=(0,))
old = hip.Bk2Key(2)
per_key = (2 * 2 * 8 * 2 * 2048 + 2 * 2048) * 8
assert hip.bk2_key_bytes(0) == per_key
hip.cleanup()
hip.initialize(keys, device_ids=(0,))
assert hip.bk2_key_bytes(0) == 0
new = hip.Bk2Key(1)
assert hip.bk2_key_bytes(0) == (1 * 2 * 8 * 2 * 2048 + 2 * 2048) * 8
old.free()                                   # a key of the earlier initialisation: freed, the new count untouched
assert hip.bk2_key_bytes(0) == (1 * 2 * 8 * 2 * 2048 + 2 * 2048) * 8
new.free()
assert hip.bk2_key_bytes(0) == 0
hip.cleanup()
print("ok reinit")
