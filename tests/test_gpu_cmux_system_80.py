"""GPU, 80-bit set: the engine of the CMUX memories refuses the set unless told that only words will be compared (the restatement of
circuit bootstrapping itself misreads ROM bits there); with the flag, one clock word for word — never a decryption."""
import numpy as np
import pytest

import cb_rotate_cases
import cmux_system_cases as cases
from iyokan_amd import client
from iyokan_amd.system import load_blueprint

pytestmark = pytest.mark.gpu

N2 = cb_rotate_cases.N2


@pytest.fixture(scope="module")
def gpu(keys80, oracle80, tmp_path_factory):
    from iyokan_amd import hip

    hip.initialize(keys80, device_ids=(0,))
    st = hip.Stream(0)
    p = keys80.params
    bk = client.bk2_rows(keys80, client.keygen_lvl2(N2, seed=31), 4, 9, cb_rotate_cases.ALPHA2, seed=32)
    bk2 = hip.Bk2Key(p.n)
    for first in range(0, p.n, 200):
        bk2.upload(st, first, bk[first:first + 200])
    pk = hip.PrivKsKey(N2, 1, 1)
    K = np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32)
    pk.upload(st, 0, K)
    st.sync()
    sysm = load_blueprint(cases.write_blueprint(str(tmp_path_factory.mktemp("cmux_system"))), cmux_memories=True)
    yield {"keys": keys80, "orc": oracle80, "bk": bk, "bk2": bk2, "K": K, "pk": pk, "sysm": sysm}
    bk2.free()
    pk.free()
    st.destroy()
    hip.cleanup()


def test_the_80_bit_set_is_refused_without_the_flag(gpu):
    with pytest.raises(ValueError, match="words_only=True"):
        cases.gpu_engine(gpu["keys"], gpu["sysm"], gpu["bk2"], gpu["pk"], None)


def test_one_clock_words_only(gpu):
    cases.one_clock_words(gpu["keys"], gpu["orc"], gpu["sysm"], gpu["bk"], gpu["K"], gpu["bk2"], gpu["pk"], words_only=True)
