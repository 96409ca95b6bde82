"""GPU, 80-bit set: runner.CmuxLaneEngine with words_only=True, K = 2 — another l, another number of TRGSW rows and the K x widest sizing
of the lvl2 store and the TRLWE scratch.  One clock, word for word against one-lane CmuxCipherEngines; never a decryption (the
restatement of circuit bootstrapping itself misreads ROM bits at this set).  A module of its own beside
tests/test_gpu_cmux_lanes.py because the library is initialised with ONE key set per module."""
import numpy as np
import pytest

import cb_rotate_cases
import cmux_system_cases as small
import test_gpu_cmux_lanes as lanes128
from iyokan_amd import client
from iyokan_amd.system import load_blueprint

pytestmark = pytest.mark.gpu

N2 = cb_rotate_cases.N2


@pytest.fixture(scope="module")
def gpu80(keys80, tmp_path_factory):
    from iyokan_amd import hip

    hip.initialize(keys80, device_ids=(0,))
    st = hip.Stream(0)
    p = keys80.params
    bk = client.bk2_rows(keys80, client.keygen_lvl2(N2, seed=31), 4, 9, cb_rotate_cases.ALPHA2, seed=32)
    bk2 = hip.Bk2Key(p.n)
    for first in range(0, p.n, 200):
        bk2.upload(st, first, bk[first:first + 200])
    pk = hip.PrivKsKey(N2, 1, 1)
    pk.upload(st, 0, np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32))
    st.sync()
    sysm = load_blueprint(small.write_blueprint(str(tmp_path_factory.mktemp("cmux_lanes_80"))), cmux_memories=True)
    yield keys80, bk2, pk, sysm
    bk2.free()
    pk.free()
    st.destroy()
    hip.cleanup()


def test_the_80_bit_set_is_refused_without_the_flag(gpu80):
    keys, bk2, pk, sysm = gpu80
    with pytest.raises(ValueError, match="words_only=True"):
        lanes128._engine(keys, sysm, bk2, pk, [None, None], 2)


@pytest.mark.parametrize("flags", [dict(stage_cb=True, refresh_aside=True)], ids=["stage_cb+refresh_aside"])
def test_lane_engine_one_clock_words_only(gpu80, flags):
    from iyokan_amd import runner
    from iyokan_amd.packet import TFHEPacket

    keys, bk2, pk, sysm = gpu80
    reqs = [small.request(31, 1), small.request(32, 1)]
    packets = [TFHEPacket.encrypt(keys, r, seed=810 + i) for i, r in enumerate(reqs)]
    dummy = lambda rows: [0] * len(rows)
    want = []
    for r in range(2):
        eng, be, plan = lanes128._engine(keys, sysm, bk2, pk, [packets[r]], 1, decrypt_ram=dummy, words_only=True, **flags)
        try:
            runner.run_packet(sysm, reqs[r], engine=eng)
            want.append((be.read_many(list(range(plan.num_slots))), eng.ram_rows("ram")))
        finally:
            eng.free()
            be.close()
    eng, be, plan = lanes128._engine(keys, sysm, bk2, pk, packets, 2, decrypt_ram=dummy, words_only=True, **flags)
    try:
        p = keys.params
        assert eng.tlwe2.slots == 2 * eng._cb_bits() * int(p.l) and eng.scratch.slots == 2 * eng._cb_bits() * int(p.trgsw_rows)
        runner.run_packets(sysm, reqs, engine=eng)
        for r in range(2):
            assert np.array_equal(be.read_many(list(range(plan.num_slots)), lane=r), want[r][0]), r
            assert np.array_equal(eng.ram_rows("ram", lane=r), want[r][1]), r
    finally:
        eng.free()
        be.close()
    assert not np.array_equal(want[0][1], want[1][1])
