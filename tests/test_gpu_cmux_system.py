"""GPU: a blueprint's rom / ram as CMUX memories behind circuit bootstrapping (runner.CmuxCipherEngine, iyk_hip_circuit_bootstrap_batch)
at the 128-bit set — one clock of the small system of tests/cmux_system_cases.py word for word against the composed restatement, and
the refusals of the one checked call."""
import numpy as np
import pytest

import cb_rotate_cases
import cmux_system_cases as cases
from iyokan_amd import client, cmux
from iyokan_amd.system import load_blueprint

pytestmark = pytest.mark.gpu

N2 = cb_rotate_cases.N2
FILL64, FILL32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0x5A5A5A5A)


@pytest.fixture(scope="module")
def gpu(keys128, oracle128, tmp_path_factory):
    """a real bk2 at n = 636 uploaded in windows, a uniform private key-switching key (n_in = 2048, t = 1, basebit = 1); two replicas
    on one GPU, so that a key of the other replica can be offered"""
    from iyokan_amd import hip

    hip.initialize(keys128, device_ids=(0, 0))
    st = hip.Stream(0)
    p = keys128.params
    bk = client.bk2_rows(keys128, client.keygen_lvl2(N2, seed=31), 4, 9, cb_rotate_cases.ALPHA2, seed=32)
    bk2 = hip.Bk2Key(p.n)
    for first in range(0, p.n, 200):
        bk2.upload(st, first, bk[first:first + 200])
    pk = hip.PrivKsKey(N2, 1, 1)
    K = np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32)
    pk.upload(st, 0, K)
    st.sync()
    path = cases.write_blueprint(str(tmp_path_factory.mktemp("cmux_system")))
    sysm = load_blueprint(path, cmux_memories=True)
    yield {"hip": hip, "keys": keys128, "orc": oracle128, "st": st, "bk": bk, "bk2": bk2, "K": K, "pk": pk, "sysm": sysm,
           "lowered": load_blueprint(path)}
    bk2.free()
    pk.free()
    st.destroy()
    hip.cleanup()


def test_one_clock_word_for_word(gpu):
    cases.one_clock_words(gpu["keys"], gpu["orc"], gpu["sysm"], gpu["bk"], gpu["K"], gpu["bk2"], gpu["pk"])


def test_six_clocks_decrypt_to_the_lowered_forms_packets(gpu):
    """real keys throughout: the fixture's bk2 and the full-size private key-switching key of the same lvl2 key (n_in = 2048, t = 10,
    basebit = 3, 2.35 GB, made and uploaded in windows of rows).  run_packet — reset cycle, ROM and cycle-0 RAM images from the packet's
    TRLWE forms, 6 clocks — and after every clock the decrypted result packet (outputs and the RAM image out of Ram.cells()) equals
    PlainEngine's on the lowered MUX form.  The RAM assertion is the full one: tests/test_cmux_ram_margin.py measured the write chain
    under such selectors on the CPU and nothing misreads there."""
    from iyokan_amd import runner
    from iyokan_amd.packet import TFHEPacket

    hip, keys, st = gpu["hip"], gpu["keys"], gpu["st"]
    req = cases.request(11, 6)
    want = []
    runner.run_packet(gpu["lowered"], req, on_cycle=lambda done, eng: want.append(runner.result_packet(gpu["lowered"], eng, done)))
    assert any(want[c].ram["ram"] != want[c + 1].ram["ram"] for c in range(5)) and any(want[c].bits["out"] != want[c + 1].bits["out"] for c in range(5))
    s2 = client.keygen_lvl2(N2, seed=31)                                            # the fixture's bk2 is under this key
    pk = hip.PrivKsKey(N2, 10, 3)
    eng = be = None
    try:
        for first in range(0, pk.rows, 8192):
            pk.upload(st, first, client.privks_key_rows(keys, s2, 10, 3, first_row=first, row_count=min(8192, pk.rows - first), seed=41))
        st.sync()
        eng, be = cases.gpu_engine(keys, gpu["sysm"], gpu["bk2"], pk, TFHEPacket.encrypt(keys, req, seed=700))
        got = []
        res = runner.run_packet(gpu["sysm"], req, engine=eng, on_cycle=lambda done, e: got.append(runner.result_packet(gpu["sysm"], e, done)))
    finally:
        if eng is not None:
            eng.free()
            be.close()
        pk.free()
    for c in range(6):
        print(f"clock {c + 1}: out {got[c].bits['out']} want {want[c].bits['out']}; ram {got[c].ram['ram']} want {want[c].ram['ram']}")
    for c in range(6):
        assert want[c].same_content(got[c]), (c, want[c].diff(got[c]))
    assert want[-1].same_content(res)


def test_engine_refuses_what_it_cannot_run(gpu):
    hip, keys, sysm = gpu["hip"], gpu["keys"], gpu["sysm"]
    other = hip.Bk2Key(2)
    try:
        with pytest.raises(ValueError, match="n = 2"):
            cases.gpu_engine(keys, sysm, other, gpu["pk"], None)
    finally:
        other.free()
    eng, be = cases.gpu_engine(keys, sysm, gpu["bk2"], gpu["pk"], None)
    try:
        with pytest.raises(ValueError, match="packet=TFHEPacket"):
            eng.load_rom("rom", None)
    finally:
        eng.free()
        be.close()


def test_circuit_bootstrap_batch_refusals_and_words(gpu):
    """every refusal the one call adds leaves the lvl2 store and the scratch rows as they were; a valid call afterwards gives the lvl2
    TLWEs, the scratch rows and — through a ROM read — the selectors of cmux.selectors_from_tlwe0"""
    hip, keys, st, bk2, pk = gpu["hip"], gpu["keys"], gpu["st"], gpu["bk2"], gpu["pk"]
    p = keys.params
    A, l, per, N = 3, int(p.l), int(p.trgsw_rows), int(p.N)
    arena = hip.Arena(4)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1, 1], seed=77))
    t2, scratch = hip.Tlwe2(N2, A * l + 1), hip.Trlwe(A * per)
    t2_short, t2_small_n, scratch_short = hip.Tlwe2(N2, A * l - 1), hip.Tlwe2(64, A * l + 1), hip.Trlwe(A * per - 1)
    pk_small_n, bk2_other, pk_other = hip.PrivKsKey(64, 1, 1), hip.Bk2Key(2, gpu_index=1), hip.PrivKsKey(N2, 1, 1, gpu_index=1)
    bk2_small_n = hip.Bk2Key(2)
    data = np.random.default_rng(93).integers(0, 1 << 32, size=(8, 2 * N), dtype=np.uint64).astype(np.uint32)
    rom_a, rom_b = (cmux.Rom(st, data, A, N.bit_length() - 1) for _ in range(2))
    out = hip.Arena(2 * N)
    fill2, fill1 = np.full((A * l + 1, N2 + 1), FILL64, dtype=np.uint64), np.full((A * per, 2 * N), FILL32, dtype=np.uint32)
    slots, sign = [2, 0, 1], [1, -1, 1]
    try:
        t2.upload(st, 0, fill2)
        t2_short.upload(st, 0, fill2[:A * l - 1])
        scratch.upload(st, 0, fill1)
        scratch_short.upload(st, 0, fill1[:-1])
        ok = dict(bk2=bk2, pk=pk, arena=arena, in_=slots, sign=sign, t2=t2, first=1, scratch=scratch, trgsw=rom_a.trgsw, first_slot=0)
        bad = {
            "short scratch": (dict(scratch=scratch_short), "fewer than bits"),
            "lvl2 store too small": (dict(t2=t2_short), "do not fit the lvl2 store"),
            "lvl2 first slot too far": (dict(first=2), "do not fit the lvl2 store"),
            "n_in of the store": (dict(t2=t2_small_n), "not the 2048"),
            "n_in of the private key": (dict(pk=pk_small_n), "not the private key-switching key's"),
            "bk2 of another replica": (dict(bk2=bk2_other), "different GPUs"),
            "bk2 of another n": (dict(bk2=bk2_small_n), "not the initialised n"),
            "private key of another replica": (dict(pk=pk_other), "different GPUs"),
            "selector slots": (dict(first_slot=1), "selector slots outside"),
            "sign": (dict(sign=[1, 0, 1]), "sign outside"),
            "input slot": (dict(in_=[2, 4, 1]), "outside the lvl0 store"),
        }
        call = lambda a: st.circuit_bootstrap_batch(a["bk2"], a["pk"], a["arena"], a["in_"], a["sign"], a["t2"], a["first"], a["scratch"],
                                                    a["trgsw"], a["first_slot"])
        for what, (change, message) in bad.items():
            with pytest.raises(hip.IykHipError, match=r"iyk_hip_circuit_bootstrap_batch failed \(-1\): .*" + message):
                call({**ok, **change})
            assert np.array_equal(t2.download(st, 0, A * l + 1), fill2), what
            assert np.array_equal(t2_short.download(st, 0, A * l - 1), fill2[:A * l - 1]), what
            assert np.array_equal(scratch.download(st, 0, A * per), fill1), what
            assert np.array_equal(scratch_short.download(st, 0, A * per - 1), fill1[:-1]), what
        call(ok)                                                                    # and a valid call afterwards succeeds
        rom_a.read(None, out, np.arange(N).reshape(1, N), resident=True)
        got = (t2.download(st, 0, A * l + 1), scratch.download(st, 0, A * per), rom_a.trlwe.download(st, rom_a.row(0, rom_a.layout.result), 1),
               st.download(out, 0, N))
        t2.upload(st, 0, fill2)
        scratch.upload(st, 0, fill1)
        for s, (slot, sg) in enumerate(zip(slots, sign)):                           # the composed path, bit by bit: it has one sign per call
            cmux.selectors_from_tlwe0(st, bk2, pk, arena, [slot], t2, 1 + s * l, scratch, rom_b.trgsw, first_slot=s, invert=sg < 0)
            if s == 0:
                first_rows = scratch.download(st, 0, per)
        rom_b.read(None, out, np.arange(N, 2 * N).reshape(1, N), resident=True)
        want = (t2.download(st, 0, A * l + 1), rom_b.trlwe.download(st, rom_b.row(0, rom_b.layout.result), 1), st.download(out, N, N))
    finally:
        for x in (arena, t2, scratch, t2_short, t2_small_n, scratch_short, pk_small_n, bk2_other, bk2_small_n, pk_other, rom_a, rom_b, out):
            x.free()
    assert np.array_equal(got[0], want[0]) and (got[0][0] == FILL64).all() and not (got[0][1:] == FILL64).all(axis=1).any()
    assert np.array_equal(got[1][:per], first_rows) and not (got[1] == FILL32).all(axis=1).any()
    assert np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2]) and got[2].any()
