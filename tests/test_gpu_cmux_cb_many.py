"""GPU: cb_many on the CMUX-memory engines (runner.CmuxCipherEngine / CmuxLaneEngine): every circuit bootstrapping of a clock as ONE
rotation per address bit (iyk_hip_circuit_bootstrap_many_batch).  The small system of tests/test_gpu_cmux_system.py word for word
against the emulation of the many-digit rotation -> privks_ref -> cmux_ref / ram_ref, the flags against the plain cb_many engine and
every lane of a two-lane engine against a one-lane engine on that lane's request (the hand-built system of tests/read_early_cases.py),
and two clocks under the full-size private key against PlainEngine on the lowered form.

The rotation's reference at n = 636 is NOT independent of the kernels: the emulation compiles the device functions the kernels run (a
restated rotation of 636 steps per address bit would take minutes).  What is independent is the numpy restatement tests/cb_many_ref.py,
which holds the emulation at n = 19 (tests/test_cb_many_cases.py) and the kernels at n = 19 (tests/test_gpu_cb_many.py), and the
decryption of the last test here."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cb_many_cases as mc
import cb_rotate_ref
import cmux_system_cases as cases
import privks_ref
from iyokan_amd import client
from test_gpu_cmux_system import N2, gpu  # noqa: F401  (the module's fixture: the keys, imported and not copied)
import test_gpu_read_early as early
from test_gpu_read_early import BOTH, _run, _same, hand  # noqa: F401  (hand: the fixture)

pytestmark = pytest.mark.gpu


def _many_selectors(p, tlwes, ntt, K):
    """cases.restated_selectors with ONE many-digit rotation per address bit: u32 [bits][(k+1) l][k+1][N]"""
    l = int(p.l)
    mu = [cb_rotate_ref.mu_of(r, p.Bgbit) for r in range(l)]
    with ThreadPoolExecutor(max_workers=8) as pool:                                 # the emulation releases the GIL
        rot = list(pool.map(lambda t: mc.rotate("wg", t, 1, 0, mu, ntt), tlwes))
    row_fn = privks_ref.key_rows_of(K)
    return np.stack([privks_ref.selector_rows(list(rot[b]), 1, 1, row_fn, l) for b in range(len(tlwes))])


def test_one_clock_word_for_word(gpu, monkeypatch):  # noqa: F811
    """the ROM result row, both memories' rdata TLWEs and the RAM cells after tick()"""
    monkeypatch.setattr(cases, "restated_selectors", _many_selectors)
    cases.one_clock_words(gpu["keys"], gpu["orc"], gpu["sysm"], gpu["bk"], gpu["K"], gpu["bk2"], gpu["pk"], cb_many=True)


def _one_lane_clock(gpu, sysm, bk2, r, monkeypatch, **kw):  # noqa: F811
    """One clock of a ONE-lane engine on lane r's request: packet r of the lane engine's packets and lane r's register values
    (test_gpu_read_early._drive gives lane r the counter bits [1, r, 1]), looked at as _drive looks at a lane engine's lane."""
    packets = early._packets(gpu, r + 1)
    with monkeypatch.context() as mp:
        mp.setattr(early, "_packets", lambda g, lanes: packets[r:r + 1])
        eng, be = early._engine(gpu, sysm, bk2, 1, **kw)
    probe = gpu["hip"].Trlwe(2 + max(pt.addr_width for pt in sysm.ports))
    try:
        N = int(gpu["keys"].params.N)
        probe.upload(eng.stream, 0, np.random.default_rng(61).integers(0, 1 << 32, size=(2, 2 * N), dtype=np.uint64).astype(np.uint32))
        eng.load_rom("rom", None)
        eng.load_ram("ram", None)
        root = sysm.nl.roots()
        rom, ram = sysm.ports
        regs = [root[a] for a in ram.addr] + [root[ram.wren[0]]]
        cnt = sorted({root[j] for a in rom.addr for j in sysm.nl.ins[root[a]]})
        eng.set_nodes(cnt + regs, [1, r, 1] + [0, 1] + [1])
        eng.run()
        state = early._state(eng, be, sysm, probe)
        eng.tick()
        return [(state, [eng.mem["ram"].cells()])]
    finally:
        probe.free()
        eng.free()
        be.close()


def test_flags_give_the_plain_cb_many_engines_words(gpu, hand):  # noqa: F811
    ref = _run(gpu, hand, gpu["bk2"], clocks=1, cb_many=True)
    _same(ref, _run(gpu, hand, gpu["bk2"], clocks=1, cb_many=True, read_early=True, **BOTH), "cb_many, stage_cb + refresh_aside + read_early")


def test_each_lane_gives_the_one_lane_engines_words(gpu, hand, monkeypatch):  # noqa: F811
    """CmuxLaneEngine(K = 2, cb_many=True): lane r's arena words, ROM row, selectors (through a probe CMUX) and RAM cells are those of a
    one-lane CmuxCipherEngine(cb_many=True) given request r; the same with every flag on"""
    (s2, c2), = _run(gpu, hand, gpu["bk2"], lanes=2, clocks=1, cb_many=True)
    assert not np.array_equal(s2[0][1], s2[1][1])                                   # the lanes read other ROM words
    (f2, d2), = _run(gpu, hand, gpu["bk2"], lanes=2, clocks=1, cb_many=True, read_early=True, **BOTH)
    for r in range(2):
        one = _one_lane_clock(gpu, hand, gpu["bk2"], r, monkeypatch, cb_many=True)
        _same(one, [([s2[r]], [c2[r]])], f"lane {r} of two against the one-lane engine on request {r}")
        _same(one, [([f2[r]], [d2[r]])], f"lane {r} of two with every flag against the one-lane engine on request {r}")


def test_cb_many_off_gives_todays_words(gpu, hand):  # noqa: F811
    today = _run(gpu, hand, gpu["bk2"], clocks=1)
    _same(today, _run(gpu, hand, gpu["bk2"], clocks=1, cb_many=False), "cb_many=False")
    on = _run(gpu, hand, gpu["bk2"], clocks=1, cb_many=True)
    assert not np.array_equal(today[0][0][0][2]["rom"], on[0][0][0][2]["rom"])      # and on: other selector words


def test_two_clocks_decrypt_to_the_lowered_forms_packets(gpu):  # noqa: F811
    """real keys throughout, built as tests/test_gpu_cmux_system.py builds them (the full-size private key-switching key of the fixture's
    lvl2 key): after each of two clocks the decrypted result packet, RAM image included, equals PlainEngine's on the lowered form."""
    from iyokan_amd import runner
    from iyokan_amd.packet import TFHEPacket

    hip, keys, st = gpu["hip"], gpu["keys"], gpu["st"]
    req = cases.request(11, 2)
    want = []
    runner.run_packet(gpu["lowered"], req, on_cycle=lambda done, eng: want.append(runner.result_packet(gpu["lowered"], eng, done)))
    s2 = client.keygen_lvl2(N2, seed=31)
    pk = hip.PrivKsKey(N2, 10, 3)
    eng = be = None
    try:
        for first in range(0, pk.rows, 8192):
            pk.upload(st, first, client.privks_key_rows(keys, s2, 10, 3, first_row=first, row_count=min(8192, pk.rows - first), seed=41))
        st.sync()
        eng, be = cases.gpu_engine(keys, gpu["sysm"], gpu["bk2"], pk, TFHEPacket.encrypt(keys, req, seed=700), cb_many=True)
        got = []
        res = runner.run_packet(gpu["sysm"], req, engine=eng, on_cycle=lambda done, e: got.append(runner.result_packet(gpu["sysm"], e, done)))
    finally:
        if eng is not None:
            eng.free()
            be.close()
        pk.free()
    for c in range(2):
        print(f"clock {c + 1}: out {got[c].bits['out']} want {want[c].bits['out']}; ram {got[c].ram['ram']} want {want[c].ram['ram']}")
    for c in range(2):
        assert want[c].same_content(got[c]), (c, want[c].diff(got[c]))
    assert want[-1].same_content(res)
