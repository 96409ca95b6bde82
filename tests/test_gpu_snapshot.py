"""GPU: snapshot and resume of the cipher engines (snapshot.EngineState on runner.CmuxCipherEngine / CmuxLaneEngine / CipherEngine) at the
128-bit set, under the keys of tests/test_gpu_cmux_system.py (a real bk2 at n = 636, a uniform private key: words only) on the small
system of tests/cmux_system_cases.py — ROM 3 x 4, RAM 2 x 2, 12 gates: a DFF, a ROM port, a RAM port with write-back, a second stage.

The engines are deterministic, so a run that is split — some clocks, state(), free(), a NEW engine on a NEW stream, load_state, the
rest — has to give the straight run's WORDS: every node's TLWE, the ROM's result row and every RAM cell row after tick().  G6 alone
decrypts, and for that builds the full-size private key-switching key as tests/test_gpu_cmux_system.py does."""
import numpy as np
import pytest

import cb_rotate_cases
import cmux_system_cases as cases
from iyokan_amd import client, runner
from iyokan_amd.snapshot import Snapshot
from netlist_util import gold
from test_gpu_cmux_system import gpu  # noqa: F401  (the module's fixture: the keys, imported and not copied)

pytestmark = pytest.mark.gpu

ALL = dict(stage_cb=True, refresh_aside=True, read_early=True)
DUMMY = lambda rows: [0] * len(rows)   # noqa: E731  (under the uniform private key nothing decrypts)


def _encrypt(keys):
    # the same bits give the same ciphertext in every engine and lane: word equality needs equal inputs
    return lambda bits: client.encrypt_bits(keys, bits, seed=9000 + sum(int(b) << i for i, b in enumerate(bits)) % 4096 + 4096 * len(bits))


def _engine(gpu, packets, pk=None, decrypt_ram=DUMMY, **kw):  # noqa: F811
    """(engine, backend) on a fresh HipBackend — a stream of its own — for the small system; len(packets) lanes"""
    import torch

    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend

    keys, sysm, lanes = gpu["keys"], gpu["sysm"], len(packets)
    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages, **({"early": sysm.ports} if kw.get("read_early") else {}))
    be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0), **({"lanes": lanes} if lanes > 1 else {}))
    common = (sysm, FrontierExecutor(plan, be), _encrypt(keys), lambda rows: client.decrypt_bits(keys, rows), client.trivial(keys.params, 0),
              gpu["bk2"], pk or gpu["pk"])
    try:
        if lanes > 1:
            eng = runner.CmuxLaneEngine(*common, packets=packets, decrypt_ram=decrypt_ram, **kw)
        else:
            eng = runner.CmuxCipherEngine(*common, packet=packets[0], decrypt_ram=decrypt_ram, **kw)
    except Exception:
        be.close()
        raise
    return eng, be


def _packet(gpu, seed, cycles):  # noqa: F811
    from iyokan_amd.packet import TFHEPacket

    req = cases.request(seed, cycles)
    return req, TFHEPacket.encrypt(gpu["keys"], req, seed=500 + seed)


def _lane(lane):
    return {"lane": lane} if lane else {}


def _words(eng, be):
    """after a run(): per lane (every node's TLWE, the ROM's result row)"""
    plan, rom = eng.ex.plan, eng.mem["rom"]
    slots = [plan.slot[i] for i in range(eng.nl.num_nodes)]
    return [(be.read_many(slots, **_lane(lane)), rom.trlwe.download(rom.stream, lane * rom.row_stride + rom.row(0, rom.layout.result), 1)[0])
            for lane in range(eng.lanes)]


def _cells(eng):
    return [eng.mem["ram"].cells(**_lane(lane)) for lane in range(eng.lanes)]


def _clock(eng, be, trace, look=True):
    """tick() + run() by hand; look: the cells after the tick and the words after the run go into `trace`"""
    eng.tick()
    cells = _cells(eng) if look else None
    eng.run()
    if look:
        trace.append((cells, _words(eng, be)))


def _start(gpu, eng, req):  # noqa: F811
    """run_packet's steps up to the first run(): images, the reset cycle"""
    sysm = gpu["sysm"]
    runner._load_roms(sysm, eng, req)
    eng.set_nodes([sysm.nl.inputs[("reset", 0)]], [1])
    eng.run()
    eng.tick()
    eng.set_nodes([sysm.nl.inputs[("reset", 0)]], [0])
    runner._load_rams(sysm, eng, req)
    eng.run()


def _same(a, b):
    for (cells_a, words_a), (cells_b, words_b) in zip(a, b):
        for lane in range(len(cells_a)):
            assert np.array_equal(cells_a[lane], cells_b[lane]), "RAM cell rows"
            assert np.array_equal(words_a[lane][0], words_b[lane][0]), "arena words"
            assert np.array_equal(words_a[lane][1], words_b[lane][1]), "ROM result row"
    assert len(a) == len(b)


def _split_by_hand(gpu, flags, look_before_state=True):  # noqa: F811
    """(the straight run's trace of clocks 3 and 4, the split run's): clock 1 is _start, clock 2 a _clock, then state() / load_state"""
    req, packet = _packet(gpu, 11, 4)
    eng, be = _engine(gpu, [packet], **flags)
    want = []
    try:
        _start(gpu, eng, req)
        _clock(eng, be, want)
        _clock(eng, be, want)
        _clock(eng, be, want)
    finally:
        eng.free()
        be.close()
    eng, be = _engine(gpu, [packet], **flags)
    try:
        _start(gpu, eng, req)
        _clock(eng, be, [], look=look_before_state)     # look=False: nothing synchronises between run() and state() but state() itself
        snap = eng.state(done=2, reset_ran=True)
    finally:
        eng.free()
        be.close()
    eng, be = _engine(gpu, [None], **flags)              # a new engine, a new stream, no request packet: the snapshot has the images
    got = []
    try:
        eng.load_state(snap)
        _clock(eng, be, got)
        _clock(eng, be, got)
    finally:
        eng.free()
        be.close()
    assert (want[1][0][0] != want[2][0][0]).any() and (want[1][1][0][0] != want[2][1][0][0]).any()   # the clocks do differ
    return want[1:], got, snap


def test_g1_cmux_engine_flags_off_split_equals_straight(gpu):  # noqa: F811
    want, got, snap = _split_by_hand(gpu, {})
    _same(want, got)
    assert snap.meta["engine"] == "CmuxCipherEngine" and snap.meta["params"]["n"] == 636 and snap.ram["ram"].shape == (1, 2, 4, 2048)
    assert snap.rom["rom"].shape == (1, 1, 2048) and snap.rom["rom"].any()


def test_g2_all_three_flags_on(gpu):  # noqa: F811
    want, got, _ = _split_by_hand(gpu, ALL, look_before_state=False)
    _same(want, got)


def test_g3_lane_engine_two_requests_through_run_packets(gpu, tmp_path):  # noqa: F811
    """snapshot_every=1 up to clock 1, resumed from the file and run up to clock 3 in total: each lane's result packet (decrypted
    with the one key both runs share; under the uniform private key the bits mean nothing, but equal words give equal bits) and
    every lane's cell rows, word for word"""
    keys, sysm = gpu["keys"], gpu["sysm"]
    pairs = [_packet(gpu, 21 + r, 3) for r in range(2)]
    reqs, packets = [p[0] for p in pairs], [p[1] for p in pairs]
    decrypt_ram = lambda rows: client.decrypt_ram_trlwe(keys, rows)
    path = str(tmp_path / "lanes.snapshot")
    eng, be = _engine(gpu, packets, decrypt_ram=decrypt_ram)
    try:
        want = runner.run_packets(sysm, reqs, engine=eng)
        want_cells, want_words = _cells(eng), _words(eng, be)
    finally:
        eng.free()
        be.close()
    eng, be = _engine(gpu, packets, decrypt_ram=decrypt_ram)
    try:
        runner.run_packets(sysm, reqs, cycles=1, engine=eng, snapshot_path=path, snapshot_every=1)
    finally:
        eng.free()
        be.close()
    snap = Snapshot.load(path)
    assert snap.done == 1 and snap.lanes == 2 and snap.reset_ran and snap.meta["engine"] == "CmuxLaneEngine"
    eng, be = _engine(gpu, [None, None], decrypt_ram=decrypt_ram)
    try:
        got = runner.run_packets(sysm, reqs, cycles=3, engine=eng, resume=path)
        got_cells, got_words = _cells(eng), _words(eng, be)
    finally:
        eng.free()
        be.close()
    for lane in range(2):
        assert want[lane].same_content(got[lane]), (lane, want[lane].diff(got[lane]))
        assert np.array_equal(want_cells[lane], got_cells[lane]) and np.array_equal(want_words[lane][0], got_words[lane][0]), lane
        assert np.array_equal(want_words[lane][1], got_words[lane][1]), lane
    assert not np.array_equal(want_cells[0], want_cells[1])


def test_g4_cipher_engine_on_a_lowered_netlist(gpu):  # noqa: F811
    """counter-4bit, 4 clocks, split at 2: the arena's words"""
    import torch

    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend
    from iyokan_amd.packet import PlainPacket
    from iyokan_amd.system import load_blueprint

    keys = gpu["keys"]
    sysm = load_blueprint(gold("counter-4bit.toml"))
    req = PlainPacket.load(gold("test13.in"))
    plan = FrontierPlan(sysm.nl, 1)

    def engine():
        be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0))
        return runner.CipherEngine(FrontierExecutor(plan, be), _encrypt(keys), lambda rows: client.decrypt_bits(keys, rows), client.trivial(keys.params, 0)), be

    arena = lambda be: be.read_many(sorted(set(plan.slot)))
    eng, be = engine()
    try:
        want = runner.run_packet(sysm, req, cycles=4, engine=eng)
        want_words = arena(be)
    finally:
        be.close()
    eng, be = engine()
    try:
        runner.run_packet(sysm, req, cycles=2, engine=eng)
        snap = eng.state(done=2, reset_ran=("reset", 0) in sysm.nl.inputs)
        at_two = arena(be)
    finally:
        be.close()
    eng, be = engine()
    try:
        got = runner.run_packet(sysm, req, cycles=4, engine=eng, resume=snap)
        got_words = arena(be)
    finally:
        be.close()
    assert np.array_equal(want_words, got_words) and not np.array_equal(at_two, got_words)
    assert want.same_content(got) and snap.meta["engine"] == "CipherEngine" and not snap.ram and not snap.rom


def test_g5_a_refused_load_state_changes_nothing(gpu):  # noqa: F811
    req, packet = _packet(gpu, 11, 4)
    eng, be = _engine(gpu, [packet])
    try:
        _start(gpu, eng, req)
        snap = eng.state(done=1, reset_ran=True)
        other = Snapshot(dict(snap.meta, lanes=2), snap.slots, np.concatenate([snap.arena, snap.arena]),
                         {n: np.concatenate([a, a]) for n, a in snap.ram.items()}, {n: np.concatenate([a, a]) for n, a in snap.rom.items()})
        slots = list(range(eng.ex.plan.num_slots))
        before = (be.read_many(slots), _cells(eng), _words(eng, be))
        with pytest.raises(ValueError, match="holds 2 lanes, this engine has 1"):
            eng.load_state(other)
        after = (be.read_many(slots), _cells(eng), _words(eng, be))
    finally:
        eng.free()
        be.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[2][0][1], after[2][0][1])
    assert before[0].any()


def test_g6_the_split_run_decrypts_to_the_lowered_forms_packet(gpu):  # noqa: F811
    """real keys throughout, as tests/test_gpu_cmux_system.py's six clocks: the fixture's bk2 and the full-size private key-switching
    key of the same lvl2 key.  G1's split — 2 clocks, state(), a new engine, 2 clocks — through run_packet; the decrypted result
    packet after clocks 3 and 4 equals PlainEngine's on the lowered form."""
    hip, keys, st, sysm = gpu["hip"], gpu["keys"], gpu["st"], gpu["sysm"]
    req, packet = _packet(gpu, 11, 4)
    want = []
    runner.run_packet(gpu["lowered"], req, on_cycle=lambda done, e: want.append(runner.result_packet(gpu["lowered"], e, done)))
    s2 = client.keygen_lvl2(cb_rotate_cases.N2, seed=31)                            # the fixture's bk2 is under this key
    pk = hip.PrivKsKey(cb_rotate_cases.N2, 10, 3)
    decrypt_ram = lambda rows: client.decrypt_ram_trlwe(keys, rows)
    got = []
    eng = be = None
    try:
        for first in range(0, pk.rows, 8192):
            pk.upload(st, first, client.privks_key_rows(keys, s2, 10, 3, first_row=first, row_count=min(8192, pk.rows - first), seed=41))
        st.sync()
        eng, be = _engine(gpu, [packet], pk=pk, decrypt_ram=decrypt_ram)
        at_two = runner.run_packet(sysm, req, cycles=2, engine=eng)
        snap = eng.state(done=2, reset_ran=True)
        eng.free()
        be.close()
        eng = be = None
        eng, be = _engine(gpu, [None], pk=pk, decrypt_ram=decrypt_ram)
        res = runner.run_packet(sysm, req, cycles=4, engine=eng, resume=snap, on_cycle=lambda done, e: got.append(runner.result_packet(sysm, e, done)))
    finally:
        if eng is not None:
            eng.free()
            be.close()
        pk.free()
    assert want[1].same_content(at_two), want[1].diff(at_two)
    assert len(got) == 2 and want[2].same_content(got[0]) and want[3].same_content(got[1]), (want[3].diff(got[1]))
    assert want[3].same_content(res) and not want[1].same_content(want[3])
