"""GPU: memory ports read as soon as their address is ready (runner.CmuxCipherEngine / CmuxLaneEngine(read_early=True): every memory on
a port stream beside the executor's), at the 128-bit set under the keys of tests/test_gpu_cmux_system.py (a real bk2 at n = 636, a
uniform private key: words only).  The system is the hand-built one of tests/read_early_cases.py; the reference is the engine with
the flag off — on the plan of before the flag — fed the same ciphertexts and images, which the existing suite pins to the emulation.

Compared word for word: the TLWE of every node after each run() (the whole arena but the DFF shadow slots, which hold a value inside
tick() only; node by node: the two plans place the address cones at different levels, the words do not depend on it), the ROM's
result row, every RAM cell after each tick(), and every selector slot through what it does — the ABI downloads no selector: ONE
cmux_batch job per slot on two uniform rows of a probe store."""
import numpy as np
import pytest

import read_early_cases as cases
from iyokan_amd import client
from iyokan_amd.system import load_blueprint
from test_gpu_cmux_system import gpu  # noqa: F401  (the module's fixture: the keys, imported and not copied)

pytestmark = pytest.mark.gpu

CLOCKS = 3
BOTH = dict(stage_cb=True, refresh_aside=True)


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    return load_blueprint(cases.write_blueprint(str(tmp_path_factory.mktemp("gpu_read_early"))), cmux_memories=True)


def _packets(gpu, lanes):  # noqa: F811
    from iyokan_amd.packet import TFHEPacket

    return [TFHEPacket.encrypt(gpu["keys"], cases.request(3 + r, 1), seed=500 + r) for r in range(lanes)]


def _engine(gpu, sysm, bk2, lanes=1, executor=None, **kw):  # noqa: F811
    """(engine, backend): the plan knows port_ready only where the flag is set, so the flag-off engine runs the plan of before it"""
    import torch

    from iyokan_amd import runner
    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend

    keys = gpu["keys"]
    if executor is None:
        plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages, **({"early": sysm.ports} if kw.get("read_early") else {}))
        be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0), **({"lanes": lanes} if lanes > 1 else {}))
        executor = FrontierExecutor(plan, be)
    be = executor.be
    # the same bits give the same ciphertext in every engine and lane: word equality needs equal inputs
    encrypt = lambda bits: client.encrypt_bits(keys, bits, seed=9000 + sum(int(b) << i for i, b in enumerate(bits)) % 4096 + 4096 * len(bits))
    common = (sysm, executor, encrypt, lambda rows: client.decrypt_bits(keys, rows), client.trivial(keys.params, 0), bk2, gpu["pk"])
    packets = _packets(gpu, lanes)
    try:
        if lanes > 1:
            eng = runner.CmuxLaneEngine(*common, packets=packets, decrypt_ram=lambda rows: [0] * len(rows), **kw)
        else:
            eng = runner.CmuxCipherEngine(*common, packet=packets[0], decrypt_ram=lambda rows: [0] * len(rows), **kw)
    except Exception:
        be.close()
        raise
    return eng, be


def _lane(lane):
    return {"lane": lane} if lane else {}


def _state(eng, be, sysm, probe):
    """after a run(): per lane (the TLWE of every node, the ROM's result row, one probe row per selector slot)"""
    plan = eng.ex.plan
    slots = [plan.slot[i] for i in range(sysm.nl.num_nodes)]
    assert min(slots) >= 0
    out = []
    for lane in range(eng.lanes):
        arena = be.read_many(slots, **_lane(lane))
        rom = eng.mem["rom"]
        row = rom.trlwe.download(rom.stream, lane * rom.row_stride + rom.row(0, rom.layout.result), 1)[0]
        sel = {}
        for pt in sysm.ports:
            mem, k = eng.mem[pt.name], pt.addr_width
            first = mem.sel_base + lane * (mem.sel_stride if eng.lanes > 1 else 0)
            mem.stream.cmux_batch(mem.trgsw, probe, np.arange(first, first + k), [0] * k, [1] * k, [0] * k, np.arange(2, 2 + k))
            sel[pt.name] = probe.download(mem.stream, 2, k)
        out.append((arena, row, sel))
    return out


def _drive(gpu, sysm, eng, be, clocks=CLOCKS, look=True):  # noqa: F811
    """`clocks` clocks from counter = 5, wren = 1, RAM address 2.  look: after every run() the state, after every tick() every RAM cell
    (each a synchronisation); look=False: nothing is read and nothing synchronises between the first run() and the last tick() — then
    only waits on the device order the streams — and the trace has the last clock's cells alone."""
    hip, p = gpu["hip"], gpu["keys"].params
    probe = hip.Trlwe(2 + max(pt.addr_width for pt in sysm.ports))
    trace = []
    try:
        probe.upload(eng.stream, 0, np.random.default_rng(61).integers(0, 1 << 32, size=(2, 2 * p.N), dtype=np.uint64).astype(np.uint32))
        for lane in range(eng.lanes):
            eng.load_rom("rom", None, **_lane(lane))
            eng.load_ram("ram", None, **_lane(lane))
        root = sysm.nl.roots()
        rom, ram = sysm.ports
        regs = [root[a] for a in ram.addr] + [root[ram.wren[0]]]
        assert all(sysm.nl.kinds[i] == "DFF" for i in regs)
        cnt = sorted({root[j] for a in rom.addr for j in sysm.nl.ins[root[a]]})      # the counter: what the address XORs read
        assert len(cnt) == 3 and all(sysm.nl.kinds[i] == "DFF" for i in cnt)
        for lane in range(eng.lanes):
            eng.set_nodes(cnt + regs, [1, lane, 1] + [0, 1] + [1], **_lane(lane))
        for c in range(clocks):
            eng.run()
            state = _state(eng, be, sysm, probe) if look else None
            eng.tick()
            cells = [eng.mem["ram"].cells(**_lane(lane)) for lane in range(eng.lanes)] if look or c == clocks - 1 else None
            trace.append((state, cells))
    finally:
        probe.free()
    return trace


def _same(want, got, what):
    assert len(want) == len(got)
    for c, ((s0, c0), (s1, c1)) in enumerate(zip(want, got)):
        if s1 is not None:
            for lane, ((a0, r0, p0), (a1, r1, p1)) in enumerate(zip(s0, s1)):
                bad = np.flatnonzero((a0 != a1).any(axis=1))
                assert bad.size == 0, (what, "arena: nodes", bad[:8], c, lane)
                assert np.array_equal(r0, r1), (what, "rom row", c, lane)
                for name in p0:
                    assert np.array_equal(p0[name], p1[name]), (what, "selectors", name, c, lane)
        if c1 is not None:
            for lane, (x0, x1) in enumerate(zip(c0, c1)):
                assert np.array_equal(x0, x1), (what, "cells", c, lane)


def _run(gpu, sysm, bk2, lanes=1, clocks=CLOCKS, look=True, **kw):  # noqa: F811
    eng, be = _engine(gpu, sysm, bk2, lanes, **kw)
    try:
        return _drive(gpu, sysm, eng, be, clocks, look)
    finally:
        eng.free()
        be.close()


@pytest.fixture(scope="module")
def want(gpu, hand):  # noqa: F811
    """three clocks of the engine as it stands, computed once"""
    trace = _run(gpu, hand, gpu["bk2"])
    for c in range(1, CLOCKS):                                                      # the clocks differ: the counter moves, every cell is refreshed
        assert not np.array_equal(trace[c][0][0][1], trace[c - 1][0][0][1]) and (trace[c][1][0] != trace[c - 1][1][0]).any(axis=2).all()
    assert all(trace[0][0][0][2][n].any() for n in ("rom", "ram"))
    return trace


def test_three_clocks_give_the_words_of_the_engine_as_it_stands(gpu, hand, want):  # noqa: F811
    _same(want, _run(gpu, hand, gpu["bk2"], read_early=True), "read_early")
    _same(want, _run(gpu, hand, gpu["bk2"], read_early=True, **BOTH), "read_early + stage_cb + refresh_aside")


def test_two_clocks_back_to_back_without_a_host_sync(gpu, hand, want):  # noqa: F811
    """tick() and the next run() enqueued behind each other: the cells after the second clock are the reference's"""
    for kw in ({}, BOTH):
        got = _run(gpu, hand, gpu["bk2"], clocks=2, look=False, read_early=True, **kw)
        assert got[0] == (None, None) and got[1][0] is None
        assert np.array_equal(got[1][1][0], want[1][1][0]), kw


def test_one_clock_under_the_fp64_form_of_the_lvl2_key(gpu, hand, want):  # noqa: F811
    hip, keys, st, bk = gpu["hip"], gpu["keys"], gpu["st"], gpu["bk"]
    bk2 = hip.Bk2Key(keys.params.n, form="fft")
    try:
        for first in range(0, keys.params.n, 200):
            bk2.upload(st, first, bk[first:first + 200])
        st.sync()
        ref = _run(gpu, hand, bk2, clocks=1)
        _same(ref, _run(gpu, hand, bk2, clocks=1, read_early=True, **BOTH), "fft key, read_early + both")
        _same(want[:1], ref, "the two key forms")                                   # every output word is the same under either form
    finally:
        bk2.free()


def test_lane_engine_two_lanes_two_clocks(gpu, hand):  # noqa: F811
    ref = _run(gpu, hand, gpu["bk2"], lanes=2, clocks=2)
    assert not np.array_equal(ref[0][0][0][1], ref[0][0][1][1])                     # the lanes read other ROM words
    _same(ref, _run(gpu, hand, gpu["bk2"], lanes=2, clocks=2, read_early=True), "two lanes, read_early")
    _same(ref, _run(gpu, hand, gpu["bk2"], lanes=2, clocks=2, read_early=True, **BOTH), "two lanes, read_early + both")


def test_free_behind_a_run_whose_join_is_pending_then_a_second_engine(gpu, hand, want):  # noqa: F811
    """two clocks, a third run() and free() at once — the join and the reads still queued on the device — then a second engine on the
    same executor and GPU: the same words again"""
    flags = dict(read_early=True, **BOTH)
    eng, be = _engine(gpu, hand, gpu["bk2"], **flags)
    eng2 = None
    try:
        first = _drive(gpu, hand, eng, be, clocks=2)
        _same(want[:2], first, "first engine")
        eng.run()
        eng.free()
        assert eng.port_stream is None and eng.refresh_stream is None
        eng2, _ = _engine(gpu, hand, gpu["bk2"], executor=eng.ex, **flags)
        _same(first, _drive(gpu, hand, eng2, be, clocks=2), "second engine")
    finally:
        if eng2 is not None:
            eng2.free()
        be.close()
