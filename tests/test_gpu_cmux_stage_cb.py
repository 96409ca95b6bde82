"""GPU: one circuit bootstrapping per stage and the RAM refresh on a second stream (runner.CmuxCipherEngine(stage_cb=, refresh_aside=)),
and iyk_hip_stream_wait_stream, at the 128-bit set under the keys of tests/test_gpu_cmux_system.py (a real bk2 at n = 636, a uniform
private key: words only).  The system is the four-port one of tests/cmux_stage_cases.py; the reference is the engine with both flags off
on the same inputs, which the existing suite pins to the emulation.

The ABI has no download of a selector slot (a store holds spectra).  A slot is compared through what it does: ONE cmux_batch job per slot
on the engine's stream, all on the same two uniform rows of a probe store — equal selectors give equal rows, word for word."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cmux_stage_cases as cases
import cmux_system_cases as small
import ram_ref
from iyokan_amd import client
from iyokan_amd.system import load_blueprint
from test_gpu_cmux_system import gpu  # noqa: F401  (the module's fixture: the keys, imported and not copied)

pytestmark = pytest.mark.gpu

CLOCKS = 3


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    return load_blueprint(cases.write_blueprint(str(tmp_path_factory.mktemp("cmux_stage"))), cmux_memories=True)


def _probe_selectors(hip, eng, probe, sysm):
    """{port: the rows one CMUX per selector slot of the port leaves}, on the engine's stream"""
    out = {}
    for pt in sysm.ports:
        mem, k = eng.mem[pt.name], pt.addr_width
        eng.stream.cmux_batch(mem.trgsw, probe, np.arange(mem.sel_base, mem.sel_base + k), [0] * k, [1] * k, [0] * k, np.arange(2, 2 + k))
        out[pt.name] = probe.download(eng.stream, 2, k)
    return out


def _run(gpu, sysm, bk2, cells_every_clock=True, clocks=CLOCKS, **kw):  # noqa: F811
    """`clocks` clocks from counter = 4, wren = 1; per clock the rdata TLWEs of every port, the selector probes and — after tick() —
    every RAM's cells.  cells_every_clock=False reads the cells after the last clock only, so that a refresh IS pending when the next
    clock's trees read: then only waits on the device stand between them."""
    eng, be = small.gpu_engine(gpu["keys"], sysm, bk2, gpu["pk"], _packet(gpu), **kw)
    try:
        return _drive(gpu, sysm, eng, be, cells_every_clock, clocks)
    finally:
        eng.free()
        be.close()


def _packet(gpu):  # noqa: F811
    from iyokan_amd.packet import TFHEPacket

    return TFHEPacket.encrypt(gpu["keys"], cases.request(3, 1), seed=500)


def _drive(gpu, sysm, eng, be, cells_every_clock=True, clocks=CLOCKS):  # noqa: F811
    hip, p = gpu["hip"], gpu["keys"].params
    probe = hip.Trlwe(2 + max(pt.addr_width for pt in sysm.ports))
    rams = [pt.name for pt in sysm.ports if pt.kind == "ram"]
    trace = []
    try:
        probe.upload(eng.stream, 0, np.random.default_rng(61).integers(0, 1 << 32, size=(2, 2 * p.N), dtype=np.uint64).astype(np.uint32))
        for pt in sysm.ports:
            (eng.load_rom if pt.kind == "rom" else eng.load_ram)(pt.name, None)
        root, slot = sysm.nl.roots(), eng.ex.plan.slot
        rom, rama = sysm.ports[0], sysm.ports[1]
        regs = [root[a] for a in rom.addr] + [root[rama.wren[0]]]
        assert all(sysm.nl.kinds[i] == "DFF" for i in regs)
        eng.set_nodes(regs, [0, 0, 1, 1])
        for c in range(clocks):
            eng.run()
            rdata = {pt.name: be.read_many([slot[i] for i in pt.rdata]) for pt in sysm.ports}
            sel = _probe_selectors(hip, eng, probe, sysm)
            eng.tick()
            last = c == clocks - 1
            trace.append((rdata, sel, {n: eng.mem[n].cells() for n in rams} if cells_every_clock or last else None))
    finally:
        probe.free()
    return trace


def _same(want, got, what):
    for c, ((r0, s0, c0), (r1, s1, c1)) in enumerate(zip(want, got)):
        for name in r0:
            assert np.array_equal(r0[name], r1[name]), (what, "rdata", name, c)
            assert np.array_equal(s0[name], s1[name]), (what, "selectors", name, c)
        if c1 is not None:
            for name in c0:
                assert np.array_equal(c0[name], c1[name]), (what, "cells", name, c)


def test_stage_cb_then_refresh_aside_give_the_words_of_the_engine_as_it_stands(gpu, four):  # noqa: F811
    want = _run(gpu, four, gpu["bk2"])
    # the clocks depend on each other: every clock rewrites every cell, and ramb / ramc read back the word the clock before wrote
    for c in range(1, CLOCKS):
        for name in ("ramb", "ramc"):
            assert not np.array_equal(want[c][0][name], want[c - 1][0][name]) and (want[c][2][name] != want[c - 1][2][name]).any(axis=2).all()
    assert all(want[0][1][n].any() for n in want[0][1])
    _same(want, _run(gpu, four, gpu["bk2"], stage_cb=True), "stage_cb")
    _same(want, _run(gpu, four, gpu["bk2"], stage_cb=True, refresh_aside=True), "stage_cb + refresh_aside")
    _same(want, _run(gpu, four, gpu["bk2"], refresh_aside=True, cells_every_clock=False), "refresh_aside, refresh pending at every read")
    _same(want, _run(gpu, four, gpu["bk2"], stage_cb=True, refresh_aside=True, rom_fused=True, tree_fused=True, cells_every_clock=False),
          "both, fused forms, refresh pending at every read")


def test_one_clock_under_the_fp64_form_of_the_lvl2_key(gpu, four):  # noqa: F811
    hip, keys, st, bk = gpu["hip"], gpu["keys"], gpu["st"], gpu["bk"]
    bk2 = hip.Bk2Key(keys.params.n, form="fft")
    try:
        for first in range(0, keys.params.n, 200):
            bk2.upload(st, first, bk[first:first + 200])
        st.sync()
        want = _run(gpu, four, bk2, clocks=1)
        _same(want, _run(gpu, four, bk2, clocks=1, stage_cb=True, refresh_aside=True), "fft key, both")
        _same(want, _run(gpu, four, gpu["bk2"], clocks=1), "the two key forms")     # every output word is the same under either form
    finally:
        bk2.free()


def test_wait_stream_orders_a_download_behind_a_queued_chain(gpu):  # noqa: F811
    hip, keys, a = gpu["hip"], gpu["keys"], gpu["st"]
    p = keys.params
    L = hip.lib()
    sub = client.encrypt_trgsw(keys, [1, 0], seed=5)
    jobs = 48
    T = np.random.default_rng(62).integers(0, 1 << 32, size=(1 + jobs, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    chains = [(0, 2, g & 3, 0, 1 + g, 1 + g) for g in range(jobs)]                   # in place on rows of their own, one shared src
    b = hip.Stream(0)
    sel, trl, ref = hip.Trgsw(2), hip.Trlwe(T.shape[0]), hip.Trlwe(T.shape[0])
    try:
        sel.upload(a, 0, sub)
        trl.upload(a, 0, T)
        ref.upload(a, 0, T)
        a.sync()
        # every refusal: nothing enqueued, the reason in the error text, the rows as they were
        for st, other, text in ((None, a.h, "null stream"), (a.h, None, "null stream"), (a.h, a.h, "cannot wait for itself")):
            assert L.iyk_hip_stream_wait_stream(st, other) == -1
            assert text in L.iyk_hip_last_error().decode()
        with pytest.raises(hip.IykHipError, match=r"iyk_hip_stream_wait_stream failed \(-1\): .*cannot wait for itself"):
            b.wait_stream(b)
        assert np.array_equal(trl.download(a, 0, T.shape[0]), T) and np.array_equal(trl.download(b, 0, T.shape[0]), T)
        a.cmux_chain_batch(sel, ref, *zip(*chains))
        want = ref.download(a, 0, T.shape[0])                                       # the chain's words, behind a synchronisation of A
        a.cmux_chain_batch(sel, trl, *zip(*chains))
        b.wait_stream(a)
        got = trl.download(b, 0, T.shape[0])                                        # synchronises B alone
    finally:
        for x in (sel, trl, ref):
            x.free()
        b.destroy()
    assert np.array_equal(got, want) and (got[1:] != T[1:]).any(axis=1).all() and np.array_equal(got[0], T[0])
    assert np.array_equal(got[:3], ram_ref.run_chains(p, T[:3].copy(), sub, chains[:2]))


def test_wait_stream_past_the_event_pool_and_twice(gpu):  # noqa: F811
    """64 waits each way, sixteen times the pool, then the two streams still hand rows over; a second stream after the first is destroyed
    does the same, and the resident key bytes are what they were"""
    hip, a = gpu["hip"], gpu["st"]
    N = int(gpu["keys"].params.N)
    rows = np.random.default_rng(63).integers(0, 1 << 32, size=(3, 2 * N), dtype=np.uint64).astype(np.uint32)
    before = hip.resident_key_bytes()
    trl = hip.Trlwe(3)
    try:
        for _ in range(2):                                                          # a second create / destroy cycle
            b = hip.Stream(0)
            try:
                trl.upload(a, 0, rows)
                for _ in range(64):
                    b.wait_stream(a)
                    a.wait_stream(b)
                a.trlwe_add_batch(trl, [0], [1], [2], 0)
                b.wait_stream(a)
                got = trl.download(b, 0, 3)
                a.sync()
            finally:
                b.destroy()
            assert np.array_equal(got[2], (rows[0] + rows[1]).astype(np.uint32)) and np.array_equal(got[:2], rows[:2])
    finally:
        trl.free()
    assert hip.resident_key_bytes() == before


def test_wait_stream_refuses_a_second_replica():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cmux_stage_child.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok replica" in r.stdout, r.stdout + r.stderr


def test_free_with_a_refresh_pending_then_a_second_engine(gpu, four):  # noqa: F811
    """the whole sequence twice in one process: two clocks, free() right behind a tick() whose refreshes are still pending, then a second
    engine on the same executor's stream and the same clocks again — the same words"""
    from iyokan_amd import runner

    keys = gpu["keys"]
    flags = dict(stage_cb=True, refresh_aside=True)
    eng, be = small.gpu_engine(keys, four, gpu["bk2"], gpu["pk"], _packet(gpu), **flags)
    eng2 = None
    try:
        first = _drive(gpu, four, eng, be, cells_every_clock=False, clocks=2)
        eng.run()
        eng.tick()
        assert all(eng.mem[n].pending_refresh is eng.refresh_stream for n in ("rama", "ramb", "ramc"))
        eng.free()                                                                  # with the refreshes pending
        assert eng.refresh_stream is None
        eng2 = runner.CmuxCipherEngine(four, eng.ex, lambda bits: client.encrypt_bits(keys, bits, seed=9001), eng.decrypt,
                                       client.trivial(keys.params, 0), gpu["bk2"], gpu["pk"], packet=_packet(gpu), decrypt_ram=eng.decrypt_ram,
                                       **flags)                                     # gpu_engine's first encryption has seed 9001
        _same(first, _drive(gpu, four, eng2, be, cells_every_clock=False, clocks=2), "second engine")
    finally:
        if eng2 is not None:
            eng2.free()
        be.close()
