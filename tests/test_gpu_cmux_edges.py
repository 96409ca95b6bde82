"""GPU: the CMUX memories at the chain lengths, batch shapes, store sizes and plan shapes the other CMUX tests do not run — the chosen
cases of tests/cmux_cases.py (the words tests/test_ram_emulation.py and tests/test_cmux_emulation.py run through the emulation), stores
beyond 4 GiB, ROM / RAM shapes, the second replica and the refusal without FFT key spectra.  Every comparison is word for word against
the exact reference (tests/cmux_ref.py, tests/ram_ref.py, the oracle's key switch and blind rotation), on both parameter sets.

The two tests that need an initialisation of their own run it in a child process (tests/cmux_edges_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cmux_cases
import cmux_ref
import memory_cases
import ram_ref
from iyokan_amd import client, cmux

pytestmark = pytest.mark.gpu


def _rows(p, seed, count):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(count, 2 * p.N), dtype=np.uint64).astype(np.uint32)


def _child(mode):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cmux_edges_child.py"), mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok {mode}" in r.stdout, r.stdout + r.stderr


def test_second_replica():
    """Two replicas aliased to device 0 (as test_gpu_zz_debug.py does), in a fresh process (tests/cmux_edges_child.py): the stores and
    the stream of replica 1 — its own copy of the transform constants — run one cmux_batch, one chain batch and one index extraction,
    word for word against the reference."""
    _child("replica")


def test_refused_without_fft_spectra():
    """IYK_HIP_NTT=fp at init, in a fresh process (tests/cmux_edges_child.py): the selector store and both CMUX entry points answer the
    state error that names the missing spectra and launch nothing; the row add and the index extraction, which need no spectra, still
    work."""
    _child("refused")


@pytest.fixture(scope="module", params=["128", "80"])
def gpu(request):
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + request.param)
    orc = request.getfixturevalue("oracle" + request.param)
    hip.initialize(keys, device_ids=(0,))
    yield hip, keys, orc, request.param
    hip.cleanup()


@pytest.fixture(scope="module")
def store(gpu):
    """The 128-slot selector store of tests/cmux_cases.py, uploaded once per parameter set."""
    hip, keys, _, _ = gpu
    trgsw = cmux_cases.selectors(keys)
    st = hip.Stream(0)
    sel = hip.Trgsw(cmux_cases.SLOTS)
    sel.upload(st, 0, trgsw)
    st.sync()
    yield st, sel, trgsw
    sel.free()
    st.destroy()


def _assert_rows(got, want, what=""):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: rows that differ from the reference: {bad[:10]}"


@pytest.mark.parametrize("name", list(cmux_cases.CHAIN_CASES))
def test_chain_cases(gpu, store, name):
    """A: 8 / 16 / 31 / 32 steps, pattern bits up to 31, chains that end on the store's last slot.  B: steps 1 .. 32 in one workgroup.
    C: 301 jobs, 38 workgroups, the last one partial.  D: src == mem, chains on zero selectors (closed forms as well).  E: twelve
    dependent batches queued without a sync.  A and B also against the same chains sent as `steps` cmux_batch launches."""
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    _, T, batches = cmux_cases.CHAIN_CASES[name](keys)
    rows = T.shape[0]
    fused = hip.Trlwe(rows)
    unfused = hip.Trlwe(rows) if name[0] in "AB" else None
    try:
        fused.upload(st, 0, T)
        for jobs in batches:
            st.cmux_chain_batch(sel, fused, *zip(*jobs))
        if unfused is not None:
            unfused.upload(st, 0, T)
            jobs = batches[0]
            step_jobs = [ram_ref.chain_as_cmux_jobs(j, cmux_cases.accumulator_row(jobs, g)) for g, j in enumerate(jobs)]
            for s in range(max(j[1] for j in jobs)):
                st.cmux_batch(sel, unfused, *zip(*(c[s] for c in step_jobs if s < len(c))))
        st.sync()
        got = fused.download(st, 0, rows)
        got_steps = unfused.download(st, 0, rows) if unfused is not None else None
    finally:
        fused.free()
        if unfused is not None:
            unfused.free()
    want = T.copy()
    for jobs in batches:
        ram_ref.run_chains(p, want, trgsw, jobs)
    _assert_rows(got, want, name)
    written = sorted({j[5] for jobs in batches for j in jobs})
    untouched = [r for r in range(rows) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])
    if got_steps is not None:
        assert np.array_equal(got[written], got_steps[written])
    if name == "D":
        for out, same in cmux_cases.D_IDENTITIES:
            assert np.array_equal(got[out], T[same]), (out, same)


def test_cmux_degenerate_and_last_slot(gpu, store):
    """in0 == in1 and rot = 0 (the output is T[in0] word for word), a job on the last selector slot, a batch that is all on it"""
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    _, T, batches = cmux_cases.cmux_cases(keys)
    trl = hip.Trlwe(T.shape[0])
    try:
        trl.upload(st, 0, T)
        st.cmux_batch(sel, trl, *zip(*batches[0]))
        st.sync()
        first = trl.download(st, 0, T.shape[0])
        st.cmux_batch(sel, trl, *zip(*batches[1]))
        st.sync()
        got = trl.download(st, 0, T.shape[0])
    finally:
        trl.free()
    want = cmux_ref.run_jobs(p, T.copy(), trgsw, batches[0])
    _assert_rows(first, want, "first batch")
    for out, same in cmux_cases.CMUX_IDENTITIES:
        assert np.array_equal(first[out], T[same]), (out, same)
    _assert_rows(got, cmux_ref.run_jobs(p, want, trgsw, batches[1]), "second batch")


def _need_free(nbytes, what):
    import torch

    free = torch.cuda.mem_get_info()[0]
    if free < 2 * nbytes:
        pytest.skip(f"{what}: needs 2 x {nbytes} bytes free, the device has {free}: short by {2 * nbytes - free}")


def test_stores_beyond_4_gib(gpu):
    """Stores past every 32-bit limit the kernels' address arithmetic could meet, one after the other.
    (a) A selector store of 2^32 // slot_bytes + 3 slots (just over 4 GiB): selectors in the first two and the last three slots, a
        mixed cmux_batch on each of them and a 3-step chain that ends on the last slot.
    (b) A row store of 2^21 + 3 rows (just over 16 GiB: past a 32-bit byte offset at row 2^19, a signed 32-bit word index at 2^20 and
        an unsigned one at 2^21): rows 0, 1, 2, 2^19 + 1, 2^20 + 1, 2^21, 2^21 + 1, 2^21 + 2 hold data; both CMUX kernels, the row add,
        the blind rotation with trlwe_out and the index extraction read and write the high rows; rows 0, 1, 2 — what the high rows
        alias modulo 2^32 bytes and modulo 2^32 words — are only ever read and must come back unchanged.
    Not covered: the selector store's 32-bit ELEMENT index (16-byte complex values) wraps only at 64 GiB, and a 32-bit index of doubles at
    32 GiB — too much memory to hold on a shared card."""
    hip, keys, orc, _ = gpu
    p = keys.params
    N = p.N
    trgsw = cmux_cases.selectors(keys)
    st = hip.Stream(0)
    try:
        # (a)
        slot_bytes = (p.k + 1) * p.l * (p.k + 1) * N * 16
        slots = (1 << 32) // slot_bytes + 3
        _need_free(slots * slot_bytes, "selector store")
        at = [0, 1, slots - 3, slots - 2, slots - 1]
        five = trgsw[[cmux_cases.UNIFORM, cmux_cases.FRESH, cmux_cases.ALT, cmux_cases.ALT + 1, cmux_cases.UNIFORM + 5]]
        T = _rows(p, 61, 16)
        jobs = [(at[g], g, -1 if g == 3 else 5 + g, 1029 if g == 3 else 0, (10 + g, g, 5 + g)[g % 3]) for g in range(5)]
        chain = (slots - 3, 3, 0b101, 12, 0, 14)
        sel = hip.Trgsw(slots)
        trl = hip.Trlwe(T.shape[0])
        try:
            sel.upload(st, 0, five[:2])
            sel.upload(st, slots - 3, five[2:])
            trl.upload(st, 0, T)
            st.cmux_batch(sel, trl, *zip(*jobs))
            st.cmux_chain_batch(sel, trl, *zip(chain))
            st.sync()
            got = trl.download(st, 0, T.shape[0])
        finally:
            sel.free()
            trl.free()
        low = {s: n for n, s in enumerate(at)}   # the reference holds the five selectors alone
        want = cmux_ref.run_jobs(p, T.copy(), five, [(low[j[0]],) + j[1:] for j in jobs])
        ram_ref.run_chains(p, want, five, [(low[chain[0]],) + chain[1:]])
        _assert_rows(got, want, "selector store beyond 4 GiB")

        # (b)
        rows = (1 << 21) + 3
        _need_free(rows * 2 * N * 4, "row store")
        A, B, C, D, E = (1 << 19) + 1, (1 << 20) + 1, 1 << 21, (1 << 21) + 1, (1 << 21) + 2
        held = [0, 1, 2, A, B, C, D, E]
        m = {r: n for n, r in enumerate(held)}   # the reference holds the eight rows alone
        T = _rows(p, 62, len(held))
        tlwe = client.encrypt_bits(keys, [1, 0], seed=63)
        U = cmux_cases.UNIFORM
        # every stage is downloaded and compared before the next one writes over its rows
        # two-row form with in0 high, rotate form in place on a high row, low ins to a high out, in1 high and written over
        jobs = [(U + 1, B, 0, 0, C), (U + 2, D, -1, 5, D), (cmux_cases.ALT + 3, 1, 2, 0, A), (U + 5, 2, E, 0, E)]
        # src high, mem low; src low, mem high, in place; src and mem high, in place
        chains = [(U + 8, 3, 0b101, C, 1, E), (cmux_cases.FRESH + 4, 2, 0b10, 0, A, A), (cmux_cases.ALT + 10, 2, 0b01, D, B, B)]
        adds = ([E, 2], [0, B], [C, B])
        rot_out = [D, A]
        ext_rows, ext_h = [A, B, C, D, E, 0], [0, 1, N // 2, N - 1, 7, 3]
        sel = hip.Trgsw(cmux_cases.SLOTS)
        trl = hip.Trlwe(rows)
        arena = hip.Arena(2 + len(ext_rows))
        snapshot = lambda: np.concatenate([trl.download(st, r, 1) for r in held])   # download(first=...), synchronises
        try:
            sel.upload(st, 0, trgsw)
            for r in held:
                trl.upload(st, r, T[m[r]])
            st.upload(arena, 0, tlwe)
            st.cmux_batch(sel, trl, *zip(*jobs))
            got_cmux = snapshot()
            st.cmux_chain_batch(sel, trl, *zip(*chains))
            got_chain = snapshot()
            st.trlwe_add_batch(trl, *adds, int(p.mu))
            got_add = snapshot()
            st.bootstrap_trlwe_batch(arena, [0, 1], [-1, -1], [1, 1], [0, 0], np.zeros(2, dtype=np.uint32), trl.ptr, trlwe_slots=trl.slots,
                                     trlwe_out=rot_out)
            st.sample_extract_index_keyswitch_batch(trl, ext_rows, ext_h, np.arange(2, 2 + len(ext_rows)), arena)
            got = snapshot()
            got_tlwe = st.download(arena, 2, len(ext_rows))
        finally:
            sel.free()
            trl.free()
            arena.free()
        want = cmux_ref.run_jobs(p, T.copy(), trgsw, [(j[0], m[j[1]], -1 if j[2] < 0 else m[j[2]], j[3], m[j[4]]) for j in jobs])
        _assert_rows(got_cmux, want, f"cmux_batch on a row store beyond 16 GiB, rows {held}")
        ram_ref.run_chains(p, want, trgsw, [j[:3] + (m[j[3]], m[j[4]], m[j[5]]) for j in chains])
        _assert_rows(got_chain, want, f"cmux_chain_batch on a row store beyond 16 GiB, rows {held}")
        for a, b, out in zip(*adds):
            row = (want[m[a]] + want[m[b]]).astype(np.uint32)
            row[N] = (int(row[N]) + int(p.mu)) & 0xFFFFFFFF
            want[m[out]] = row
        _assert_rows(got_add, want, f"trlwe_add_batch on a row store beyond 16 GiB, rows {held}")
        for r, ct in zip(rot_out, tlwe):
            want[m[r]] = ram_ref.blind_rotate(orc, ct)
        _assert_rows(got, want, f"bootstrap_trlwe_batch on a row store beyond 16 GiB, rows {held}")
        for stage in (got_cmux, got_chain, got_add, got):
            assert np.array_equal(stage[:3], T[:3])   # the rows the high ones alias
        for g, (r, h) in enumerate(zip(ext_rows, ext_h)):
            assert np.array_equal(got_tlwe[g], orc.keyswitch(cmux_ref.sample_extract_index(want[m[r]], h, N))), (r, h)
    finally:
        st.destroy()


@pytest.mark.parametrize("aw,lw", memory_cases.ROM_SHAPES)
def test_rom_shapes(gpu, aw, lw):
    """cmux.Rom sized for three reads, two reads per call (reads < max_reads), two calls: no upper tree, a one-level tree that writes
    the result row directly, a two-level tree, 1-bit words, no rotate steps.  Every arena word equals CMUX plan -> index extraction ->
    the oracle's key switch (at 1024-bit words: all 1024 of one read, 16 of each of the others); every bit decrypts."""
    hip, keys, orc, _ = gpu
    p = keys.params
    bits, data, addresses, trgsw = memory_cases.rom_case(keys, aw, lw)
    wb = 1 << lw
    st = hip.Stream(0)
    rom = cmux.Rom(st, data, aw, lw, max_reads=3)
    arena = hip.Arena(4 * wb)
    try:
        for call in range(2):
            rom.read(trgsw[2 * call : 2 * call + 2], arena, np.arange(2 * call * wb, (2 * call + 2) * wb).reshape(2, wb))
        st.sync()
        got = st.download(arena, 0, 4 * wb)
    finally:
        arena.free()
        rom.free()
        st.destroy()
    sample = np.random.default_rng(aw).choice(wb, size=min(16, wb), replace=False)
    for r, addr in enumerate(addresses):
        row = cmux_ref.rom_read(p, data, trgsw[r], aw, lw)
        for i in (range(wb) if r == 0 or wb <= 16 else sample):
            assert np.array_equal(got[r * wb + i], orc.keyswitch(cmux_ref.sample_extract_index(row, i, p.N))), (addr, i)
    want_bits = np.stack([bits[a * wb : (a + 1) * wb] for a in addresses])
    assert np.array_equal(client.decrypt_bits(keys, got).reshape(4, wb), want_bits)


@pytest.mark.parametrize("aw", memory_cases.RAM_SHAPES)
def test_ram_shapes(gpu, aw):
    """cmux.Ram at 2 x 1 (addr_width = 1) and 16 x 1, fused and unfused: a write, then a read of the same address; rdata and the cells
    word for word against ram_ref.clock and by decryption"""
    hip, keys, orc, _ = gpu
    p = keys.params
    content, cells, clocks = memory_cases.ram_case(keys, aw)
    trace = ram_ref.run_clocks(p, orc, cells, clocks)
    runs = {}
    for fused in (True, False):
        st = hip.Stream(0)
        ram = cmux.Ram(st, cells, aw, 1)
        arena = hip.Arena(3)   # wren, wdata, rdata
        out = []
        try:
            for _, _, _, sel, cts in clocks:
                st.upload(arena, 0, cts)
                ram.clock(sel, arena, 0, [1], [2], fused=fused)
                st.sync()
                out.append((st.download(arena, 2, 1), ram.cells()))
        finally:
            arena.free()
            ram.free()
            st.destroy()
        runs[fused] = out
    words = [int(b) for b in content]
    for n, ((addr, wren, wdata, _, _), (rdata, _, new)) in enumerate(zip(clocks, trace)):
        read = words[addr]
        if wren:
            words[addr] = wdata
        for fused, out in runs.items():
            got_rdata, got_cells = out[n]
            assert np.array_equal(got_rdata, rdata), (fused, n)
            _assert_rows(got_cells[0], new[0], f"fused={fused}, clock {n}")
            assert [int(b) for b in client.decrypt_bits(keys, got_rdata)] == [read], (fused, n)
            assert [int(b) for b in client.decrypt_ram_trlwe(keys, got_cells[0])] == words, (fused, n)
