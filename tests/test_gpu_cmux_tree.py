"""GPU: the fused CMUX read tree — cmux_tree_kernel through iyk_hip_cmux_tree_batch, Rom.read(fused_tree=True) and
Ram.read_port(fused_tree=True).  The cases of tests/cmux_tree_cases.py (the words tests/test_cmux_tree_emulation.py runs through the
emulation) word for word against the exact reference of tests/cmux_ref.py applied level by level, against the same trees sent as `levels`
cmux_batch launches on the same store, Rom.read and Ram.read_port fused against unfused, the refusals through the C ABI and the debug
build's rounding figure.  The 128-bit set here; the 80-bit set and the debug initialisation run in a child process
(tests/cmux_tree_child.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cmux_tree_cases as cases
import memory_cases
from iyokan_amd import client, cmux

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(keys128):
    from iyokan_amd import hip

    hip.initialize(keys128, device_ids=(0,))
    yield hip, keys128
    hip.cleanup()


@pytest.fixture(scope="module")
def store(gpu):
    """The 32-slot selector store of tests/cmux_tree_cases.py, uploaded once."""
    hip, keys = gpu
    st = hip.Stream(0)
    sel = hip.Trgsw(cases.SLOTS)
    sel.upload(st, 0, cases.selectors(keys))
    st.sync()
    yield st, sel
    sel.free()
    st.destroy()


def _run(hip, st, sel, T, batches, unfused=False):
    """every batch queued on the stream without a sync in between, then the rows; unfused: as cmux_batch launches, the candidates of job
    g between its levels in rows behind T"""
    extra = 14 * max(len(jobs) for jobs in batches) if unfused else 0
    trl = hip.Trlwe(T.shape[0] + extra)
    try:
        trl.upload(st, 0, T)
        for jobs in batches:
            if unfused:
                for launch in cases.as_cmux_launches(jobs, T.shape[0]):
                    st.cmux_batch(sel, trl, *zip(*launch))
            else:
                st.cmux_tree_batch(sel, trl, *zip(*jobs))
        st.sync()
        return trl.download(st, 0, T.shape[0])
    finally:
        trl.free()


@pytest.mark.parametrize("name", list(cases.GPU_CASES))
def test_kernel_equals_reference(gpu, store, name):
    """single: 1 job of 4 levels.  side_by_side: levels 1 .. 4 in one launch on shared leaves, every job ending on the store's last
    selector slot.  nine: 9 jobs that share their leaves, selectors of every kind.  in_place: out == the job's own first (and last)
    leaf.  zero: the result is leaf 0 exactly.  last: fresh selectors of 1, 1, 1, 1 on leaves that encrypt a 1 in the last leaf only —
    the result decrypts to 1.  two_groups: two dependent batches without a sync."""
    hip, keys = gpu
    st, sel = store
    (_, T, batches), want = cases.expected_of(keys, name)
    got = _run(hip, st, sel, T, batches)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{name}: rows that differ from the reference: {bad[:10]}"
    written = {j[3] for jobs in batches for j in jobs}
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])
    for out, same in cases.IDENTITIES.get(name, ()):
        assert np.array_equal(got[out], T[same]), (out, same)
    if name == "last":
        assert list(client.decrypt_ram_trlwe(keys, got[[j[3] for j in batches[0]]])) == [1, 1, 1, 1]


@pytest.mark.parametrize("name", ["side_by_side", "nine", "in_place", "two_groups"])
def test_kernel_equals_cmux_batch_launches(gpu, store, name):
    """the same trees as max(levels) cmux_batch launches of two-row jobs on the same stream and store: byte-equal rows"""
    hip, keys = gpu
    st, sel = store
    _, T, batches = cases.GPU_CASES[name](keys)
    assert np.array_equal(_run(hip, st, sel, T, batches), _run(hip, st, sel, T, batches, unfused=True))


@pytest.mark.parametrize("aw,lw", [(9, 3), (12, 0)])
def test_rom_read_fused_tree_equals_unfused(gpu, aw, lw):
    """two simultaneous reads of a ROM with a two-level upper tree: the tree as one cmux_tree_batch and as one cmux_batch per level, in
    front of the unfused and of the fused tail — every rdata arena word and the result rows equal, and every bit decrypts to the ROM's
    content"""
    hip, keys = gpu
    bits, data, addresses, trgsw = memory_cases.rom_case(keys, aw, lw)
    wb = 1 << lw
    got = {}
    for kw in ((False, False), (False, True), (True, True)):
        st = hip.Stream(0)
        rom = cmux.Rom(st, data, aw, lw, max_reads=2)
        arena = hip.Arena(2 * wb)
        try:
            rom.read(trgsw[2:4], arena, np.arange(2 * wb).reshape(2, wb), fused=kw[0], fused_tree=kw[1])
            st.sync()
            got[kw] = (st.download(arena, 0, 2 * wb), np.stack([rom.trlwe.download(st, rom.row(r, rom.layout.result), 1)[0] for r in range(2)]))
        finally:
            arena.free()
            rom.free()
            st.destroy()
    for kw in ((False, True), (True, True)):
        assert np.array_equal(got[kw][0], got[False, False][0]) and np.array_equal(got[kw][1], got[False, False][1]), kw
    want_bits = np.stack([bits[a * wb : (a + 1) * wb] for a in addresses[2:4]])
    assert np.array_equal(client.decrypt_bits(keys, got[False, True][0]).reshape(2, wb), want_bits)


@pytest.mark.parametrize("aw,dw", [(1, 1), (5, 2), (8, 1)])
def test_ram_read_port_fused_tree_equals_unfused(gpu, aw, dw):
    """RAM 2 x 1 (one level), 32 x 2 (five levels: a group of 4 and a group of 1, two planes) and 256 x 1 (two groups of 4): rdata words
    equal fused against unfused, and rdata decrypts to the addressed word"""
    hip, keys = gpu
    p = keys.params
    C = 1 << aw
    rng = np.random.default_rng([11, 0x7D, aw, dw])
    content = rng.integers(0, 2, size=dw * C).astype(np.uint8)
    cells = client.encrypt_ram_trlwe(keys, content, seed=60 + aw).reshape(dw * C, 2 * p.N)
    addr = (0xB5 & (C - 1)) | (C >> 1)
    trgsw = client.encrypt_trgsw(keys, [(addr >> k) & 1 for k in range(aw)], seed=70 + aw)
    got = {}
    for fused_tree in (False, True):
        st = hip.Stream(0)
        ram = cmux.Ram(st, cells, aw, dw)
        arena = hip.Arena(dw)
        try:
            ram.trgsw.upload(st, 0, np.ascontiguousarray(trgsw, dtype=np.uint32).reshape(aw, ram.trgsw.words))
            ram.read_port(arena, np.arange(dw), fused_tree=fused_tree)
            st.sync()
            got[fused_tree] = st.download(arena, 0, dw)
            assert np.array_equal(ram.cells().reshape(dw * C, -1), cells)   # a read writes no cell
        finally:
            arena.free()
            ram.free()
            st.destroy()
    assert np.array_equal(got[True], got[False])
    assert list(client.decrypt_bits(keys, got[True])) == [int(content[d * C + addr]) for d in range(dw)]


def test_refusals_leave_the_store_unchanged(gpu, store):
    """one bad field each through the C ABI: IYK_ERR_INVALID with its text, nothing staged or launched — the rows come back as uploaded"""
    hip, keys = gpu
    st, sel = store
    _, T, _ = cases.nine(keys)
    rows, slots = T.shape[0], cases.SLOTS
    L = hip.lib()
    bad = {
        "levels 0": (([0], [0], [0], [16]), "levels outside [1, 4]"),
        "levels 5": (([0], [5], [0], [16]), "levels outside [1, 4]"),
        "sel0 -1": (([-1], [1], [0], [16]), "selector index outside the selector store"),
        "sel0 + levels > trgsw_slots": (([slots - 3], [4], [0], [16]), "selector index outside the selector store"),
        "first -1": (([0], [1], [-1], [16]), "TRLWE index outside the buffer"),
        "the last leaf == trlwe_slots": (([0], [4], [rows - 15], [0]), "TRLWE index outside the buffer"),
        "out == trlwe_slots": (([0], [1], [0], [rows]), "TRLWE index outside the buffer"),
        "out[g] a leaf of h": (([0, 0], [2, 2], [0, 4], [5, 16]), "a job reads a TRLWE row that another job of the batch writes"),
        "out[g] == out[h]": (([0, 0], [2, 2], [0, 4], [16, 16]), "two jobs of one batch write the same TRLWE row"),
    }
    trl = hip.Trlwe(rows)
    try:
        trl.upload(st, 0, T)
        for name, (lists, text) in bad.items():
            arrs = [np.asarray(a, dtype=np.int32) for a in lists]
            rc = L.iyk_hip_cmux_tree_batch(st.h, sel.ptr, sel.slots, trl.ptr, trl.slots, len(arrs[0]),
                                           *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for a in arrs])
            assert rc == -1, name
            assert L.iyk_hip_last_error().decode() == text, name
        with pytest.raises(hip.IykHipError, match="levels outside"):
            st.cmux_tree_batch(sel, trl, [0], [0], [0], [16])
        st.sync()
        assert np.array_equal(trl.download(st, 0, rows), T)
        # an own leaf as out and shared leaves are accepted
        st.cmux_tree_batch(sel, trl, [cases.ZERO] * 3, [4, 2, 1], [0, 0, 18], [16, 17, 19])
        st.sync()
        got = trl.download(st, 0, rows)
    finally:
        trl.free()
    want = T.copy()
    want[16], want[17], want[19] = T[0], T[0], T[18]   # zero selectors: leaf 0 of each job comes back
    assert np.array_equal(got, want)


def _child(mode, env=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cmux_tree_child.py"), mode], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and f"ok {mode}" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_80bit_set():
    """levels 1 .. 4 side by side and the nine jobs at the 80-bit set (Gadget<2, 10>), in a fresh process, against the reference"""
    env = {k: v for k, v in os.environ.items() if k != "IYK_HIP_DEBUG"}
    _child("80bit", env)


def test_debug_round_error():
    """IYK_HIP_DEBUG=1 in a fresh process: the CHECK form of the kernel equals the reference on the nine jobs and on the worst-case words
    and feeds iyk_hip_fft_round_error; the figure stays below the bound DESIGN.md section 2b proves for the 128-bit set, 2^-8.5"""
    out = _child("debug", dict(os.environ, IYK_HIP_DEBUG="1"))
    line = [ln for ln in out.splitlines() if ln.startswith("round_error")][-1]
    print(line)
    assert 0.0 < float(line.split()[1]) < 2.0 ** -8.5
