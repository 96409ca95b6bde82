"""GPU: the fused rotate chain of a ROM read — cmux_rotate_chain_kernel through iyk_hip_cmux_rotate_chain_batch and Rom.read(fused=True).
The cases of tests/rom_chain_cases.py (the words tests/test_rom_chain_emulation.py runs through the emulation) word for word against the
exact reference of tests/cmux_ref.py applied step by step, against the same chains sent as `steps` cmux_batch launches, Rom.read fused
against unfused, the refusals through the C ABI and the debug build's rounding figure.  The 128-bit set here; the 80-bit set and the
debug initialisation run in a child process (tests/rom_chain_child.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cmux_cases
import memory_cases
import rom_chain_cases as cases
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
    """The 128-slot selector store of tests/cmux_cases.py, uploaded once."""
    hip, keys = gpu
    st = hip.Stream(0)
    sel = hip.Trgsw(cmux_cases.SLOTS)
    sel.upload(st, 0, cmux_cases.selectors(keys))
    st.sync()
    yield st, sel
    sel.free()
    st.destroy()


def _run_fused(hip, st, sel, T, batches):
    """every batch queued on the stream without a sync in between, then the rows"""
    trl = hip.Trlwe(T.shape[0])
    try:
        trl.upload(st, 0, T)
        for jobs in batches:
            st.cmux_rotate_chain_batch(sel, trl, *cases.flat(jobs))
        st.sync()
        return trl.download(st, 0, T.shape[0])
    finally:
        trl.free()


@pytest.mark.parametrize("name", list(cases.GPU_CASES))
def test_kernel_equals_reference(gpu, store, name):
    """one: 1 job.  wg8: steps 1 .. 8 side by side in one workgroup.  wg9: a second, partial workgroup; shared src, in place.  many: 301
    jobs, 38 workgroups, every third on the shared src.  steps32: 32 steps on the store's last slots.  rot0 (out == src exactly) and
    rotN.  queued: twelve dependent batches without a sync, more than the stream's eight staging slots."""
    hip, keys = gpu
    st, sel = store
    (_, T, batches), want = cases.expected_of(keys, name)
    got = _run_fused(hip, st, sel, T, batches)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{name}: rows that differ from the reference: {bad[:10]}"
    written = {j[4] for jobs in batches for j in jobs}
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])
    for out, same in cases.IDENTITIES.get(name, ()):
        assert np.array_equal(got[out], T[same]), (out, same)


@pytest.mark.parametrize("name", ["wg9", "steps32"])
def test_kernel_equals_cmux_batch_launches(gpu, store, name):
    """the same chains as max(steps) cmux_batch launches of rotate-form jobs on the same stream: byte-equal rows"""
    hip, keys = gpu
    st, sel = store
    _, T, batches = cases.GPU_CASES[name](keys)
    fused = _run_fused(hip, st, sel, T, batches)
    trl = hip.Trlwe(T.shape[0])
    try:
        trl.upload(st, 0, T)
        for jobs in batches:
            for launch in cases.as_cmux_launches(jobs):
                st.cmux_batch(sel, trl, *zip(*launch))
        st.sync()
        unfused = trl.download(st, 0, T.shape[0])
    finally:
        trl.free()
    assert np.array_equal(fused, unfused)


@pytest.mark.parametrize("aw,lw", [(8, 3), (12, 0), (2, 10), (3, 3)])   # (3, 3): no upper tree, both reads start from the one data row
def test_rom_read_fused_equals_unfused(gpu, aw, lw):
    """two simultaneous reads of a ROM, the tail as one cmux_rotate_chain_batch and as one cmux_batch per step: every rdata arena word
    equal, and every bit decrypts to the ROM's content.  (2, 10) has no rotate step: fused=True sends what fused=False sends."""
    hip, keys = gpu
    bits, data, addresses, trgsw = memory_cases.rom_case(keys, aw, lw)
    wb = 1 << lw
    got = {}
    for fused in (False, True):
        st = hip.Stream(0)
        rom = cmux.Rom(st, data, aw, lw, max_reads=2)
        arena = hip.Arena(2 * wb)
        try:
            rom.read(trgsw[2:4], arena, np.arange(2 * wb).reshape(2, wb), fused=fused)
            st.sync()
            got[fused] = st.download(arena, 0, 2 * wb)
            result = [rom.trlwe.download(st, rom.row(r, rom.layout.result), 1)[0] for r in range(2)]
        finally:
            arena.free()
            rom.free()
            st.destroy()
        got[fused, "rows"] = np.stack(result)
    assert np.array_equal(got[True], got[False])
    assert np.array_equal(got[True, "rows"], got[False, "rows"])
    want_bits = np.stack([bits[a * wb : (a + 1) * wb] for a in addresses[2:4]])
    assert np.array_equal(client.decrypt_bits(keys, got[True]).reshape(2, wb), want_bits)
    upper, chain = rom.launches_fused(2)   # plan and layout only: the stores are gone
    assert (chain is None) == (lw == 10) and len(upper) + (chain[0][0] if chain else 0) == len(rom.plan)


def test_refusals_leave_the_store_unchanged(gpu, store):
    """one bad field each through the C ABI: IYK_ERR_INVALID with its text, nothing staged or launched — the rows come back as uploaded"""
    hip, keys = gpu
    st, sel = store
    _, T, _ = cases.workgroup(keys, 8)
    rows, slots, N2 = T.shape[0], cmux_cases.SLOTS, 2 * keys.params.N
    L = hip.lib()
    bad = {
        "steps 0": (([0], [0], [1], [0], [9]), "steps outside [1, 32]"),
        "steps 33": (([33], [0] * 33, [1] * 33, [0], [9]), "steps outside [1, 32]"),
        "sel -1": (([2], [0, -1], [1, 1], [0], [9]), "selector index outside the selector store"),
        "sel == trgsw_slots": (([1], [slots], [1], [0], [9]), "selector index outside the selector store"),
        "rot -1": (([1], [0], [-1], [0], [9]), "rot outside [0, 2N)"),
        "rot == 2N": (([1], [0], [N2], [0], [9]), "rot outside [0, 2N)"),
        "src == trlwe_slots": (([1], [0], [1], [rows], [9]), "TRLWE index outside the buffer"),
        "out == trlwe_slots": (([1], [0], [1], [0], [rows]), "TRLWE index outside the buffer"),
        "out[g] == src[h]": (([1, 1], [0, 1], [1, 2], [0, 9], [9, 10]), "a job reads a TRLWE row that another job of the batch writes"),
        "out[g] == out[h]": (([1, 1], [0, 1], [1, 2], [0, 1], [9, 9]), "two jobs of one batch write the same TRLWE row"),
    }
    trl = hip.Trlwe(rows)
    try:
        trl.upload(st, 0, T)
        for name, (lists, text) in bad.items():
            arrs = [np.asarray(a, dtype=np.int32) for a in lists]
            rc = L.iyk_hip_cmux_rotate_chain_batch(st.h, sel.ptr, sel.slots, trl.ptr, trl.slots, len(arrs[0]),
                                                   *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for a in arrs])
            assert rc == -1, name
            assert L.iyk_hip_last_error().decode() == text, name
        with pytest.raises(hip.IykHipError, match="steps outside"):
            st.cmux_rotate_chain_batch(sel, trl, [0], [0], [1], [0], [9])
        with pytest.raises(ValueError):   # fewer (sel, rot) pairs than the jobs state: never handed to the library
            st.cmux_rotate_chain_batch(sel, trl, [2], [0], [1], [0], [9])
        st.sync()
        assert np.array_equal(trl.download(st, 0, rows), T)
        # in place and a shared src are accepted
        st.cmux_rotate_chain_batch(sel, trl, [1, 1, 1], [cmux_cases.ZERO] * 3, [5, 6, 7], [0, 0, 3], [9, 10, 3])
        st.sync()
        got = trl.download(st, 0, rows)
    finally:
        trl.free()
    want = T.copy()
    want[9], want[10] = T[0], T[0]   # zero selectors: the accumulator comes back
    assert np.array_equal(got, want)


def _child(mode, env=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "rom_chain_child.py"), mode], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and f"ok {mode}" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_80bit_set():
    """the nine-job batch and the 32-step chain at the 80-bit set (Gadget<2, 10>), in a fresh process, against the reference"""
    env = {k: v for k, v in os.environ.items() if k != "IYK_HIP_DEBUG"}
    _child("80bit", env)


def test_debug_round_error():
    """IYK_HIP_DEBUG=1 in a fresh process: the CHECK form of the kernel equals the reference on the 32-step chain and feeds
    iyk_hip_fft_round_error; the figure stays below the suite's trip-wire of 2^-10 (DESIGN.md section 2b proves 2^-8.5)"""
    out = _child("debug", dict(os.environ, IYK_HIP_DEBUG="1"))
    line = [ln for ln in out.splitlines() if ln.startswith("round_error")][-1]
    print(line)
    assert 0.0 < float(line.split()[1]) < 2.0 ** -10
