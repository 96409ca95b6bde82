"""GPU: the matrix form of the key switch (keyswitch_mfma_kernel, IYK_HIP_KS_KERNEL=3 and the default for wide batches) against the
wave kernel (IYK_HIP_KS_KERNEL=1), word for word over the whole arena, at both parameter sets: the batch sizes around a wave's and
a workgroup's share of the gates, chosen digits (ks_words) and a key whose rows carry the bytes 0x80 / 0x7F in every plane."""
import ctypes
import os

import numpy as np
import pytest

import ks_matrix_cases as M
import ks_words as K
from iyokan_amd import client
from iyokan_amd.params import OPS
from test_gpu_keyswitch import FILL, KS_ENV, _run_case, _u32p

pytestmark = pytest.mark.gpu

ENV = KS_ENV + ("IYK_HIP_KS_MATRIX_MAX_BYTES",)
NCELLS = 640


def _emul():
    L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iyokan_amd", "lib", "libiyk_emul.so"))
    L.iyk_emul_ks_matrix_bytes.argtypes = [ctypes.c_int] * 2
    L.iyk_emul_ks_matrix_bytes.restype = ctypes.c_int64
    return L


_carry_keys = M.carry_keys    # the doctored key and the named cells live in ks_matrix_cases.py (checked by test_ks_matrix_cases.py)


def _cells(p, seed):
    """[NCELLS][2 N] TRLWE images: first the cells named by the test — every digit 0, every digit 3, a' = 0xFFFFFFFF, a' = -prec,
    one non-zero digit at (i, j) in the four corners —, then the families of ks_words.chosen_images, then uniform words.
    Returns (cells, number of named cells, number of named + chosen cells, t1[N] of the every-digit-0 cell)."""
    return M.cells(p, seed, NCELLS)


def _both(hip, st, d_trlwe, idx, p, monkeypatch, kinds, seed):
    """The same case (same output slots) under each of `kinds` (None: IYK_HIP_KS_KERNEL unset): {kind: arena}, out_slot."""
    got = {}
    for kind in kinds:
        if kind is None:
            monkeypatch.delenv("IYK_HIP_KS_KERNEL", raising=False)
        else:
            monkeypatch.setenv("IYK_HIP_KS_KERNEL", kind)
        got[kind], out_slot = _run_case(hip, st, d_trlwe, NCELLS, idx, p, np.random.default_rng(seed))
    return got, out_slot


def _same(got, a, b, out_slot, p, what):
    n = p.n
    rows = np.nonzero((got[a] != got[b]).any(axis=1))[0]
    if len(rows):
        s = rows[0]
        words = np.nonzero(got[a][s] != got[b][s])[0]
        job = np.nonzero(out_slot == s)[0]
        pytest.fail(f"{what}: {len(rows)} slots differ between kinds {a} and {b}; slot {s} (job {job.tolist()}): {len(words)} words, "
                    f"first {words[:6].tolist()} (word n = {n})")
    free = np.setdiff1d(np.arange(len(got[a])), out_slot)
    assert (got[a][free] == FILL).all(), f"{what}: a slot no job wrote lost its fill"   # the words behind a gate's row included


@pytest.mark.parametrize("which", ["128", "80"])
def test_matrix_form_equals_the_wave_kernel(which, request, monkeypatch):
    """First the default dispatch at KS_MATRIX_MIN_JOBS gates: the words of IYK_HIP_KS_KERNEL=2, and the resident key bytes grow by
    exactly the operand.  Then kind 3 against kind 1 at 1 (each named cell alone), 31, 33, W - 1, W + 1, B - 1, B, B + 1 and 2 B + 1
    gates (W = 64 gates per wave, B = 256 per workgroup), the named cells first and from 128 gates on every chosen cell at the first
    job, at the last job and across the middle: every word of the arena — words 0, n - 1 and n (the body) of every row, and every
    slot no job wrote.  The every-digit-0 cell comes out as (0, .., 0, b').  Then a 70-gate batch with MUX gates (two rotation
    rows per key switch) under both kinds."""
    from iyokan_amd import hip

    keys = _carry_keys(request.getfixturevalue("keys" + which))
    p = keys.params
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    em = _emul()
    nc = (((p.n + 1 + 3) & ~3) + 127) // 128
    mat_bytes = em.iyk_emul_ks_matrix_bytes(p.t, nc)
    W, B, min_jobs = em.iyk_emul_ks_matrix_gates(1), em.iyk_emul_ks_matrix_gates(0), em.iyk_emul_ks_matrix_min_jobs()
    cells, nnamed, nspecial, b0 = _cells(p, seed=int(which))
    rng = np.random.default_rng(900 + int(which))
    hip.initialize(keys, device_ids=(0,))
    try:
        st = hip.Stream(0)
        L = hip.lib()
        d_trlwe = ctypes.c_void_p()
        assert L.iyk_hip_trlwe_alloc(0, NCELLS, ctypes.byref(d_trlwe)) == 0
        try:
            assert L.iyk_hip_trlwe_upload(st.h, d_trlwe, NCELLS, 0, NCELLS, cells.ctypes.data_as(_u32p)) == 0
            st.sync()
            bare = hip.resident_key_bytes()
            idx = K.job_layout(min_jobs, list(range(nspecial)), NCELLS, rng)
            got, out_slot = _both(hip, st, d_trlwe.value, idx, p, monkeypatch, (None,), 1)
            assert hip.resident_key_bytes() - bare == mat_bytes
            got.update(_both(hip, st, d_trlwe.value, idx, p, monkeypatch, ("2",), 1)[0])
            _same(got, None, "2", out_slot, p, f"t={p.t} default dispatch, {min_jobs} gates")
            assert hip.resident_key_bytes() - bare == mat_bytes + K.table_bytes(p)

            runs = [np.array([c], dtype=np.int32) for c in range(nnamed)]
            for n in (31, 33, W - 1, W + 1, B - 1, B, B + 1, 2 * B + 1):
                if n >= 128:
                    runs.append(K.job_layout(n, list(range(nspecial)), NCELLS, rng))
                else:
                    idx = rng.integers(0, NCELLS, size=n).astype(np.int32)
                    idx[:nnamed] = np.arange(nnamed)
                    idx[n - nnamed:] = np.arange(nnamed)
                    runs.append(idx)
            for k, idx in enumerate(runs):
                got, out_slot = _both(hip, st, d_trlwe.value, idx, p, monkeypatch, ("3", "1"), 10 + k)
                _same(got, "3", "1", out_slot, p, f"t={p.t} {len(idx)} gates")
                zero = np.nonzero(idx == 0)[0]
                assert len(zero) or len(idx) == 1
                for j in zero:
                    row = got["3"][out_slot[j]]
                    assert not row[:p.n].any() and int(row[p.n]) == b0
            assert hip.resident_key_bytes() - bare == mat_bytes + K.table_bytes(p)

            ng, nin = 70, 16
            ops = np.array([OPS["MUX"], OPS["NAND"], OPS["MUX"], OPS["XOR"], OPS["MUX"]] * (ng // 5), dtype=np.int32)
            in0, in1, in2 = (rng.integers(0, nin, size=ng).astype(np.int32) for _ in range(3))
            in2 = np.where(ops == OPS["MUX"], in2, -1).astype(np.int32)
            out = np.arange(nin, nin + ng, dtype=np.int32)
            host = np.zeros((nin + ng + 3, p.n + 1), dtype=np.uint32)
            host[:nin] = client.encrypt_bits(keys, rng.integers(0, 2, size=nin).astype(np.uint8), seed=5)
            host[nin + ng:] = FILL
            res = {}
            for kind in ("3", "1"):
                monkeypatch.setenv("IYK_HIP_KS_KERNEL", kind)
                arena = hip.Arena(host.shape[0])
                try:
                    st.upload(arena, 0, host)
                    st.gate_batch(arena, ops, in0, in1, in2, out)
                    st.sync()
                    res[kind] = st.download(arena, 0, host.shape[0])
                finally:
                    arena.free()
            assert np.array_equal(res["3"], res["1"]) and (res["3"][nin + ng:] == FILL).all()
            assert (res["3"][nin:nin + ng] != 0).any(axis=1).all()
        finally:
            assert L.iyk_hip_trlwe_free(0, d_trlwe) == 0
            st.destroy()
    finally:
        hip.cleanup()


def test_operand_cap_falls_back_to_the_plan(keys128, monkeypatch):
    """IYK_HIP_KS_MATRIX_MAX_BYTES=0: the operand is never built — a batch that asks for the matrix form (kind 3, and the default at
    KS_MATRIX_MIN_JOBS gates) succeeds with the words of kinds 1 and 2, and the resident key bytes grow by the table of the
    default's fall-back only, never by the operand."""
    from iyokan_amd import hip

    keys = keys128
    p = keys.params
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    em = _emul()
    min_jobs = em.iyk_emul_ks_matrix_min_jobs()
    cells, nnamed, nspecial, _ = _cells(p, seed=11)
    rng = np.random.default_rng(12)
    hip.initialize(keys, device_ids=(0,))
    try:
        st = hip.Stream(0)
        L = hip.lib()
        d_trlwe = ctypes.c_void_p()
        assert L.iyk_hip_trlwe_alloc(0, NCELLS, ctypes.byref(d_trlwe)) == 0
        try:
            assert L.iyk_hip_trlwe_upload(st.h, d_trlwe, NCELLS, 0, NCELLS, cells.ctypes.data_as(_u32p)) == 0
            st.sync()
            bare = hip.resident_key_bytes()
            monkeypatch.setenv("IYK_HIP_KS_MATRIX_MAX_BYTES", "0")
            idx = K.job_layout(300, list(range(nspecial)), NCELLS, rng)
            got, out_slot = _both(hip, st, d_trlwe.value, idx, p, monkeypatch, ("3", "1"), 3)
            _same(got, "3", "1", out_slot, p, "capped operand, 300 gates")
            assert hip.resident_key_bytes() == bare
            idx = K.job_layout(min_jobs, list(range(nspecial)), NCELLS, rng)
            got, out_slot = _both(hip, st, d_trlwe.value, idx, p, monkeypatch, (None, "2"), 4)
            _same(got, None, "2", out_slot, p, f"capped operand, default dispatch, {min_jobs} gates")
            assert hip.resident_key_bytes() == bare + K.table_bytes(p)
        finally:
            assert L.iyk_hip_trlwe_free(0, d_trlwe) == 0
            st.destroy()
    finally:
        hip.cleanup()
