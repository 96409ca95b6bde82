"""The throughput rotation kernel forms the rotated difference (X^abar - 1) acc of BOTH accumulator polynomials in one pass
(csrc/blind_rotate_fft.hpp::diff16_pair): the rotated byte index, the wrapped LDS address and the sign mask of a coefficient do not
depend on the polynomial, and the two polynomials of a wave lie 4 096 bytes apart, so one address register and one two-word read
serve both.  No arithmetic on a value changes, so every check here is an equality.

CPU: the host path of diff16_pair and the host restatement of the device path's byte arithmetic (diff16_pair_device_order: byte
index, 0xFFC wrap, bit 12 as the sign, polynomial b at +4 096 bytes) against two calls of diff16 and against numpy, on an
accumulator whose word is a function of (polynomial, index).
GPU: blind_rotate_fft_kernel against the oracle word for word at 1 and 9 rotations (9 = a second workgroup whose seven idle waves
recompute job njobs - 1), sample extract and raw TRLWE output, both parameter sets (l = 3 and l = 2: polynomial b's digits take
over at another row), on seeded encryptions and on one hand-made input per set whose steps run through the edge rotations."""
import ctypes
import os

import numpy as np
import pytest

from iyokan_amd import client

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
# wrap of the address (idx & 0xFFC), the sign bit (bit 12 of the byte index), the lane boundary at abar mod 64, abar = 0 (no difference)
EDGE_ABAR = (0, 1, 63, 64, 65, 511, 512, 1023, 1024, 1025, 1087, 2047)
GADGET = {"128": (0, 3, 6), "80": (1, 2, 10)}   # emulation set index, l, Bgbit
TWO_CALLS, PAIR_HOST, PAIR_DEVICE_ORDER = 0, 1, 2
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _emul():
    em = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    em.iyk_emul_diff16_pair.restype = ctypes.c_int
    em.iyk_emul_diff16_pair.argtypes = [ctypes.c_int, ctypes.c_uint32, _u32p, ctypes.c_int, _u32p]
    return em


def _accumulator():
    """acc[c][j]: an odd multiple of a (polynomial, index) counter — a bijection of it, so no two of the 2 048 words are equal, and the
    two polynomials differ at every index."""
    j = np.arange(N, dtype=np.uint64)
    acc = np.stack([((c * N + j) * 2 + 1) * 0x9E3779B1 & 0xFFFFFFFF for c in (0, 1)]).astype(np.uint32)
    assert len(np.unique(acc)) == 2 * N and np.all(acc[0] != acc[1])
    return acc


def _numpy_diff(acc, abar, l, bgbit):
    """u[c][lane][q] = prepare(((X^abar - 1) acc_c)[lane + 64 q]) from the definition: negacyclic rotation, gadget offset, flipped sign bits."""
    x = np.arange(N, dtype=np.int64)
    src = (x - abar) % (2 * N)
    rot = np.where(src >= N, (0 - acc[:, src % N].astype(np.int64)), acc[:, src % N].astype(np.int64))
    td = (rot - acc.astype(np.int64)) & 0xFFFFFFFF
    half = 1 << (bgbit - 1)
    offset = sum(half << (32 - j * bgbit) for j in range(1, l + 1)) + (1 << (32 - l * bgbit - 1))
    flip = sum(half << (32 - j * bgbit) for j in range(1, l + 1))
    u = ((td + offset) & 0xFFFFFFFF) ^ flip
    return u.astype(np.uint32).reshape(2, 16, 64).transpose(0, 2, 1)   # [c][q][lane] -> [c][lane][q]


@pytest.mark.parametrize("which", ["128", "80"])
def test_pair_equals_two_calls_on_the_host(which):
    em = _emul()
    set_, l, bgbit = GADGET[which]
    acc = np.ascontiguousarray(_accumulator())
    for abar in EDGE_ABAR:
        out = {}
        for form in (TWO_CALLS, PAIR_HOST, PAIR_DEVICE_ORDER):
            out[form] = np.zeros((2, 64, 16), dtype=np.uint32)
            assert em.iyk_emul_diff16_pair(set_, abar, acc.ctypes.data_as(_u32p), form, out[form].ctypes.data_as(_u32p)) == 0
        want = _numpy_diff(acc, abar, l, bgbit)
        assert np.array_equal(out[TWO_CALLS], want), f"diff16 itself, abar {abar}"
        assert np.array_equal(out[PAIR_HOST], out[TWO_CALLS]), f"host path, abar {abar}"
        assert np.array_equal(out[PAIR_DEVICE_ORDER], out[TWO_CALLS]), f"device-order byte arithmetic, abar {abar}"
        if abar == 0:   # the difference is zero: every word is the prepared zero
            assert len(np.unique(want)) == 1


@pytest.mark.parametrize("which", ["128", "80"])
def test_emulated_rotation_with_the_pair_equals_the_oracle(which, request):
    """The host emulation of the kernel (emul.cpp::blind_rotate_fft calls diff16_pair once per step, as the kernel does) on the
    hand-made edge input: the oracle's words."""
    em = _emul()
    keys, orc = request.getfixturevalue("keys" + which), request.getfixturevalue("oracle" + which)
    p = keys.params
    dp = ctypes.POINTER(ctypes.c_double)
    bk = np.zeros(p.bk_words * 2, dtype=np.float64)
    assert em.iyk_emul_bk_fft(ctypes.byref(p), keys.bk.ctypes.data_as(_u32p), bk.ctypes.data_as(dp)) == 0
    lin = _edge_input(p)
    got = np.zeros(p.N + 1, dtype=np.uint32)
    assert em.iyk_emul_blind_rotate_fft(ctypes.byref(p), lin.ctypes.data_as(_u32p), bk.ctypes.data_as(dp), got.ctypes.data_as(_u32p)) == 0
    assert np.array_equal(got, orc.bootstrap_lvl1(lin))


def _edge_input(p, shift=0):
    """A mod-switched input whose steps run through EDGE_ABAR (cyclically, starting at `shift`): word = abar << 21 is rounded back to
    abar by the mod switch; b's word rotates the test vector by an odd amount."""
    lin = np.zeros(p.n + 1, dtype=np.uint32)
    for i in range(p.n):
        lin[i] = (EDGE_ABAR[(i + shift) % len(EDGE_ABAR)] << 21) & 0xFFFFFFFF
    lin[p.n] = (389 + 2 * shift) << 21
    return lin


_inputs_cache = {}


def _inputs(which, keys, orc):
    """Nine inputs per set — eight sums of two seeded encryptions as a NAND forms them (the existing parity tests' inputs) and, LAST, the
    hand-made edge vector (row 8 is the job the idle waves of the second workgroup recompute) — with the oracle's raw accumulators.
    Computed once, shared, read-only."""
    if which not in _inputs_cache:
        import ram_ref

        p = keys.params
        cts = client.encrypt_bits(keys, np.random.default_rng(16).integers(0, 2, size=16).astype(np.uint8), seed=1616)
        lins = np.zeros((9, p.n + 1), dtype=np.uint32)
        for j in range(8):
            lins[j] = (np.uint32(0) - cts[j] - cts[8 + j]).astype(np.uint32)
            lins[j, p.n] = (int(lins[j, p.n]) + int(p.mu)) & 0xFFFFFFFF
        lins[8] = _edge_input(p)
        trlwe = np.stack(ram_ref.blind_rotate_many(orc, lins))
        for a in (lins, trlwe):
            a.setflags(write=False)
        _inputs_cache[which] = (lins, trlwe)
    return _inputs_cache[which]


def _sample_extract0(trlwe):
    out = np.zeros((trlwe.shape[0], N + 1), dtype=np.uint32)
    out[:, 0] = trlwe[:, 0]
    out[:, 1:N] = (np.uint32(0) - trlwe[:, N - 1:0:-1]).astype(np.uint32)
    out[:, N] = trlwe[:, N]
    return out


@pytest.fixture
def fft_env(monkeypatch):
    for v in ("IYK_HIP_DECOMP", "IYK_HIP_LATENCY_KERNEL", "IYK_HIP_KS_KERNEL", "IYK_HIP_KS_SHARED_MAX", "IYK_HIP_KS_SHARED_WG",
              "IYK_HIP_DEBUG", "IYK_HIP_COALESCE"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("IYK_HIP_NTT", "fft")
    monkeypatch.setenv("IYK_HIP_ROT_KERNEL", "fft")   # the wave-per-rotation kernel: the size-based dispatch would take the narrow one
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize("trlwe_mode", [False, True], ids=["extract", "trlwe"])
@pytest.mark.parametrize("rotations", [1, 9])
@pytest.mark.parametrize("which", ["128", "80"])
def test_rotation_words_equal_the_oracle(which, rotations, trlwe_mode, request, fft_env):
    import torch

    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + which)
    lins, trlwe = _inputs(which, keys, request.getfixturevalue("oracle" + which))
    rows = [8] if rotations == 1 else list(range(9))   # one rotation: the edge vector
    want = trlwe[rows] if trlwe_mode else _sample_extract0(trlwe[rows])
    hip.initialize(keys, device_ids=(0,))
    try:
        assert hip.ntt_path() == "fft"
        st = hip.Stream(0)
        arena = hip.Arena(len(rows))
        try:
            st.upload(arena, 0, np.ascontiguousarray(lins[rows]))
            out = torch.zeros(want.shape, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ia, none, one, zero = np.arange(len(rows)), [-1] * len(rows), [1] * len(rows), [0] * len(rows)
            if trlwe_mode:
                st.bootstrap_trlwe_batch(arena, ia, none, one, zero, np.zeros(len(rows), dtype=np.uint32), out.data_ptr())
            else:
                st.blind_rotate_batch(arena, ia, none, one, zero, np.zeros(len(rows), dtype=np.uint32), out.data_ptr())
            st.sync()
            got = out.cpu().numpy().view(np.uint32)
        finally:
            arena.free()
            st.destroy()
    finally:
        hip.cleanup()
    assert np.array_equal(got, want)
