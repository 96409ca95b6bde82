"""The paired inverse transform of the throughput rotation kernel (csrc/kernels_fft.hpp::fft_inverse2) fetches the lane's conjugated
T2 and T1 twiddle columns once per pair of halves instead of once per half.  The arithmetic is the parent's, operation for
operation, so every check here is an equality: output words against the CPU oracle, the CHECK instantiation's worst rounding
distance against the parent build's to the bit, and the host restatement of the pair against two single inverses bit for bit.

Shapes: 1 gate = one live wave beside seven idle ones (they recompute the job and discard), 8 gates = one full workgroup, 9 gates =
a second workgroup with seven recomputed waves — the smallest at which a register shared wrongly between the halves, or a read
taken before the exchange has landed, shows."""
import ctypes
import os

import numpy as np
import pytest

from iyokan_amd import client
from iyokan_amd.params import OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# iyk_hip_fft_round_error after the 9-gate batch below with IYK_HIP_DEBUG=1, measured on the PARENT of the change (commit c96d6d4,
# build id fcd7c08d62b0e3cf, one MI355X; the kernel takes the maximum over all waves, idle ones included, so the value does not
# depend on scheduling).  float.hex() of the double the library returned.
PARENT_WORST = {"128": "0x1.4000000000000p-24", "80": "0x1.a000000000000p-21"}

_ref_cache = {}


def nand_batch(keys, gates):
    """`gates` NANDs on 2 * gates fresh encryptions: arena rows [0, 2 g) inputs, [2 g, 3 g) outputs."""
    p = keys.params
    bits = np.random.default_rng(1000 + gates).integers(0, 2, size=2 * gates).astype(np.uint8)
    host = np.zeros((3 * gates, p.n + 1), dtype=np.uint32)
    host[:2 * gates] = client.encrypt_bits(keys, bits, seed=500 + gates)
    ops = np.full(gates, OPS["NAND"], dtype=np.int32)
    in0 = np.arange(gates, dtype=np.int32)
    in1 = np.arange(gates, 2 * gates, dtype=np.int32)
    in2 = np.full(gates, -1, dtype=np.int32)
    out = np.arange(2 * gates, 3 * gates, dtype=np.int32)
    return bits, host, (ops, in0, in1, in2, out)


def run_batch(hip, host, job):
    st = hip.Stream(0)
    arena = hip.Arena(host.shape[0])
    st.upload(arena, 0, host)
    st.gate_batch(arena, *job)
    st.sync()
    got = st.download(arena, 0, host.shape[0])
    arena.free()
    st.destroy()
    return got


def _reference(which, gates, keys, orc):
    """The oracle's arena for (set, gates): computed once, shared by the tests, never written to."""
    if (which, gates) not in _ref_cache:
        bits, host, job = nand_batch(keys, gates)
        ref = host.copy()
        orc.gate_batch(*job, ref, nthreads=min(gates, os.cpu_count() or 1))
        ref.setflags(write=False)
        _ref_cache[(which, gates)] = (bits, host, job, ref)
    return _ref_cache[(which, gates)]


@pytest.fixture
def fft_env(monkeypatch):
    for v in ("IYK_HIP_DECOMP", "IYK_HIP_LATENCY_KERNEL", "IYK_HIP_KS_KERNEL", "IYK_HIP_KS_SHARED_MAX", "IYK_HIP_KS_SHARED_WG",
              "IYK_HIP_DEBUG", "IYK_HIP_COALESCE"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("IYK_HIP_NTT", "fft")
    monkeypatch.setenv("IYK_HIP_ROT_KERNEL", "fft")   # the wave-per-rotation kernel: the size-based dispatch would take the narrow one
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize("gates", [1, 8, 9])
@pytest.mark.parametrize("which", ["128", "80"])
def test_nand_words_equal_the_oracle(which, gates, request, fft_env):
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + which)
    bits, host, job, ref = _reference(which, gates, keys, request.getfixturevalue("oracle" + which))
    hip.initialize(keys, device_ids=(0,))
    try:
        assert hip.ntt_path() == "fft"
        got = run_batch(hip, host, job)
    finally:
        hip.cleanup()
    assert np.array_equal(got, ref)
    assert np.array_equal(client.decrypt_bits(keys, got[2 * gates:]), 1 - (bits[:gates] & bits[gates:]))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["128", "80"])
def test_check_build_reports_the_parents_rounding_distance(which, request, fft_env):
    """The 9-gate batch through blind_rotate_fft_kernel<G, true> (IYK_HIP_DEBUG=1 at init).  Sharing the twiddle registers changes
    no operand and no order of operations, so max |z - rint(z)| over every inverse-transform output is the parent's to the bit.
    PARENT_WORST: measured with the parent commit's library on one MI355X, this batch, this environment (see the constant)."""
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + which)
    bits, host, job, ref = _reference(which, 9, keys, request.getfixturevalue("oracle" + which))
    fft_env.setenv("IYK_HIP_DEBUG", "1")
    hip.initialize(keys, device_ids=(0,))
    try:
        got = run_batch(hip, host, job)
        err = hip.fft_round_error(0)
    finally:
        hip.cleanup()
    print(f"worst rounding distance, {which}-bit set, 9 gates: {err!r} = {float(err).hex()} (parent {PARENT_WORST[which]})")
    assert np.array_equal(got, ref)
    assert float(err).hex() == PARENT_WORST[which]


@pytest.mark.parametrize("scale_bits", [0, 17])
def test_host_pair_equals_two_single_inverses(scale_bits):
    """The host restatement of fft_inverse2 (emul.cpp::fft_inverse2_wave: both halves through one exchange buffer in the kernel's issue
    order, twiddle columns fetched once) against two fft_inverse1_wave calls on random spectra of 16-bit integers (times 2^17: the
    size of a step's sums): every output double has the same bit pattern."""
    em = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    em.iyk_emul_fft_inverse2_selftest.restype = ctypes.c_int
    for seed in range(8):
        assert em.iyk_emul_fft_inverse2_selftest(seed, scale_bits) == 0
