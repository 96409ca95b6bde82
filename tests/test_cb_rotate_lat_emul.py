"""CPU: the latency form of the lvl0 -> lvl2 rotation (csrc/cb_rotate_lat.hpp) run lane by lane by csrc/emul.cpp — its 64-point pass
of two lanes, the N2 = 2048 transform through its unpadded swizzled slot, whole rotation jobs against the numpy restatement
(tests/cb_rotate_ref.py) and against the wide form's emulation, word for word — and dispatch::cb_plan."""
import ctypes
import functools

import numpy as np
import pytest

import cb_rotate_cases as cases
import cb_rotate_ref as ref

P = (1 << 64) - (1 << 32) + 1
_u64p, _u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
_intp = ctypes.POINTER(ctypes.c_int)
AUTO, WG, LAT, UNKNOWN = -1, 0, 1, 2   # dispatch.hpp: CB_KIND_*; the forms are CB_FORM_WG = 0, CB_FORM_LAT = 1


@functools.lru_cache(maxsize=None)
def emul():
    L = cases.emul()
    L.iyk_emul_cb_lat_ntt64.argtypes = [_u64p, ctypes.c_int, _u64p]
    L.iyk_emul_cb_lat_ntt64.restype = None
    L.iyk_emul_cb_lat_ntt.argtypes = [_u64p, ctypes.c_int, _u64p]
    L.iyk_emul_cb_lat_ntt.restype = None
    L.iyk_emul_cb_rotate_lat.argtypes = [ctypes.c_uint32] * 3 + [_u32p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, _u64p, _u64p]
    L.iyk_emul_cb_plan.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, _intp, _intp]
    L.iyk_emul_cb_kind.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.iyk_emul_cb_lat_max_jobs.restype = ctypes.c_uint64
    return L


def emul_rotate_lat(w, sign, off, mu, ntt, l2=cases.L2, bgbit2=cases.BGBIT2):
    w = np.ascontiguousarray(w, dtype=np.uint32)
    out = np.zeros(cases.N2 + 1, dtype=np.uint64)
    rc = emul().iyk_emul_cb_rotate_lat(w.size - 1, l2, bgbit2, w.ctypes.data_as(_u32p), int(sign), int(off) & 0xFFFFFFFF, int(mu) & ref.M64,
                                       ntt.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError(f"iyk_emul_cb_rotate_lat refused its arguments ({rc})")
    return out


def plan(count, cus, kind):
    form, grid = ctypes.c_int(7), ctypes.c_int(7)
    rc = emul().iyk_emul_cb_plan(count, cus, kind, ctypes.byref(form), ctypes.byref(grid))
    return rc, form.value, grid.value


def plan_counts(cus):
    """the widths the default can change at and the launch shapes change at: 1, either side of the threshold, CUs, CUs + 1, 2 CUs + 1"""
    t = int(emul().iyk_emul_cb_lat_max_jobs())
    return sorted({1, max(t - 1, 1), max(t, 1), t + 1, cus, cus + 1, 2 * cus + 1})


def _field(rng, n):
    x = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    x[x >= np.uint64(P)] -= np.uint64(P)
    x[:4] = [0, 1, P - 1, P >> 1]
    return x


@pytest.mark.parametrize("inverse", [0, 1])
def test_two_lane_ntt64_is_the_dft_with_root_8(inverse):
    x = _field(np.random.default_rng(15 + inverse), 64)
    out = np.zeros(64, dtype=np.uint64)
    emul().iyk_emul_cb_lat_ntt64(x.ctypes.data_as(_u64p), inverse, out.ctypes.data_as(_u64p))
    root = pow(8, P - 2, P) if inverse else 8
    want = [sum(int(x[j]) * pow(root, j * k % 64, P) for j in range(64)) % P for k in range(64)]
    assert [int(v) for v in out] == want
    old = np.zeros(64, dtype=np.uint64)
    emul().iyk_emul_ntt64(x.ctypes.data_as(_u64p), inverse, old.ctypes.data_as(_u64p))
    assert np.array_equal(out, old)


def test_n2_transform_against_direct_evaluation_the_wide_form_and_round_trip():
    rng = np.random.default_rng(19)
    x = _field(rng, ref.N2)
    X, Xw, back = (np.zeros(ref.N2, dtype=np.uint64) for _ in range(3))
    psi = ctypes.c_uint64()
    emul().iyk_emul_cb_lat_ntt(x.ctypes.data_as(_u64p), 0, X.ctypes.data_as(_u64p))
    emul().iyk_emul_cb_ntt(x.ctypes.data_as(_u64p), 0, Xw.ctypes.data_as(_u64p), ctypes.byref(psi))
    psi = psi.value
    pw = [1] * 4096
    for e in range(1, 4096):
        pw[e] = pw[e - 1] * psi % P
    xs = [int(v) for v in x]
    for k in list(range(0, 2048, 61)) + [1, 31, 32, 33, 63, 64, 65, 2047]:     # X[k] = sum_j x[j] psi^(j (2k+1)), O(N) each
        assert int(X[k]) == sum(xs[j] * pw[j * (2 * k + 1) % 4096] for j in range(2048)) % P, k
    assert np.array_equal(X, Xw)          # the key's layout: natural order, as bk2_ntt_kernel leaves it
    emul().iyk_emul_cb_lat_ntt(X.ctypes.data_as(_u64p), 1, back.ctypes.data_as(_u64p))
    assert np.array_equal(back, x)


@pytest.mark.parametrize("name", cases.CASES)
def test_emulated_latency_form_word_for_word(name):
    bk, jobs = cases.case(name)
    ntt = cases.key_ntt(bk)
    want = cases.expected(name)
    for g, (w, sign, off, mu) in enumerate(jobs):
        got = emul_rotate_lat(w, sign, off, mu, ntt)
        bad = np.flatnonzero(got != want[g])
        assert bad.size == 0, (name, g, bad[:8])
        assert np.array_equal(got, cases.emul_rotate(w, sign, off, mu, ntt)), (name, g)
    assert want.any()


def test_refused_arguments():
    bk, jobs = cases.case("uniform-n1")
    ntt = cases.key_ntt(bk)
    w = jobs[0][0]
    for l2, bg, sign in ((3, 9, 1), (4, 10, 1), (4, 9, 0), (4, 9, 2)):
        with pytest.raises(ValueError):
            emul_rotate_lat(w, sign, 0, 1, ntt, l2, bg)


@pytest.mark.parametrize("cus", [256, 304, 7])
def test_cb_plan_forced_forms_and_grid(cus):
    for count in plan_counts(cus):
        for kind in (WG, LAT):
            assert plan(count, cus, kind) == (0, kind, min(count, cus)), (count, kind)


@pytest.mark.parametrize("cus", [256, 7])
def test_cb_plan_default_follows_the_threshold(cus):
    t = int(emul().iyk_emul_cb_lat_max_jobs())
    for count in plan_counts(cus):
        assert plan(count, cus, AUTO) == (0, LAT if count <= t else WG, min(count, cus)), count


def test_cb_plan_refuses_an_unknown_kind():
    for count in (1, 256, 513):
        assert plan(count, 256, UNKNOWN) == (-1, -1, 0)
        assert plan(count, 256, 3) == (-1, -1, 0)


def test_kind_of_the_knob_and_of_a_device_without_the_lds():
    kind = emul().iyk_emul_cb_kind
    assert [kind(None, 1), kind(b"wg", 1), kind(b"lat", 1)] == [AUTO, WG, LAT]
    for text in (b"nonsense", b"", b"WG", b"lat ", b"wgx", b"l", b"1"):
        assert kind(text, 1) == UNKNOWN and kind(text, 0) == UNKNOWN, text
    # not granted: whatever is asked for runs cb_rotate_kernel
    assert [kind(None, 0), kind(b"wg", 0), kind(b"lat", 0)] == [WG, WG, WG]
    for count in plan_counts(256):
        assert plan(count, 256, kind(b"lat", 0)) == (0, WG, min(count, 256))
        assert plan(count, 256, kind(None, 0)) == (0, WG, min(count, 256))
