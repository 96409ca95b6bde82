"""CPU: the chosen key-switch words of tests/ks_words.py do what tests/test_gpu_keyswitch.py relies on — the cover family selects every
row of the pair table, the TRLWE images extract to the intended TLWE1 words, the table restatement equals the oracle on the edge
families, and the case list reaches every launch shape of the three key-switch kernels."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import ks_words as K
import numpy_tfhe as T
from iyokan_amd.params import params_128bit, params_80bit

SETS = {"128": params_128bit, "80": params_80bit}


@pytest.mark.parametrize("which", ["128", "80"])
def test_cover_family_selects_every_pair_table_row(which):
    """Digits decoded as orc_keyswitch decodes them ((a' + prec) >> (32 - 2 (j + 1))) & 3, paired as keyswitch_lut_kernel pairs them:
    the 16 cover cells select all N x rows_per_i rows, the zero row of every stage included; the lbits variants select the same rows."""
    p = SETS[which]()
    fam = K.chosen_t1(p)
    rpi = K.rows_per_i(p.t)
    for cells in (fam["cover"], fam["lbits"][0:16], fam["lbits"][16:32], fam["lbits"][32:48], fam["lbits"][48:64]):
        hit = np.zeros((p.N, rpi), dtype=bool)
        for w in cells:
            for rows in K.table_rows_selected(w[:p.N], p.t):
                hit[np.arange(p.N), rows] = True
        assert hit.all()
    # every KSK row (i, j, v) of the digit-by-digit kernels too (v = 0: no row)
    seen = np.zeros((p.N, p.t, 4), dtype=bool)
    for w in fam["cover"]:
        for j, d in enumerate(K.digit_list(w[:p.N], p.t)):
            seen[np.arange(p.N), j, d] = True
    assert seen.all()


@pytest.mark.parametrize("which", ["128", "80"])
def test_digit_and_low_bit_construction(which):
    """a' + prec carries exactly D above L; the carry wrap, every-0 and every-3 edges decode as intended; L takes its extremes."""
    p = SETS[which]()
    t, low = p.t, 1 << (32 - 2 * p.t)
    rng = np.random.default_rng(5)
    D = rng.integers(0, 1 << (2 * t), size=4096)
    L = rng.integers(0, low, size=4096, dtype=np.uint64)
    D[:4], L[:4] = [0, 0, (1 << 2 * t) - 1, (1 << 2 * t) - 1], [0, low - 1, 0, low - 1]
    w = K.words_from_digits(D, L, t)
    assert np.array_equal(K.digits_of(w, t), D)
    assert np.array_equal((w.astype(np.uint64) + K.prec_of(t)) & np.uint64(low - 1), L)
    fam = K.chosen_t1(p)
    e = [x[:p.N] for x in fam["edges"]]
    assert not K.digits_of(e[0], t).any() and (K.digits_of(e[1], t) == (1 << 2 * t) - 1).all()
    assert not K.digits_of(e[2], t).any() and (e[2] >= np.uint32((1 << 32) - K.prec_of(t))).all()   # wraps past 2^32 to D = 0
    assert (K.digits_of(e[3], t) == (1 << 2 * t) - 1).all()
    lows = [(x[:p.N].astype(np.uint64) + K.prec_of(t)) & np.uint64(low - 1) for x in fam["lbits"][::16]]
    assert [set(v.tolist()) for v in lows] == [{0}, {low - 1}, {K.prec_of(t) - 1}, {K.prec_of(t) + 1}]
    assert {int(x[p.N]) for x in fam["cover"]} >= {0, K.MASK32}


@pytest.mark.parametrize("which", ["128", "80"])
def test_images_extract_to_the_intended_words(which, request):
    """orc_sample_extract0 of every chosen image is the TLWE1 it was built from; b[1 .. N - 1] is ignored."""
    import oracle_lib

    keys = request.getfixturevalue("keys" + which)
    orc = request.getfixturevalue("oracle" + which)
    p = keys.params
    imgs, names = K.chosen_images(p)
    fam = K.chosen_t1(p)
    want = fam["cover"] + fam["edges"] + fam["lbits"]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert names.count("raw") == len(imgs) - len(want)
    for c, img in enumerate(imgs):
        img = np.ascontiguousarray(img)
        t1 = np.zeros(p.N + 1, dtype=np.uint32)
        oracle_lib.lib().orc_sample_extract0(orc.ctx, img.ctypes.data_as(u32p), t1.ctypes.data_as(u32p))
        assert np.array_equal(t1, K.t1_from_image(img, p.N))
        if c < len(want):
            assert np.array_equal(t1, want[c])
        other = img.copy()
        other[p.N + 1:] ^= np.uint32(0x5A5A5A5A)
        assert np.array_equal(K.t1_from_image(other, p.N), t1)


@pytest.mark.slow
@pytest.mark.parametrize("which", ["128", "80"])
def test_table_restatement_equals_oracle_on_edge_families(which, request):
    """numpy_tfhe.keyswitch_by_table (the table kernel's arithmetic) equals orc_keyswitch word for word on the edges, the L extremes of
    two cover cells, the raw words and one cover cell."""
    keys = request.getfixturevalue("keys" + which)
    orc = request.getfixturevalue("oracle" + which)
    p = keys.params
    table = T.keyswitch_pair_table(keys.ksk, p)
    fam = K.chosen_t1(p)
    imgs, names = K.chosen_images(p)
    words = fam["edges"] + fam["lbits"][0::16] + fam["lbits"][5::16] + [fam["cover"][3]]
    words += [K.t1_from_image(img, p.N) for img, nm in zip(imgs, names) if nm == "raw"]
    for w in words:
        want = orc.keyswitch(w)
        assert np.array_equal(T.keyswitch_by_table(w, table, p), want)
    zero = T.keyswitch_by_table(fam["edges"][0], table, p)
    assert not zero[:p.n].any() and zero[p.n] == fam["edges"][0][p.N]       # every digit 0: no row subtracted


@pytest.mark.parametrize("t", [7, 8])
def test_case_list_reaches_every_launch_shape(t):
    """The cases of tests/test_gpu_keyswitch.py, through the mirror of launch_keyswitch_t / _wave / _lut at 256 CUs: every slice count
    each form can take, and the table form's 8 / 4 / 2 / 1 slices each with a whole and a ragged last workgroup."""
    cases = K.cases(256, t)
    assert K.reached_shapes(cases, t, 256) == K.expected_shapes()
    # the forms and grids the issue's table names (256 CUs)
    g = lambda kind, smax, n: K.ks_geometry(kind, smax, n, t, 256)
    assert g("2", None, 4097) == ("table", 33, 8) and g("2", None, 8192) == ("table", 64, 4)
    assert g("2", None, 16384) == ("table", 128, 2) and g("2", None, 16385) == ("table", 129, 2)
    assert g("2", None, 32768) == ("table", 256, 1) and g("2", None, 32769) == ("table", 257, 1)
    assert g(None, None, 32769) == g("2", None, 32769) and g("x", None, 4097) == ("table", 33, 8)   # unset / other: the default 2
    assert g("2", None, 4096) == ("shared", 256, 2) and g("1", None, 4096) == ("shared", 256, 2)
    assert g("1", None, 1) == ("shared", 1, 256) and g("1", None, 17) == ("shared", 2, 128) and g("1", None, 64) == ("shared", 4, 64)
    assert g("1", None, 4097) == ("wide", 65, 8) and g("1", "0", 1) == ("wide", 1, 256) and g("1", "0", 32769) == ("wide", 513, 1)
    assert g("0", None, 1) == ("kind0", 1, 64) and g("0", None, 8193) == ("kind0", 513, 1)
    assert K.ks_geometry("1", None, 100, 5, 256)[0] == "kind0"       # no wave or table kernel at t = 5
    # more CUs: the table keeps 8 slices longer; the boundary sizes follow
    assert K.reached_shapes(K.cases(304, t), t, 304) >= {s for s in K.expected_shapes() if s[0] == "table"}


def test_geometry_mirror_equals_the_library_dispatch():
    """ks_words.ks_geometry (what the GPU test's case list and its claim "every (form, slices) shape is reached" rest on) is ks_plan
    of csrc/dispatch.hpp — the function iyokan_hip.hip launches by, exported by the test-support library — for every batch size
    1 .. 40 000 at the default IYK_HIP_KS_SHARED_MAX / _WG, and on 1 .. 5 000 (both of their thresholds lie below) at the others."""
    em = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iyokan_amd", "lib", "libiyk_emul.so"))
    ip = ctypes.POINTER(ctypes.c_int)
    em.iyk_emul_ks_plan.argtypes = [ctypes.c_int] * 3 + [ip, ctypes.c_int] + [ctypes.c_int] * 3 + [ip] * 4
    em.iyk_emul_ks_plan.restype = None
    forms = ["kind0", "shared", "wide", "table"]
    unset = lambda v: -1 if v is None else int(v)
    checked = 0
    for kind, smax, swg, t, cus in itertools.product(("0", "1", "2", None), (None, "0", "1000"), (None, "64"), (5, 7, 8), (64, 256, 304)):
        ns = np.arange(1, (40000 if smax is None and swg is None else 5000) + 1, dtype=np.intc)
        out = [np.zeros(len(ns), dtype=np.intc) for _ in range(4)]
        em.iyk_emul_ks_plan(unset(kind), unset(smax), unset(swg), ns.ctypes.data_as(ip), len(ns), t, {7: 5, 8: 4}.get(t, 5), cus,
                            *[o.ctypes.data_as(ip) for o in out])
        form, groups, slices, ips = (o.tolist() for o in out)
        for k, n in enumerate(ns.tolist()):
            got = (forms[form[k]], groups[k], slices[k])
            if got != K.ks_geometry(kind, smax, n, t, cus, swg):
                raise AssertionError((kind, smax, swg, t, cus, n, got, K.ks_geometry(kind, smax, n, t, cus, swg)))
        assert all(i * s == 1024 for i, s in zip(ips, slices))
        checked += len(ns)
    assert checked == 4 * 3 * 3 * (40000 + 5 * 5000)


def test_job_layout_places_the_chosen_cells():
    """Every case of len(special) jobs or more holds all special cells, with special[0] at the first job, special[-1] at the last and a
    16-gate wave boundary inside a copy; shorter cases hold a prefix."""
    rng = np.random.default_rng(1)
    special = list(range(100, 189))
    for n in (1, 17, 64, 65, 89, 90, 129, 1000, 4097, 32769):
        idx = K.job_layout(n, special, 32769, rng)
        assert len(idx) == n and idx.dtype == np.int32 and (idx >= 0).all() and (idx < 32769).all()
        if n >= len(special):
            assert set(special) <= set(idx.tolist()) and idx[0] == special[0] and idx[-1] == special[-1]
            mid = (n // 2) // 16 * 16
            if n >= 4 * len(special):
                assert idx[mid - 1] == special[len(special) // 2 - 1] and idx[mid] == special[len(special) // 2]
        elif n > 1:
            assert list(idx) == special[:n]
