"""CPU: the many-digit form of the lvl0 -> lvl2 rotation.  The emulation of the three kernel forms — the kernels' own
prologue, step and epilogue functions, lane by lane — against the numpy restatement tests/cb_many_ref.py word for word, the restatement
itself against a real key, and the argument checks of the two new entry points (csrc/batch_args.hpp) through libiyk_emul.so."""
import ctypes

import numpy as np
import pytest

import cb_many_cases as mc
import cb_many_ref as many
import cb_rotate_edge_cases as edge
import cb_rotate_ref as ref

N2 = ref.N2
INVALID = -1


# ---- the restatement's own pieces ---------------------------------------------------------------------------------------------------------
def test_grid_reaches_the_edges_it_names():
    for l in (3, 2):
        bw = many.bw_of(l)
        arena, jobs, _ = mc.grid_case(l)
        abar, _ = many.modswitch(ref.linear(arena[mc.GRID_SLOTS // 2], 1, 0), bw)
        assert list(abar[:3]) == [0, 1 << bw, 0]
        assert mc.grid_bbars(l) == [0, N2 - (1 << bw), N2, 2 * N2 - (1 << bw)]
        # an input on which the per-digit abar is no multiple of 2^bw, and the coarser one differs from it
        old = ref.modswitch(ref.linear(arena[mc.GRID_SLOTS // 2], 1, 0))[0]
        assert old[3] % (1 << bw) != 0 and abar[3] != old[3]
        assert {s for _, s, _ in jobs} == {1, -1} and len({o for _, _, o in jobs[4:]}) == 3 and {i for i, _, _ in jobs} == {0, 3, 6}


def test_l1_restatement_is_the_per_digit_restatement():
    arena, jobs, mu = mc.l1_case()
    i, s, off = jobs[1]
    assert np.array_equal(many.rotate_job(arena[i], s, off, mu, mc.grid_key()), mc.l1_expected()[1])


@pytest.mark.parametrize("l", [3, 2])
def test_real_key_every_output_decrypts(l):
    """the check that the definition is right, not just self-consistent: 2 mu_r for a positive phase, 0 for a negative one"""
    bound = edge.decrypt_bound(mc.GRID_N)
    errs = mc.real_errors(l, mc.real_expected(l))
    print("largest |error| / bound:", max(abs(e) for row in errs for e in row) / bound)
    assert all(abs(e) <= bound for row in errs for e in row), errs
    assert bound < min(mc.MUS[l]) / 2


# ---- the emulation of the three forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
def test_l1_is_per_digit(form):
    arena, jobs, mu = mc.l1_case()
    got = mc.rotate_jobs(form, arena, jobs, mu, edge.device_key("mid", form))
    assert np.array_equal(got, mc.l1_expected())
    # and the per-digit emulation's words
    per = edge.rotate_jobs(form, arena, [j + (mu[0],) for j in jobs], edge.device_key("mid", form))
    assert np.array_equal(got[:, 0], per)


@pytest.mark.parametrize("l", [3, 2])
@pytest.mark.parametrize("form", mc.FORMS)
def test_grid_n19(form, l):
    arena, jobs, mu = mc.grid_case(l)
    got = mc.rotate_jobs(form, arena, jobs, mu, edge.device_key("mid", form))
    want = mc.grid_expected(l)
    bad = [(g, r) for g in range(len(jobs)) for r in range(l) if not np.array_equal(got[g, r], want[g, r])]
    assert not bad, bad


@pytest.mark.parametrize("lanes", [256, 512])
def test_extract(lanes):
    acc, mu = mc.extract_case()
    for l in (1, 2, 3, 4):
        got = mc.extract(acc, lanes, mu[:l])
        for r in range(l):
            want = many.extract(acc, r, mu[r])
            assert np.array_equal(got[r], want), (l, r)
            assert got[r, r] == acc[0, 0] and got[r, r + 1] == (-int(acc[0, N2 - 1])) % (1 << 64)   # the sign flips at i = r + 1


@pytest.mark.parametrize("form", mc.FORMS)
def test_real_key_emulation_is_the_restatement(form):
    _, bk, ct, jobs = mc.real_case()
    edge.KEYS.setdefault("many-real", lambda: bk)
    got = mc.rotate_jobs(form, ct, [j[:3] for j in jobs], mc.MUS[3], edge.device_key("many-real", form))
    assert np.array_equal(got, mc.real_expected(3))


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
R = dict(tlwe0_slots=8, tlwe2_slots=12, count=2, in_=[0, 7], sign=[1, -1], off=[0, 0x9E3779B9], l=3, mu=mc.MUS[3], out=[0, 9])


def _rot(**over):
    return mc.rotate_many_args(**dict(R, **over))


def test_rotate_args_legal_at_the_limits():
    code, text, words, counts = _rot()
    assert (code, text) == (0, "") and list(counts[:2]) == [2, 1]
    assert list(words[:8]) == [0, 1, 0, 0, 7, 0xFFFFFFFF, 0x9E3779B9, 9]                 # CbManyJob{in, sign, off, out}
    shared = words[8:18].view(np.uint64)
    assert list(shared[:4]) == mc.MUS[3] + [0] and list(words[16:18]) == [3, 2]        # CbManyMu{mu0 .. mu3, l, bw}
    for l, bw in ((1, 0), (2, 1), (4, 2)):
        code, _, words, _ = _rot(l=l, mu=mc.MUS[l], out=[0, 12 - l])
        assert code == 0 and list(words[16:18]) == [l, bw]
    assert _rot(out=[3, 0])[0] == 0 and _rot(out=[6, 9])[0] == 0                         # ranges that touch


@pytest.mark.parametrize("over, text", [
    (dict(l=0), "l outside [1, 4]"),
    (dict(l=5, mu=[1, 2, 3, 4, 5]), "l outside [1, 4]"),
    (dict(out=[0, 10]), "l TLWEs from out do not fit the lvl2 store"),
    (dict(out=[-1, 9]), "l TLWEs from out do not fit the lvl2 store"),
    (dict(out=[0, 2]), "two jobs of one batch write the same lvl2 TLWE"),
    (dict(out=[5, 3]), "two jobs of one batch write the same lvl2 TLWE"),
    (dict(out=[4, 4]), "two jobs of one batch write the same lvl2 TLWE"),
    (dict(in_=[0, 8]), "TLWE index outside the lvl0 store"),
    (dict(in_=[-1, 0]), "TLWE index outside the lvl0 store"),
    (dict(sign=[1, 0]), "sign outside {+1, -1}"),
    (dict(sign=[2, 1]), "sign outside {+1, -1}"),
    (dict(count=(1 << 20) + 1), "batch too large"),
    (dict(tlwe2_slots=(1 << 28) + 1), "store larger than an allocation can be"),
    (dict(count=(1 << 20) + 1, l=0), "batch too large"),
])
def test_rotate_args_refusals(over, text):
    code, got, _, counts = _rot(**over)
    assert (code, got) == (INVALID, text) and not counts.any()


def _params():
    from iyokan_amd.params import params_128bit

    return params_128bit()   # the ctypes iyk_params itself


C = dict(bk2_n=636, privks_n_in=2048, tlwe0_slots=8, in_=[1, 5], sign=[1, -1], tlwe2_n_in=2048, tlwe2_slots=10, tlwe2_first=4, trlwe_slots=12,
         trgsw_slots=5, trgsw_first=3, bits=2)


def _cb(**over):
    return mc.circuit_bootstrap_many_args(_params(), **dict(C, **over))


def test_circuit_bootstrap_args_legal_at_the_limits():
    code, text, words, counts = _cb()
    assert (code, text) == (0, "") and list(counts[:5]) == [2, 1, 12, 12, 2]
    assert list(words[:8]) == [1, 1, 0, 4, 5, 0xFFFFFFFF, 0, 7]                         # one rotation per bit, out = first + bit l
    assert list(words[8:16].view(np.uint64)) == mc.MUS[3] + [0] and list(words[16:18]) == [3, 2]
    privks = words[18:18 + 36].reshape(12, 3)                                            # PrivksJob{in, c, out}: the per-digit call's
    assert [list(r) for r in privks] == [[4 + b * 3 + r, c, (b * 2 + c) * 3 + r] for b in range(2) for c in range(2) for r in range(3)]
    assert list(words[54:66]) == list(range(12)) and list(words[66:68]) == [3, 4]


@pytest.mark.parametrize("over, text", [
    (dict(bits=(1 << 20) // 6 + 1), "batch too large"),
    (dict(bk2_n=500), "the lvl2 bootstrapping key's n is not the initialised n of the lvl0 store's rows"),
    (dict(tlwe2_n_in=1024), "the lvl2 store's n_in is not the 2048 the rotation writes"),
    (dict(privks_n_in=1024), "the lvl2 store's n_in is not the private key-switching key's"),
    (dict(tlwe2_first=5), "bits * l lvl2 slots from the first do not fit the lvl2 store"),
    (dict(trlwe_slots=11), "the TRLWE scratch store has fewer than bits (k+1) l rows"),
    (dict(trgsw_first=4), "selector slots outside the selector store"),
    (dict(in_=[1, 8]), "TLWE index outside the lvl0 store"),
    (dict(sign=[1, 3]), "sign outside {+1, -1}"),
    (dict(tlwe0_slots=(1 << 28) + 1), "store larger than an allocation can be"),
])
def test_circuit_bootstrap_args_refusals(over, text):
    code, got, _, counts = _cb(**over)
    assert (code, got) == (INVALID, text) and not counts.any()
