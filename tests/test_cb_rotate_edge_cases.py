"""CPU: the edge cases of tests/cb_rotate_edge_cases.py through the emulation of the three forms of the lvl0 -> lvl2 rotation
(iyk_emul_cb_rotate, iyk_emul_cb_rotate_lat, iyk_emul_cb_rotate_fft).  The GPU test (tests/test_gpu_cb_rotate_edges.py) holds the
kernels to the emulation at the sizes the numpy restatement is too slow for, so the emulation is held to the restatement here first:
at n = 19 on every job and at n = 257 (a second pass over the row of the 256-lane form) on one; the three emulations are compared with
one another on every job of `row-pass`; and the full-size outputs decrypt inside the derived bound before any kernel is asked to."""
import math

import numpy as np
import pytest

import cb_rotate_edge_cases as edge
import cb_rotate_ref as ref


@pytest.mark.parametrize("form", edge.FORMS)
def test_mid_n19_against_the_restatement(form):
    arena, jobs = edge.mid_case()
    want = edge.mid_expected()
    got = edge.rotate_jobs(form, arena, jobs, edge.device_key("mid", form))
    for g in range(len(jobs)):
        bad = np.flatnonzero(got[g] != want[g])
        assert bad.size == 0, (form, g, bad[:8])
    assert all((want[g] != want[h]).any() for g in range(len(jobs)) for h in range(g))


def test_case_tables_hold_what_they_promise():
    """A guard on the case TABLES only: it runs none of the code under test"""
    arena, jobs = edge.mid_case()
    assert {(i, s) for i, s, _, _ in jobs} == {(i, s) for i in (0, 3, edge.MID_SLOTS - 1) for s in (1, -1)}
    assert {(off, s) for _, s, off, _ in jobs} == {(off, s) for off in (0, 0x9E3779B9, 0xFFF80000) for s in (1, -1)}
    assert {mu for _, _, _, mu in jobs} >= {ref.mu_of(r, 6) for r in range(3)} | {ref.mu_of(r, 10) for r in range(2)}
    for n in edge.ROW_NS:
        arena, jobs = edge.row_case(n)
        assert arena.shape == (edge.ROW_SLOTS, n + 1) and [(j[0], j[1]) for j in jobs] == [(0, 1), (edge.ROW_SLOTS - 1, -1)]
        assert jobs[1][2] != 0
    assert {n % 256 for n in edge.ROW_NS[:3]} == {255, 0, 1} and {n % 512 for n in edge.ROW_NS[3:]} == {511, 0, 1}
    for cus in (256, 304, 7):
        arena, jobs, slots, which = edge.rounds_case(cus)
        outs = [j[4] for j in jobs]
        assert len(jobs) == cus + 3 and len(set(outs)) == len(jobs) and {0, slots - 1} <= set(outs) and slots == len(jobs) + 2
        assert which[cus:] == [cus % 6, (cus + 1) % 6, (cus + 2) % 6] and set(which) == set(range(6))


def test_n257_against_the_restatement():
    """one job at n = 257 (the last slot, sign = -1, an off): the three emulations give the restatement's words.  One restatement run
    of 257 steps, about 8 s."""
    arena, jobs = edge.row_case(257)
    i, sign, off, mu = jobs[1]
    want = ref.rotate_job(arena[i], sign, off, mu, edge.row_key()[:257])
    for form in edge.FORMS:
        bad = np.flatnonzero(edge.row_expected(form)[257][1] != want)
        assert bad.size == 0, (form, bad[:8])
    assert want.any()


def test_row_pass_three_forms_agree():
    got = {form: edge.row_expected(form) for form in edge.FORMS}
    for n in edge.ROW_NS:
        for form in ("lat", "fft"):
            assert np.array_equal(got["wg"][n], got[form][n]), (n, form)
        assert (got["wg"][n][0] != got["wg"][n][1]).any()
    # a key one step longer is another rotation: no two sizes share an output
    flat = [got["wg"][n][g] for n in edge.ROW_NS for g in range(2)]
    assert all((flat[a] != flat[b]).any() for a in range(len(flat)) for b in range(a))


@pytest.mark.parametrize("name", ["128", "80"])
def test_full_size_decrypts_inside_the_derived_bound(name, request):
    """n = 636 / 500 under a real key.  The derived bound clears mu_r / 2 for every r of the set (otherwise the decryption assertion of
    the GPU test would say nothing); the words of two jobs (the smallest mu_r on the 1 bit and on the 0 bit) are the same from the three
    emulations and decrypt inside the bound; and so do all off = 0 jobs through the FP64 form's emulation, the one fast enough to run
    them all here.  The worst error is printed."""
    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    l = int(p.l)
    s2, bk, arena, jobs, bits = edge.full_case(name, keys)
    bound = edge.decrypt_bound(p.n)
    for r in range(l):
        assert bound < ref.mu_of(r, int(p.Bgbit)) / 2, (name, r)
    assert len(jobs) == 4 * l + 1 and [j[2] != 0 for j in jobs] == [False] * (4 * l) + [True]
    two = (l - 1, 3 * l - 1)
    assert [(bits[g], jobs[g][1], jobs[g][3]) for g in two] == [(b, 1, ref.mu_of(l - 1, int(p.Bgbit))) for b in (1, 0)]
    words = {form: edge.full_expected(name, form, two) for form in edge.FORMS}
    assert np.array_equal(words["wg"], words["lat"]) and np.array_equal(words["wg"], words["fft"])
    errs = edge.phase_errors(s2, words["wg"], [jobs[g] for g in two], [bits[g] for g in two])
    assert max(map(abs, errs)) < bound, (name, errs, bound)
    every = edge.full_expected(name, "fft")
    assert np.array_equal(every[list(two)], words["fft"])
    errs = edge.phase_errors(s2, every[:4 * l], jobs[:4 * l], bits[:4 * l])
    worst = max(map(abs, errs))
    print(f"set {name}: worst |phase error| of {4 * l} rotations 2^{math.log2(max(worst, 1)):.2f}, bound 2^{math.log2(bound):.2f}, "
          f"smallest mu_r / 2 2^{math.log2(ref.mu_of(l - 1, int(p.Bgbit)) / 2):.0f}")
    assert worst < bound, (name, errs, bound)
