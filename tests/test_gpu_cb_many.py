"""GPU: the many-digit form of the lvl0 -> lvl2 rotation (iyk_hip_cb_rotate_many_batch, iyk_hip_circuit_bootstrap_many_batch) on each of
the three kernel forms by name — `wg`, `lat` (IYK_HIP_CB_KERNEL) and `fft` (a key of form="fft") — against the numpy restatement
tests/cb_many_ref.py and the emulation, word for word on u64 [l][N2 + 1].  The store is filled with a canary first: the slots no job
writes must come back unchanged.  hip.cb_rotate_form is asserted before every launch of an integer form, with count = the number of
jobs (rotations), as tests/test_gpu_cb_rotate_edges.py does."""
import math

import numpy as np
import pytest

import cb_many_cases as mc
import cb_rotate_edge_cases as edge
import cb_rotate_ref as ref
from iyokan_amd import client, cmux
from test_gpu_cb_rotate import FILL, _arena
from test_gpu_cb_rotate_edges import _assert_form, _key, form, gpu  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N2 = ref.N2
FILL32 = np.uint32(0xA5A5A5A5)
CAP = (1 << 20) + 1   # one more than MAX_CB_BATCH rotations / private key switches of a call


def _run_many(gpu, key, tlwes, jobs, mu, slots, twice=False):
    """jobs (in, sign, off, out) -> the whole store u64 [slots][N2 + 1] after the batch (enqueued twice without a sync where `twice`)"""
    hip, _, st, _, _ = gpu
    arena, store = _arena(gpu, tlwes), hip.Tlwe2(N2, slots)
    try:
        store.upload(st, 0, np.full((slots, N2 + 1), FILL, dtype=np.uint64))
        for _ in range(2 if twice else 1):
            st.cb_rotate_many_batch(key, arena, *zip(*[j[:3] for j in jobs]), mu, store, [j[3] for j in jobs])
        return store.download(st, 0, slots)
    finally:
        store.free()


def _launch_and_compare(gpu, form, key, arena, jobs, mu, want, slots, twice=False):
    """want[g]: u64 [l][N2 + 1] of job g"""
    _assert_form(gpu, form, len(jobs))
    got = _run_many(gpu, key, arena, jobs, mu, slots, twice)
    l, written = len(mu), {}
    for g, job in enumerate(jobs):
        for r in range(l):
            written[job[3] + r] = want[g][r]
    assert len(written) == len(jobs) * l
    for s in range(slots):
        if s in written:
            bad = np.flatnonzero(got[s] != written[s])
            assert bad.size == 0, (form, s, bad[:8])
        else:
            assert (got[s] == FILL).all(), f"slot {s} that no job writes changed"
    return got


def _outs(count, l, blocks, seed):
    """`count` disjoint ranges of l slots of a store of blocks * l slots in a shuffled order, the first and the last range among them"""
    at = np.random.default_rng(seed).permutation(blocks)[:count].tolist()
    for need, where in ((0, 0), (blocks - 1, -1)):
        if need not in at:
            at[where] = need
    assert len(set(at)) == count
    return [a * l for a in at]


@pytest.mark.parametrize("l", [3, 2])
def test_grid_n19(gpu, form, l):
    arena, jobs, mu = mc.grid_case(l)
    blocks = len(jobs) + 2
    slots, out = blocks * l, _outs(len(jobs), l, blocks, seed=19 + l)
    key = _key(gpu, "mid", form, mc.grid_key(), [0, 1, mc.GRID_N])
    _launch_and_compare(gpu, form, key, arena, [j + (out[g],) for g, j in enumerate(jobs)], mu, mc.grid_expected(l), slots)


def test_l1_is_per_digit(gpu, form):
    arena, jobs, mu = mc.l1_case()
    key = _key(gpu, "mid", form, mc.grid_key(), [0, 1, mc.GRID_N])
    _launch_and_compare(gpu, form, key, arena, [j + (o,) for j, o in zip(jobs, (4, 0, 2))], mu, mc.l1_expected(), 5)


def test_rounds_n19_and_the_same_batch_twice(gpu, form):
    """CUs + 3 jobs of 19 steps in one launch: three workgroups run a second job behind a first; output ranges at the start and the end
    of the store.  The batch is enqueued twice on the stream without a sync: the second run rewrites the same words."""
    cus = gpu[4].cuda.get_device_properties(0).multi_processor_count
    arena, eight, mu = mc.grid_case(3)
    count = cus + 3
    slots = 3 * (count + 2)
    out = _outs(count, 3, count + 2, seed=cus)
    want = mc.grid_expected(3)
    key = _key(gpu, "mid", form, mc.grid_key(), [0, 1, mc.GRID_N])
    _launch_and_compare(gpu, form, key, arena, [eight[g % 8] + (out[g],) for g in range(count)], mu, [want[g % 8] for g in range(count)], slots,
                        twice=True)


@pytest.mark.parametrize("n", mc.ROW_NS)
def test_row_pass(gpu, form, n):
    arena, two = edge.row_case(n)
    i, sign, off, _ = two[1]
    l = 3 if n % 2 == 0 else 2
    key = _key(gpu, f"row{n}", form, edge.row_key()[:n], [0, 200, n])
    _launch_and_compare(gpu, form, key, arena, [(i, sign, off, 1)], mc.MUS[l], mc.row_expected(form, n, l), l + 2)


@pytest.mark.parametrize("name", ["128", "80"])
def test_full_size(gpu, form, name, request):
    """n = 636 / 500 under a real key: one bit of 1 and one of 0 under both signs, ONE rotation each.  The emulation's words, and all l
    outputs decrypt to (bit if sign == +1 else 1 - bit) * 2 mu_r inside edge.decrypt_bound(n)."""
    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    l, mu = int(p.l), [ref.mu_of(r, int(p.Bgbit)) for r in range(int(p.l))]
    s2, bk, arena, _, _ = edge.full_case(name, keys)
    jobs = [(slot, sign, 0) for slot in (0, edge.FULL_SLOTS - 1) for sign in (1, -1)]
    bits = [1, 1, 0, 0]
    key = _key(gpu, "full" + name, form, bk, list(range(0, p.n, 200)) + [p.n])
    want = mc.rotate_jobs(form, arena, jobs, mu, edge.device_key("full" + name, form))
    slots = 4 * l + 2
    out = [1 + g * l for g in (2, 0, 3, 1)]
    got = _launch_and_compare(gpu, form, key, arena, [j + (out[g],) for g, j in enumerate(jobs)], mu, want, slots)
    bound = edge.decrypt_bound(p.n)
    assert all(bound < m / 2 for m in mu)
    worst = 0
    for g, (slot, sign, _) in enumerate(jobs):
        errs = edge.phase_errors(s2, got[out[g]:out[g] + l], [(slot, sign, 0, m) for m in mu], [bits[g]] * l)
        worst = max([worst] + [abs(e) for e in errs])
    print(f"set {name} {form}: worst |phase error| of {4 * l} outputs 2^{math.log2(max(worst, 1)):.2f}, bound 2^{math.log2(bound):.2f}")
    assert worst < bound, (name, form, worst, bound)


def test_rotate_many_refusals_leave_the_store(gpu):
    hip, _, st, _, _ = gpu
    tlwes, jobs, mu = mc.grid_case(3)
    key = _key(gpu, "mid", "lat", mc.grid_key(), [0, 1, mc.GRID_N])
    arena, store = _arena(gpu, tlwes), hip.Tlwe2(N2, 8)
    fill = np.full((8, N2 + 1), FILL, dtype=np.uint64)
    ok = dict(in_=[0, 6], sign=[1, -1], off=[0, 5], mu=mu, out=[0, 5])
    bad = {
        "l = 0": (dict(mu=[]), "l outside"),
        "l = 5": (dict(mu=[1, 2, 3, 4, 5]), "l outside"),
        "range past the store": (dict(out=[0, 6]), "do not fit the lvl2 store"),
        "negative out": (dict(out=[-1, 5]), "do not fit the lvl2 store"),
        "overlapping ranges": (dict(out=[3, 5]), "write the same lvl2 TLWE"),
        "input slot": (dict(in_=[0, 7]), "outside the lvl0 store"),
        "sign": (dict(sign=[1, 0]), "sign outside"),
        "over the batch cap": (dict(in_=[0] * CAP, sign=[1] * CAP, off=[0] * CAP, out=list(range(0, 3 * CAP, 3))), "batch too large"),
    }
    try:
        store.upload(st, 0, fill)
        for what, (change, message) in bad.items():
            a = {**ok, **change}
            with pytest.raises(hip.IykHipError, match=r"iyk_hip_cb_rotate_many_batch failed \(-1\): .*" + message):
                st.cb_rotate_many_batch(key, arena, a["in_"], a["sign"], a["off"], a["mu"], store, a["out"])
            assert np.array_equal(store.download(st, 0, 8), fill), what
        st.cb_rotate_many_batch(key, arena, ok["in_"], ok["sign"], ok["off"], ok["mu"], store, ok["out"])   # and a valid call succeeds
        got = store.download(st, 0, 8)
    finally:
        store.free()
    assert (got[3:5] == FILL).all() and not (got[[0, 1, 2, 5, 6, 7]] == FILL).all(axis=1).any()


def test_circuit_bootstrap_many_batch_refusals_and_words(gpu, request):
    """every refusal leaves the lvl2 store and the scratch rows as they were; a valid call gives the lvl2 TLWEs, the scratch rows and —
    through a probe ROM read, the ABI downloads no selector — the selectors of cb_rotate_many_batch + privks_batch + trgsw_from_rows
    called apart (cmux.selectors_from_tlwe0(many=True), bit by bit: it has one sign per call)."""
    hip, keys, st, made, _ = gpu
    p = keys.params
    _, bk, _, _, _ = edge.full_case("128", keys)
    bk2 = _key(gpu, "full128", "lat", bk, list(range(0, p.n, 200)) + [p.n])
    pk = made.setdefault(("pk", "uniform"), hip.PrivKsKey(N2, 1, 1))
    pk.upload(st, 0, np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32))
    A, l, per, N = 3, int(p.l), int(p.trgsw_rows), int(p.N)
    arena = hip.Arena(4)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1, 1], seed=77))
    t2, scratch = hip.Tlwe2(N2, A * l + 1), hip.Trlwe(A * per)
    t2_short, t2_small_n, scratch_short = hip.Tlwe2(N2, A * l - 1), hip.Tlwe2(64, A * l + 1), hip.Trlwe(A * per - 1)
    pk_small_n, bk2_small_n = hip.PrivKsKey(64, 1, 1), hip.Bk2Key(2)
    data = np.random.default_rng(93).integers(0, 1 << 32, size=(8, 2 * N), dtype=np.uint64).astype(np.uint32)
    rom_a, rom_b = (cmux.Rom(st, data, A, N.bit_length() - 1) for _ in range(2))
    out = hip.Arena(2 * N)
    fill2, fill1 = np.full((A * l + 1, N2 + 1), FILL, dtype=np.uint64), np.full((A * per, 2 * N), FILL32, dtype=np.uint32)
    slots, sign = [2, 0, 1], [1, -1, 1]
    try:
        t2.upload(st, 0, fill2)
        scratch.upload(st, 0, fill1)
        ok = dict(bk2=bk2, pk=pk, arena=arena, in_=slots, sign=sign, t2=t2, first=1, scratch=scratch, trgsw=rom_a.trgsw, first_slot=0)
        bad = {
            "short scratch": (dict(scratch=scratch_short), "fewer than bits"),
            "lvl2 store too small": (dict(t2=t2_short), "do not fit the lvl2 store"),
            "lvl2 first slot too far": (dict(first=2), "do not fit the lvl2 store"),
            "n_in of the store": (dict(t2=t2_small_n), "not the 2048"),
            "n_in of the private key": (dict(pk=pk_small_n), "not the private key-switching key's"),
            "bk2 of another n": (dict(bk2=bk2_small_n), "not the initialised n"),
            "selector slots": (dict(first_slot=1), "selector slots outside"),
            "sign": (dict(sign=[1, 0, 1]), "sign outside"),
            "input slot": (dict(in_=[2, 4, 1]), "outside the lvl0 store"),
            "over the batch cap": (dict(in_=[0] * (CAP // per + 1), sign=[1] * (CAP // per + 1)), "batch too large"),
        }
        call = lambda a: st.circuit_bootstrap_many_batch(a["bk2"], a["pk"], a["arena"], a["in_"], a["sign"], a["t2"], a["first"], a["scratch"],
                                                         a["trgsw"], a["first_slot"])
        for what, (change, message) in bad.items():
            with pytest.raises(hip.IykHipError, match=r"iyk_hip_circuit_bootstrap_many_batch failed \(-1\): .*" + message):
                call({**ok, **change})
            assert np.array_equal(t2.download(st, 0, A * l + 1), fill2), what
            assert np.array_equal(scratch.download(st, 0, A * per), fill1), what
        call(ok)
        rom_a.read(None, out, np.arange(N).reshape(1, N), resident=True)
        got = (t2.download(st, 0, A * l + 1), scratch.download(st, 0, A * per), rom_a.trlwe.download(st, rom_a.row(0, rom_a.layout.result), 1),
               st.download(out, 0, N))
        t2.upload(st, 0, fill2)
        scratch.upload(st, 0, fill1)
        for s, (slot, sg) in enumerate(zip(slots, sign)):
            cmux.selectors_from_tlwe0(st, bk2, pk, arena, [slot], t2, 1 + s * l, scratch, rom_b.trgsw, first_slot=s, invert=sg < 0, many=True)
            if s == 0:
                first_rows = scratch.download(st, 0, per)
        rom_b.read(None, out, np.arange(N, 2 * N).reshape(1, N), resident=True)
        want = (t2.download(st, 0, A * l + 1), rom_b.trlwe.download(st, rom_b.row(0, rom_b.layout.result), 1), st.download(out, N, N))
        # the per-digit call's selectors hold the same bits and other noise: other words
        t2.upload(st, 0, fill2)
        st.circuit_bootstrap_batch(bk2, pk, arena, slots, sign, t2, 1, scratch, rom_b.trgsw, 0)
        per_digit = t2.download(st, 0, A * l + 1)
    finally:
        for x in (arena, t2, scratch, t2_short, t2_small_n, scratch_short, pk_small_n, bk2_small_n, rom_a, rom_b, out):
            x.free()
    assert np.array_equal(got[0], want[0]) and (got[0][0] == FILL).all() and not (got[0][1:] == FILL).all(axis=1).any()
    assert np.array_equal(got[1][:per], first_rows) and not (got[1] == FILL32).all(axis=1).any()
    assert np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2]) and got[2].any()
    assert not np.array_equal(per_digit[1:], got[0][1:])
