"""GPU: the latency form of the lvl0 -> lvl2 rotation (cb_rotate_lat_kernel, IYK_HIP_CB_KERNEL=lat) word for word against the numpy
restatement, the emulation and the wide form (IYK_HIP_CB_KERNEL=wg), and the dispatch of iyk_hip_cb_rotate_batch /
iyk_hip_circuit_bootstrap_batch through dispatch::cb_plan.  The knob is read per batch, so every test sets it with monkeypatch."""
import numpy as np
import pytest

import cb_rotate_cases as cases
import cb_rotate_ref as ref
from test_cb_rotate_lat_emul import emul as lat_emul, plan, plan_counts
from test_gpu_cb_rotate import FILL, _arena, _check, _key, _n2_inputs, _n2_jobs, _run

pytestmark = pytest.mark.gpu

N2 = ref.N2
KNOB = "IYK_HIP_CB_KERNEL"


@pytest.fixture(scope="module")
def gpu(request):
    import torch

    from iyokan_amd import hip

    keys = request.getfixturevalue("keys128")
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    made = {}
    yield hip, keys, st, made, torch
    for key in made.values():
        key.free()
    st.destroy()
    hip.cleanup()


@pytest.fixture
def lat(monkeypatch):
    monkeypatch.setenv(KNOB, "lat")


def _full_key(gpu):
    """a uniform key at the initialised n = 636, resident once per module: (Bk2Key, torus words)"""
    hip, keys, st, made, _ = gpu
    if "full" not in made:
        n = keys.params.n
        bk = np.random.default_rng(636).integers(0, 1 << 64, size=(n, 2 * cases.L2, 2, N2), dtype=np.uint64)
        key = hip.Bk2Key(n)
        for first in range(0, n, 200):
            key.upload(st, first, bk[first:first + 200])
        made["full"], made_bk["full"] = key, bk
    return made["full"], made_bk["full"]


made_bk = {}


@pytest.mark.parametrize("name", cases.CASES)
def test_cases_word_for_word(gpu, lat, name):
    hip = gpu[0]
    bk, jobs = cases.case(name)
    want = cases.expected(name)
    tl = np.stack([j[0] for j in jobs])
    out = list(range(len(jobs)))[::-1]
    assert hip.cb_rotate_form(len(jobs)) == 1
    got = _run(gpu, _key(gpu, name), tl, [(g, s, off, mu, out[g]) for g, (_, s, off, mu) in enumerate(jobs)], len(jobs) + 1)
    for g in range(len(jobs)):
        bad = np.flatnonzero(got[out[g]] != want[g])
        assert bad.size == 0, (name, g, bad[:8])
    assert (got[len(jobs)] == FILL).all()


@pytest.mark.parametrize("count", [1, 3, 27, "2cus+1"])
def test_batch_shapes(gpu, lat, count):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * cus + 1 if count == "2cus+1" else count     # the last: two rounds inside one launch
    slots = count + 3 if count > 1 else 2
    jobs = _n2_jobs(count, slots)
    assert len({j[4] for j in jobs}) == count
    _check(_run(gpu, _key(gpu, "uniform-n2"), _n2_inputs(), jobs, slots), jobs, slots)


def test_queued_batches_reuse_the_output_slots(gpu, lat):
    hip, _, st, _, torch = gpu
    key = _key(gpu, "uniform-n2")
    slots = 12
    a, b = _n2_jobs(5, slots), _n2_jobs(7, slots, salt=3)
    arena, s1 = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, slots)
    args = lambda jobs: tuple(zip(*[j[:4] for j in jobs]))
    try:
        s1.upload(st, 0, np.full((slots, N2 + 1), FILL, dtype=np.uint64))
        torch.cuda.synchronize()                                            # the arena's copy, which torch's stream made
        st.cb_rotate_batch(key, arena, *args(a), s1, [j[4] for j in a])     # two batches back to back, no sync between them
        st.cb_rotate_batch(key, arena, *args(b), s1, [j[4] for j in b])
        got = s1.download(st, 0, slots)
    finally:
        s1.free()
    later = {j[4] for j in b}
    assert later & {j[4] for j in a}
    _check(got, [j for j in a if j[4] not in later] + b, slots)


def test_full_size_against_the_emulation(gpu, lat):
    """n = 636, 3 rotations, a uniform key: the words of iyk_emul_cb_rotate"""
    key, bk = _full_key(gpu)
    n = bk.shape[0]
    tl = cases._u32(np.random.default_rng(41), (2, n + 1))
    jobs = [(0, 1, 0, ref.mu_of(0, 6), 2), (1, -1, 0x9E3779B9, ref.mu_of(1, 6), 0), (0, 1, 0, ref.mu_of(2, 6), 1)]
    got = _run(gpu, key, tl, jobs, 4)
    ntt = cases.key_ntt(bk)
    for i, sign, off, mu, out in jobs:
        assert np.array_equal(got[out], cases.emul_rotate(tl[i], sign, off, mu, ntt)), out
    assert (got[3] == FILL).all()


def test_both_forms_give_equal_stores(gpu, monkeypatch):
    hip = gpu[0]
    slots = 40
    jobs = _n2_jobs(37, slots)
    stores = {}
    for kind, form in (("wg", 0), ("lat", 1)):
        monkeypatch.setenv(KNOB, kind)
        assert hip.cb_rotate_form(len(jobs)) == form
        stores[kind] = _run(gpu, _key(gpu, "uniform-n2"), _n2_inputs(), jobs, slots)
    assert np.array_equal(stores["wg"], stores["lat"]) and (stores["lat"] != FILL).any()


def test_circuit_bootstrap_batch_dispatches_too(gpu, monkeypatch):
    """a 2-bit address: iyk_hip_circuit_bootstrap_batch under lat gives the lvl2 TLWEs and the (k+1) l selector rows per bit that
    cmux.selectors_from_tlwe0 gives under wg (the selector slots are trgsw_from_rows of those rows on both sides).  At the
    initialised n = 636: the one call refuses a lvl2 key of any other n."""
    from iyokan_amd import client, cmux

    hip, keys, st, made, _ = gpu
    p = keys.params
    A, l, per = 2, int(p.l), int(p.trgsw_rows)
    key, _ = _full_key(gpu)
    if "privks" not in made:
        pk = hip.PrivKsKey(N2, 1, 1)
        pk.upload(st, 0, np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32))
        made["privks"] = pk
    pk = made["privks"]
    arena = hip.Arena(3)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1], seed=77))
    t2 = {k: hip.Tlwe2(N2, A * l + 1) for k in ("wg", "lat")}
    rows = {k: hip.Trlwe(A * per) for k in ("wg", "lat")}
    trgsw = {k: hip.Trgsw(A) for k in ("wg", "lat")}
    got = {}
    try:
        for k in ("wg", "lat"):
            t2[k].upload(st, 0, np.full((A * l + 1, N2 + 1), FILL, dtype=np.uint64))
        monkeypatch.setenv(KNOB, "wg")
        cmux.selectors_from_tlwe0(st, key, pk, arena, [2, 0], t2["wg"], 1, rows["wg"], trgsw["wg"])
        got["wg"] = (t2["wg"].download(st, 0, A * l + 1), rows["wg"].download(st, 0, A * per))
        monkeypatch.setenv(KNOB, "lat")
        st.circuit_bootstrap_batch(key, pk, arena, [2, 0], [1, 1], t2["lat"], 1, rows["lat"], trgsw["lat"])
        got["lat"] = (t2["lat"].download(st, 0, A * l + 1), rows["lat"].download(st, 0, A * per))
    finally:
        for store in list(t2.values()) + list(rows.values()) + list(trgsw.values()) + [arena]:
            store.free()
    assert np.array_equal(got["wg"][0], got["lat"][0]) and (got["lat"][0][0] == FILL).all() and (got["lat"][0][1:] != FILL).any()
    assert np.array_equal(got["wg"][1], got["lat"][1]) and got["lat"][1].any()


def test_form_is_cb_plans_answer(gpu, monkeypatch):
    hip, _, _, _, torch = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kind = lat_emul().iyk_emul_cb_kind
    for text in (None, "wg", "lat"):
        if text is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, text)
        for count in plan_counts(cus):
            rc, form, _ = plan(count, cus, kind(text.encode() if text else None, 1))
            assert rc == 0 and hip.cb_rotate_form(count) == form, (text, count)


def test_an_unknown_kind_is_refused_and_the_store_untouched(gpu, monkeypatch):
    hip, _, st, _, _ = gpu
    key = _key(gpu, "uniform-n2")
    arena, store = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, 4)
    fill = np.full((4, N2 + 1), FILL, dtype=np.uint64)
    mu = [1 << 56]
    try:
        store.upload(st, 0, fill)
        monkeypatch.setenv(KNOB, "nonsense")
        with pytest.raises(hip.IykHipError, match=r"iyk_hip_cb_rotate_batch failed \(-1\): .*IYK_HIP_CB_KERNEL"):
            st.cb_rotate_batch(key, arena, [1], [1], [0], mu, store, [3])
        with pytest.raises(hip.IykHipError, match=r"iyk_hip_cb_rotate_form failed \(-1\): .*IYK_HIP_CB_KERNEL"):
            hip.cb_rotate_form(1)
        assert np.array_equal(store.download(st, 0, 4), fill)
        monkeypatch.setenv(KNOB, "lat")
        st.cb_rotate_batch(key, arena, [1], [1], [0], mu, store, [3])               # and the stream still works
        _check(store.download(st, 0, 4), [(1, 1, 0, mu[0], 3)], 4)
    finally:
        store.free()
