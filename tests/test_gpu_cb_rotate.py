"""GPU: the lvl0 -> lvl2 blind rotation of circuit bootstrapping (iyk_hip_cb_rotate_batch, the lvl2 bootstrapping key object,
cmux.selectors_from_tlwe0) word for word against the numpy restatement of tests/cb_rotate_ref.py, or against the CPU emulation of the
kernel (itself held to the restatement by tests/test_cb_rotate_emul.py) where the restatement is too slow.

Every test that launches rotations runs twice, and its id says under which setting of IYK_HIP_CB_KERNEL: `wg` runs cb_rotate_kernel,
the 256-lane form this file was written for; `unset` runs whatever dispatch::cb_plan answers for the batch's width, which since the
latency form became the default for every width is cb_rotate_lat_kernel.  Before every launch hip.cb_rotate_form is asserted to be the
form the id stands for (0 under `wg`; unset, cb_plan's own answer through the emulation), so a change of the threshold cannot move
these tests onto another kernel unnoticed.  The knob is read per batch, so monkeypatch sets it per test."""
import functools

import numpy as np
import pytest

import cb_rotate_cases as cases
import cb_rotate_ref as ref
import cmux_ref
import privks_ref
from iyokan_amd import client, cmux
from test_cb_rotate_lat_emul import emul as lat_emul, plan

pytestmark = pytest.mark.gpu

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
N2 = ref.N2
KNOB = "IYK_HIP_CB_KERNEL"


@pytest.fixture(scope="module")
def gpu(request):
    import torch

    from iyokan_amd import hip

    keys = request.getfixturevalue("keys128")
    hip.initialize(keys, device_ids=(0, 0))   # two replicas on one GPU: a key of the other replica can be offered
    st = hip.Stream(0)
    made = {}
    yield hip, keys, st, made, torch
    for key in made.values():
        key.free()
    st.destroy()
    hip.cleanup()


@pytest.fixture(params=["wg", "unset"])
def kind(request, monkeypatch):
    """the setting of IYK_HIP_CB_KERNEL the test's id names"""
    if request.param == "wg":
        monkeypatch.setenv(KNOB, "wg")
    else:
        monkeypatch.delenv(KNOB, raising=False)
    return request.param


def _form(gpu, kind, count):
    """asserts, before a launch of `count` rotations, that the batch will run the form the id names, and returns it: 0 under `wg`;
    unset, what dispatch::cb_plan answers for that count on this device"""
    hip, _, _, _, torch = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc, want, _ = plan(count, cus, lat_emul().iyk_emul_cb_kind(b"wg" if kind == "wg" else None, 1))
    assert rc == 0 and (kind != "wg" or want == 0)
    assert hip.cb_rotate_form(count) == want, (kind, count)
    return want


def _arena(gpu, tlwes):
    """lvl0 TLWEs of any n as an arena: a torch tensor wrapped by Arena.from_torch (kept alive by the wrapper)"""
    hip, _, _, _, torch = gpu
    t = torch.from_numpy(np.ascontiguousarray(tlwes, dtype=np.uint32).view(np.int32)).to("cuda:0")
    return hip.Arena.from_torch(t)


def _key(gpu, name):
    """the case's key, resident once per module, uploaded as one step and then the rest"""
    hip, _, st, made, _ = gpu
    if name not in made:
        bk, _ = cases.case(name)
        key = hip.Bk2Key(bk.shape[0])
        key.upload(st, 0, bk[:1])
        if bk.shape[0] > 1:
            key.upload(st, 1, bk[1:])
        made[name] = key
    return made[name]


def _run(gpu, key, tlwes, jobs, slots, stream=None, kind=None):
    """jobs: (in, sign, off, mu, out) -> the whole store u64 [slots][N2 + 1] after the batch, FILL where nothing wrote.  kind: the
    knob's setting whose form is asserted just before the launch"""
    hip, _, st, _, _ = gpu
    st = stream or st
    arena, store = _arena(gpu, tlwes), hip.Tlwe2(N2, slots)
    try:
        store.upload(st, 0, np.full((slots, N2 + 1), FILL, dtype=np.uint64))
        if kind is not None:
            _form(gpu, kind, len(jobs))
        st.cb_rotate_batch(key, arena, *zip(*[(j[0], j[1], j[2], j[3]) for j in jobs]), store, [j[4] for j in jobs])
        return store.download(st, 0, slots)
    finally:
        store.free()


@pytest.mark.parametrize("name", cases.CASES)
def test_cases_word_for_word(gpu, kind, name):
    bk, jobs = cases.case(name)
    want = cases.expected(name)
    tl = np.stack([j[0] for j in jobs])
    out = list(range(len(jobs)))[::-1]
    got = _run(gpu, _key(gpu, name), tl, [(g, s, off, mu, out[g]) for g, (_, s, off, mu) in enumerate(jobs)], len(jobs) + 1,
               kind=kind)
    for g in range(len(jobs)):
        bad = np.flatnonzero(got[out[g]] != want[g])
        assert bad.size == 0, (name, g, bad[:8])
    assert (got[len(jobs)] == FILL).all()


# ---- batch shapes at n = 2 ------------------------------------------------------------------------------------------------------------
NIN = 5


@functools.lru_cache(maxsize=None)
def _n2_inputs():
    return cases._u32(np.random.default_rng(77), (NIN, 3))


@functools.lru_cache(maxsize=None)
def _n2_want(i, sign, off, mu):
    bk, _ = cases.case("uniform-n2")
    return cases.emul_rotate(_n2_inputs()[i], sign, off, mu, _n2_ntt())


@functools.lru_cache(maxsize=None)
def _n2_ntt():
    return cases.key_ntt(cases.case("uniform-n2")[0])


def _n2_jobs(count, slots, salt=0):
    """in repeats (5 inputs), 12 distinct (sign, off, mu) per input at most; out: a permutation with slot 0 and the last slot"""
    perm = np.random.default_rng(count + salt).permutation(slots)[:count].tolist()
    if 0 not in perm:
        perm[0] = 0
    if slots - 1 not in perm:
        perm[-1 if count > 1 else 0] = slots - 1
    jobs = []
    for g in range(count):
        v = (g + salt) % 12
        jobs.append(((g + salt) % NIN, 1 if v & 1 else -1, (0, 0x9E3779B9)[(v >> 1) & 1], ref.mu_of(v % 3, 6) + (v >> 2), perm[g]))
    return jobs


def _check(got, jobs, slots):
    written = {}
    for i, sign, off, mu, out in jobs:
        written[out] = _n2_want(i, sign, off, mu)
    for s in range(slots):
        want = written.get(s)
        if want is None:
            assert (got[s] == FILL).all(), f"slot {s} that no job writes changed"
        else:
            assert np.array_equal(got[s], want), f"slot {s}"


@pytest.mark.parametrize("count", [1, 3, 27, "2cus+1"])
def test_batch_shapes(gpu, kind, count):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * cus + 1 if count == "2cus+1" else count
    slots = count + 3 if count > 1 else 2
    jobs = _n2_jobs(count, slots)
    assert len({j[4] for j in jobs}) == count and {0, slots - 1} <= {j[4] for j in jobs} | ({0, 1} if count == 1 else set())
    _check(_run(gpu, _key(gpu, "uniform-n2"), _n2_inputs(), jobs, slots, kind=kind), jobs, slots)


def test_queued_batches_and_two_streams(gpu, kind):
    hip, _, st, _, torch = gpu
    key = _key(gpu, "uniform-n2")
    slots = 12
    a, b = _n2_jobs(5, slots), _n2_jobs(7, slots, salt=3)
    arena, s1, s2, s3 = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, slots), hip.Tlwe2(N2, slots), hip.Tlwe2(N2, slots)
    st2 = hip.Stream(0)
    args = lambda jobs: tuple(zip(*[j[:4] for j in jobs]))
    try:
        fill = np.full((slots, N2 + 1), FILL, dtype=np.uint64)
        for s in (s1, s2, s3):
            s.upload(st, 0, fill)
        st.sync()                                                           # the fills above, before another stream writes s3
        torch.cuda.synchronize()                                            # and the arena's copy, which torch's stream made
        _form(gpu, kind, len(a))
        _form(gpu, kind, len(b))
        st.cb_rotate_batch(key, arena, *args(a), s1, [j[4] for j in a])     # the same batch twice without a sync
        st.cb_rotate_batch(key, arena, *args(a), s1, [j[4] for j in a])
        st.cb_rotate_batch(key, arena, *args(a), s2, [j[4] for j in a])     # two different batches back to back
        st.cb_rotate_batch(key, arena, *args(b), s2, [j[4] for j in b])
        st2.cb_rotate_batch(key, arena, *args(b), s3, [j[4] for j in b])    # a second stream on the same key
        g1, g2, g3 = s1.download(st, 0, slots), s2.download(st, 0, slots), s3.download(st2, 0, slots)
    finally:
        for s in (s1, s2, s3):
            s.free()
        st2.destroy()
    _check(g1, a, slots)
    _check(g3, b, slots)
    later = {j[4] for j in b}
    _check(g2, [j for j in a if j[4] not in later] + b, slots)


def test_refusals_leave_the_store_untouched(gpu, kind):
    hip, _, st, _, _ = gpu
    key = _key(gpu, "uniform-n2")
    arena, store, small = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, 4), hip.Tlwe2(64, 4)
    fill = np.full((4, N2 + 1), FILL, dtype=np.uint64)
    mu = [1 << 56]
    try:
        store.upload(st, 0, fill)
        _form(gpu, kind, 1)                                                         # the widths of the batches below
        _form(gpu, kind, 2)
        bad = {"duplicate out": ([0, 1], [1, 1], [0, 0], mu * 2, [2, 2]), "in": ([NIN], [1], [0], mu, [0]), "in<0": ([-1], [1], [0], mu, [0]),
               "out": ([0], [1], [0], mu, [4]), "out<0": ([0], [1], [0], mu, [-1]), "sign 0": ([0], [0], [0], mu, [0]),
               "sign 2": ([0], [2], [0], mu, [0])}
        for what, (i, s, o, m, out) in bad.items():
            with pytest.raises(hip.IykHipError, match=r"iyk_hip_cb_rotate_batch failed \(-1\): .+"):
                st.cb_rotate_batch(key, arena, i, s, o, m, store, out)
        with pytest.raises(ValueError):
            st.cb_rotate_batch(key, arena, [0], [1], [0], mu, small, [0])           # a store of another n_in
        with pytest.raises(hip.IykHipError, match=r"step range outside the key"):
            key.upload(st, 2, cases.case("uniform-n2")[0][:1])
        for n, l2, bg in ((0, 4, 9), (2048, 4, 9), (2, 3, 9), (2, 4, 10)):
            with pytest.raises(hip.IykHipError, match=r"iyk_hip_bk2_key_create failed \(-1\): .+"):
                hip.Bk2Key(n, l2, bg)
        assert np.array_equal(store.download(st, 0, 4), fill)
        _form(gpu, kind, 1)
        st.cb_rotate_batch(key, arena, [1], [1], [0], mu, store, [3])               # and the stream still works
        got = store.download(st, 0, 4)
        _check(got, [(1, 1, 0, mu[0], 3)], 4)
    finally:
        store.free()
        small.free()


def test_key_of_another_replica_is_refused(gpu):
    hip, _, st, _, _ = gpu
    bk, _ = cases.case("uniform-n2")
    other = hip.Bk2Key(2, gpu_index=1)
    arena, store = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, 2)
    fill = np.full((2, N2 + 1), FILL, dtype=np.uint64)
    try:
        assert hip.bk2_key_bytes(1) == (2 * 2 * 8 * 2 * N2 + 2 * N2) * 8
        store.upload(st, 0, fill)
        with pytest.raises(hip.IykHipError, match=r"the stream and the key are on different GPUs"):
            other.upload(st, 0, bk)
        with pytest.raises(hip.IykHipError, match=r"the stream and the key are on different GPUs"):
            st.cb_rotate_batch(other, arena, [0], [1], [0], [1 << 56], store, [0])
        assert np.array_equal(store.download(st, 0, 2), fill)
    finally:
        other.free()
        store.free()
    assert hip.bk2_key_bytes(1) == 0


def test_upload_in_windows_and_key_bytes(gpu, kind):
    hip, _, st, made, _ = gpu
    bk, jobs = cases.case("uniform-n5")
    before = hip.bk2_key_bytes(0)
    whole = hip.Bk2Key(5)
    per_key = (5 * 2 * 8 * 2 * N2 + 2 * N2) * 8
    assert hip.bk2_key_bytes(0) == before + per_key          # create allocates; upload adds nothing
    whole.upload(st, 0, bk)
    assert hip.bk2_key_bytes(0) == before + per_key
    try:
        tl = np.stack([j[0] for j in jobs])
        js = [(g, s, off, mu, g) for g, (_, s, off, mu) in enumerate(jobs)]
        a = _run(gpu, whole, tl, js, len(jobs), kind=kind)
        b = _run(gpu, _key(gpu, "uniform-n5"), tl, js, len(jobs), kind=kind)   # 1 step, then the rest
    finally:
        whole.free()
    assert np.array_equal(a, b) and np.array_equal(a, cases.expected("uniform-n5"))
    assert hip.bk2_key_bytes(0) == sum((k.n * 2 * 8 * 2 * N2 + 2 * N2) * 8 for k in made.values())


@pytest.mark.parametrize("name", ["128", "80"])
def test_full_size_against_the_emulation(gpu, kind, name, request):
    """n = 636 / 500: a real key uploaded in windows, the l rotations of one address bit; words against the emulation"""
    hip, _, st, _, _ = gpu
    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    s2 = client.keygen_lvl2(N2, seed=31)
    bk = client.bk2_rows(keys, s2, 4, 9, cases.ALPHA2, seed=32)
    ct = client.encrypt_bits(keys, [1], seed=33)
    key = hip.Bk2Key(p.n)
    try:
        for first in range(0, p.n, 200):
            key.upload(st, first, bk[first:first + 200])
        mus = [ref.mu_of(r, p.Bgbit) for r in range(p.l)]
        got = _run(gpu, key, ct, [(0, 1, 0, mu, r) for r, mu in enumerate(mus)], p.l, kind=kind)
    finally:
        key.free()
    ntt = cases.key_ntt(bk)
    for r, mu in enumerate(mus):
        assert np.array_equal(got[r], cases.emul_rotate(ct[0], 1, 0, mu, ntt)), r


_PRIVKS_ROWS = {}


@pytest.mark.parametrize("invert", [False, True])
def test_selectors_from_tlwe0(gpu, kind, invert, request):
    """a 3-bit address at n = 5, a uniform private key-switching key (n_in = 2048, t = 1, basebit = 1): selectors_from_tlwe0 gives the
    selector slots selectors_from_tlwe2 gives from the downloaded rotation outputs — compared through a ROM read on known rows — and the
    rotation outputs are the emulation's words.  The read row is the restatements' (privks_ref on those words, cmux_ref's exact CMUX
    tree), and the extracted TLWEs are the oracle's key switch of that row."""
    hip, keys, st, made, _ = gpu
    orc = request.getfixturevalue("oracle128")
    p = keys.params
    A, l, per = 3, int(p.l), int(p.trgsw_rows)
    bk, _ = cases.case("uniform-n5")
    tl0 = cases._u32(np.random.default_rng(91), (A, 6))
    if "privks" not in made:
        pk = hip.PrivKsKey(N2, 1, 1)
        K = np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32)
        pk.upload(st, 0, K)
        made["privks"], _PRIVKS_ROWS["K"] = pk, K
    pk, K = made["privks"], _PRIVKS_ROWS["K"]
    data = np.random.default_rng(93).integers(0, 1 << 32, size=(8, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    arena0, out_arena = _arena(gpu, tl0), hip.Arena(2 * p.N)
    ta, tb, scratch = hip.Tlwe2(N2, A * l + 1), hip.Tlwe2(N2, A * l + 1), hip.Trlwe(A * per)
    rom = cmux.Rom(st, data, A, int(p.N).bit_length() - 1, max_reads=1)
    try:
        _form(gpu, kind, A * l)                                                     # the one rotation batch of selectors_from_tlwe0
        cmux.selectors_from_tlwe0(st, _key(gpu, "uniform-n5"), pk, arena0, [2, 0, 1], ta, 1, scratch, rom.trgsw, invert=invert)
        rom.read(None, out_arena, np.arange(p.N).reshape(1, p.N), resident=True)
        row_a = rom.trlwe.download(st, rom.row(0, rom.layout.result), 1)[0]
        tlwe_a = st.download(out_arena, 0, p.N)
        rot = ta.download(st, 1, A * l)
        tb.upload(st, 1, rot)
        cmux.selectors_from_tlwe2(st, pk, tb, 1, A, scratch, rom.trgsw)
        rom.read(None, out_arena, np.arange(p.N, 2 * p.N).reshape(1, p.N), resident=True)
        row_b = rom.trlwe.download(st, rom.row(0, rom.layout.result), 1)[0]
        tlwe_b = st.download(out_arena, p.N, p.N)
    finally:
        for x in (out_arena, ta, tb, scratch, rom):
            x.free()
    ntt = cases.key_ntt(bk)
    for bit, slot in enumerate([2, 0, 1]):
        for r in range(l):
            assert np.array_equal(rot[bit * l + r], cases.emul_rotate(tl0[slot], -1 if invert else 1, 0, ref.mu_of(r, p.Bgbit), ntt)), (bit, r)
    assert np.array_equal(row_a, row_b) and np.array_equal(tlwe_a, tlwe_b) and row_a.any()
    row_fn = privks_ref.key_rows_of(K)
    trgsw = np.stack([privks_ref.selector_rows(rot[bit * l:(bit + 1) * l], 1, 1, row_fn, l) for bit in range(A)])
    want = cmux_ref.rom_read(p, data, trgsw, A, int(p.N).bit_length() - 1)
    assert np.array_equal(row_a, want), np.flatnonzero(row_a != want)[:8]
    for i in (0, p.N // 2 + 1, p.N - 1):
        assert np.array_equal(tlwe_a[i], orc.keyswitch(cmux_ref.sample_extract_index(want, i, p.N))), i


def test_cleanup_and_initialize_with_a_key_alive():
    """in a fresh process (tests/cb_rotate_child.py): the module's fixture keeps a stream, and cleanup refuses while one lives"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cb_rotate_child.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok reinit" in r.stdout, r.stdout + r.stderr
