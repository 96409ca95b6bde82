"""GPU: seeded evaluation keys.  A key uploaded as b halves plus a public mask seed (PrivKsKey.upload_seeded / Bk2Key.upload_seeded:
key_mask_expand_kernel writes the a halves) must leave the store the unseeded upload of the host-rebuilt full rows leaves: compared
through the kernels that read the keys, all words of every output row.  Cases and keys: tests/key_expand_cases.py, whose restated
generator tests/test_key_expand.py holds to RFC 8439 and to the client library on the CPU."""
import ctypes

import numpy as np
import pytest

import key_expand_cases as cases
import privks_edge_cases as edge
import privks_ref

pytestmark = pytest.mark.gpu

N2 = cases.N2
FILL2 = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def gpu(request):
    import torch

    from iyokan_amd import hip

    keys = request.getfixturevalue("keys128")
    hip.initialize(keys, device_ids=(0, 0))   # two replicas on one GPU: a stream of the other replica can be offered
    st = hip.Stream(0)
    made = {}
    yield hip, keys, st, made, torch
    for x in made.values():
        x.free()
    st.destroy()
    hip.cleanup()


def _switch(gpu, key, shape, st=None):
    """every row of the key read once: the whole TRLWE store after privks_batch of cases.privks_jobs"""
    hip, _, st0, _, _ = gpu
    st = st or st0
    tl, jobs = cases.privks_jobs(shape)
    rows = len(jobs) + 1
    store, trl = hip.Tlwe2(tl.shape[1] - 1, len(tl)), hip.Trlwe(rows)
    try:
        store.upload(st, 0, tl)
        trl.upload(st, 0, np.full((rows, edge.WORDS), edge.FILL, dtype=np.uint32))
        st.privks_batch(key, store, [j[0] for j in jobs], [j[1] for j in jobs], trl, [j[2] for j in jobs])
        return trl.download(st, 0, rows)
    finally:
        store.free()
        trl.free()


def _key_a(gpu, shape="small"):
    """key A: uploaded whole with upload() from host-rebuilt full rows; resident once per module, with the words privks_batch gives"""
    hip, keys, st, made, _ = gpu
    if ("A", shape) not in made:
        key = hip.PrivKsKey(*cases.PRIVKS_SHAPES[shape])
        made["A", shape] = key
        key.upload(st, 0, cases.privks_full_rows(cases.privks_b(keys, shape), cases.SEED_A))
        made["A words", shape] = _Words(_switch(gpu, key, shape))
    return made["A", shape], made["A words", shape].w


class _Words:
    def __init__(self, w):
        self.w = w

    def free(self):
        pass


def _assert_rows(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: rows that differ: {bad[:10]} of {got.shape[0]}"


@pytest.mark.parametrize("shape", ["small", "wide"])
def test_private_key_seeded_in_odd_windows_equals_unseeded(gpu, shape):
    """n_in = 3, t = 2, basebit = 2 (48 rows) and t = 1, basebit = 8 (2040 rows, 255 per (c, i, j), more than one staging chunk): key B
    in three windows cut at odd rows, one a single row, sent out of order.  Chosen-digit TLWEs read every key row once."""
    hip, keys, st, _, _ = gpu
    _, want = _key_a(gpu, shape)
    b = cases.privks_b(keys, shape)
    key = hip.PrivKsKey(*cases.PRIVKS_SHAPES[shape])
    try:
        assert key.rows == b.shape[0]
        for first, count in cases.odd_windows(key.rows):
            key.upload_seeded(st, cases.SEED_A, first, b[first:first + count])
        got = _switch(gpu, key, shape)
    finally:
        key.free()
    _assert_rows(got, want, f"seeded {shape} key")
    assert (got[-1] == edge.FILL).all()
    if shape == "small":   # and both are the restatement's words under the rebuilt key
        tl, jobs = cases.privks_jobs(shape)
        _, t, bb = cases.PRIVKS_SHAPES[shape]
        rows_of = edge.expected_rows(tl, [j[:2] for j in jobs], t, bb, privks_ref.key_rows_of(cases.privks_full_rows(b, cases.SEED_A)))
        for i, c, out in jobs:
            assert np.array_equal(got[out], rows_of[(i, c)]), (i, c)


def _rotate(gpu, key):
    hip, _, st, _, torch = gpu
    tl, jobs = cases.bk2_jobs()
    t = torch.from_numpy(np.ascontiguousarray(tl).view(np.int32)).to("cuda:0")
    arena, store = hip.Arena.from_torch(t), hip.Tlwe2(N2, len(jobs) + 1)
    try:
        store.upload(st, 0, np.full((len(jobs) + 1, N2 + 1), FILL2, dtype=np.uint64))
        st.cb_rotate_batch(key, arena, *zip(*[j[:4] for j in jobs]), store, [j[4] for j in jobs])
        return store.download(st, 0, len(jobs) + 1)
    finally:
        store.free()


@pytest.mark.parametrize("form", ["ntt", "fft"])
def test_lvl2_key_seeded_equals_unseeded(gpu, form):
    """n = 3, both forms of the key: seeded in windows of 1 + 2 steps against the whole unseeded upload of the rebuilt steps; four
    rotations, signs +-1, all N2 + 1 words of every lvl2 TLWE"""
    hip, _, st, _, _ = gpu
    b = cases.bk2_b()
    made = []
    try:
        for _ in range(2):
            try:
                made.append(hip.Bk2Key(cases.BK2_N, form=form))
            except hip.IykHipError as e:
                if form == "fft" and "did not grant" in str(e):
                    pytest.skip("the device did not grant cb_rotate_fft_kernel its LDS: no lvl2 key of the FP64 form")
                raise
        plain, seeded = made
        plain.upload(st, 0, cases.bk2_full_steps(b, cases.SEED_A))
        seeded.upload_seeded(st, cases.SEED_A, 0, b[:1])      # the first upload of this key: it sends the tables
        seeded.upload_seeded(st, cases.SEED_A, 1, b[1:])
        want, got = _rotate(gpu, plain), _rotate(gpu, seeded)
    finally:
        for k in made:
            k.free()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
    assert (got[-1] == FILL2).all() and not (got[:-1] == FILL2).all(axis=1).any()


def test_seeded_and_unseeded_windows_on_one_key(gpu):
    hip, keys, st, _, _ = gpu
    _, want = _key_a(gpu)
    b = cases.privks_b(keys, "small")
    key = hip.PrivKsKey(*cases.PRIVKS_SHAPES["small"])
    try:
        key.upload_seeded(st, cases.SEED_A, 0, b[:17])
        key.upload(st, 17, cases.privks_full_rows(b[17:], cases.SEED_A, first_row=17))
        got = _switch(gpu, key, "small")
    finally:
        key.free()
    _assert_rows(got, want, "first window seeded, second unseeded")


def test_refusals_leave_the_store_untouched(gpu):
    """every refusal of args::key_upload_seeded_args through the C ABI: IYK_ERR_INVALID, and privks_batch still gives A's words"""
    hip, keys, st, _, _ = gpu
    key, want = _key_a(gpu)
    L = hip.lib()
    junk = np.full((key.rows + 2, keys.params.N), 0xDEADBEEF, dtype=np.uint32)   # what a wrongly accepted call would write
    pb = junk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    seed = cases.SEED_B
    other = hip.Stream(1)   # replica 1 on the same device
    try:
        calls = {
            "null stream": (None, key.h, seed, 0, 1, pb),
            "null key": (st.h, None, seed, 0, 1, pb),
            "null seed": (st.h, key.h, None, 0, 1, pb),
            "null buffer": (st.h, key.h, seed, 0, 1, None),
            "another replica": (other.h, key.h, seed, 0, 1, pb),
            "empty window": (st.h, key.h, seed, 0, 0, pb),
            "window starts past the key": (st.h, key.h, seed, key.rows + 1, 1, pb),
            "window ends past the key": (st.h, key.h, seed, key.rows - 1, 2, pb),
            "window wraps 2^64": (st.h, key.h, seed, (1 << 64) - 1, 2, pb),
        }
        assert set(calls) == set(cases.REFUSALS) - {"another GPU"}   # one GPU here: the other-GPU refusal is the CPU test's
        for name, a in calls.items():
            assert L.iyk_hip_privks_key_upload_seeded(*a) == -1, name
            assert cases.REFUSALS[name][1] in L.iyk_hip_last_error().decode(), name
        with pytest.raises(ValueError):
            key.upload_seeded(st, b"short", 0, junk[:1])
        got = _switch(gpu, key, "small")
        bk = hip.Bk2Key(2)
        try:
            pb64 = junk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            for a in ((st.h, bk.h, None, 0, 1, pb64), (st.h, bk.h, seed, 0, 1, None), (st.h, bk.h, seed, 2, 1, pb64), (st.h, bk.h, seed, 0, 0, pb64),
                      (other.h, bk.h, seed, 0, 1, pb64), (st.h, None, seed, 0, 1, pb64)):
                assert L.iyk_hip_bk2_key_upload_seeded(*a) == -1
        finally:
            bk.free()
    finally:
        other.destroy()
    _assert_rows(got, want, "after the refused calls")


def test_lifetimes(gpu):
    """upload_seeded queued behind a running batch that reads the same key on the same stream (the batch sees the old key, the next
    batch the new one); the host b buffer overwritten as soon as the call returns; two create / seeded-upload / free cycles"""
    hip, keys, _, _, _ = gpu
    _, want_a = _key_a(gpu)
    shape = "small"
    b1, b2 = cases.privks_b(keys, shape), cases.privks_b(keys, shape, mask_seed=cases.SEED_B)
    tl, jobs = cases.privks_jobs(shape)
    ins, cs, outs = [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs]
    rows = len(jobs) + 1
    _, t, bb = cases.PRIVKS_SHAPES[shape]
    rows_of = edge.expected_rows(tl, [j[:2] for j in jobs], t, bb, privks_ref.key_rows_of(cases.privks_full_rows(b2, cases.SEED_B)))
    want_b = np.full((rows, edge.WORDS), edge.FILL, dtype=np.uint32)
    for i, c, out in jobs:
        want_b[out] = rows_of[(i, c)]
    for cycle in range(2):
        st = hip.Stream(0)
        key = hip.PrivKsKey(*cases.PRIVKS_SHAPES[shape])
        store, r1, r2 = hip.Tlwe2(tl.shape[1] - 1, len(tl)), hip.Trlwe(rows), hip.Trlwe(rows)
        try:
            store.upload(st, 0, tl)
            fill = np.full((rows, edge.WORDS), edge.FILL, dtype=np.uint32)
            r1.upload(st, 0, fill)
            r2.upload(st, 0, fill)
            host = b1.copy()
            key.upload_seeded(st, cases.SEED_A, 0, host)
            host[:] = 0xFFFFFFFF                              # copied before return
            st.privks_batch(key, store, ins, cs, r1, outs)    # no sync from here on
            host2 = b2.copy()
            key.upload_seeded(st, cases.SEED_B, 0, host2)     # behind the batch that reads the key
            host2[:] = 0
            st.privks_batch(key, store, ins, cs, r2, outs)
            got1, got2 = r1.download(st, 0, rows), r2.download(st, 0, rows)
        finally:
            for x in (key, store, r1, r2):
                x.free()
            st.destroy()
        _assert_rows(got1, want_a, f"cycle {cycle}: the batch ahead of the second upload")
        _assert_rows(got2, want_b, f"cycle {cycle}: the batch behind it")
    assert not np.array_equal(want_a, want_b)
