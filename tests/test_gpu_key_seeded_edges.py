"""GPU: the seeded key uploads where their host code stops being trivial (tests/test_gpu_key_seeded.py runs one staging chunk per call on
a long-lived stream): windows cut at the chunk edges, a whole key in one call (`done` = 0, 8, 16), more chunks in a call than the staging
ring has slots, the ring reallocated inside an upload on a fresh stream, a key read on another stream than it was sent on, seeded and
unseeded windows on one lvl2 key, host buffers that are views, and a real seeded key of nine chunks under which rotations decrypt.

The expected store is always the UNSEEDED upload of the host-rebuilt full rows (cases.bk2_full_steps / cases.privks_full_rows: the
restated generator), sent whole on the module's stream; every output row is compared word for word, the canary row must stay.  The
b halves of a lvl2 key are cases.bk2_b(n=17), a real key's, or uniform words (n = 67, ring wrap): the stores must agree whatever b is.
The rotation here is not test_gpu_key_seeded._rotate, which is tied to n = 3 and the module's stream: _Rot builds its arena and stores
ahead of the case, since a store's upload synchronises its stream and the ring-wrap and growth cases must enqueue without one.

The ring-wrap cases guard the order of acquire_stage / release_stage around the expand kernel and the transform.  A release recorded
too early is a race: these cases can catch it, they cannot be required to."""
import functools
import math

import numpy as np
import pytest

import cb_rotate_edge_cases as cb_edge
import key_expand_cases as cases
import privks_edge_cases as edge
from test_gpu_key_seeded import FILL2, _assert_rows, _key_a, _switch, _Words, gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N2 = cases.N2
N17 = 17   # three staging chunks: 8 + 8 + 1 steps


@pytest.fixture(params=["ntt", "fft"])
def form(request):
    return request.param


def _new_key(gpu, n, form):
    hip = gpu[0]
    try:
        return hip.Bk2Key(n, form=form)
    except hip.IykHipError as e:
        if form == "fft" and "did not grant" in str(e):
            pytest.skip("the device did not grant cb_rotate_fft_kernel its LDS: no lvl2 key of the FP64 form")
        raise


class _Rot:
    """cases.bk2_jobs(n) (or the jobs given, (in, sign, off, mu, out)) ready on the device: the arena and `stores` canary-filled lvl2
    stores.  run() only enqueues; words() downloads a whole store, canary row last."""

    def __init__(self, gpu, n, stores=1, tl=None, jobs=None):
        hip, _, st, _, torch = gpu
        if tl is None:
            tl, jobs = cases.bk2_jobs(n)
        assert tl.shape[1] == n + 1 and sorted(j[4] for j in jobs) == list(range(len(jobs)))
        self.jobs, self.rows = jobs, len(jobs) + 1
        self.t = torch.from_numpy(np.ascontiguousarray(tl).view(np.int32)).to("cuda:0")
        self.arena = hip.Arena.from_torch(self.t)
        self.stores = [hip.Tlwe2(N2, self.rows) for _ in range(stores)]
        for s in self.stores:
            s.upload(st, 0, np.full((self.rows, N2 + 1), FILL2, dtype=np.uint64))

    def run(self, st, key, k=0):
        st.cb_rotate_batch(key, self.arena, *zip(*[j[:4] for j in self.jobs]), self.stores[k], [j[4] for j in self.jobs])

    def words(self, st, k=0):
        return self.stores[k].download(st, 0, self.rows)

    def free(self):
        for s in self.stores:
            s.free()


def _rotate(gpu, key, n, st=None):
    st = st or gpu[2]
    rot = _Rot(gpu, n)
    try:
        rot.run(st, key)
        return rot.words(st)
    finally:
        rot.free()


def _assert_words(got, want, what):
    _assert_rows(got, want, what)
    assert (got[-1] == FILL2).all() and not (got[:-1] == FILL2).all(axis=1).any(), what


@functools.lru_cache(maxsize=None)
def _b17(seed=cases.SEED_A):
    return cases.bk2_b(mask_seed=seed, n=N17)


@functools.lru_cache(maxsize=None)
def _full17(seed=cases.SEED_A):
    return cases.bk2_full_steps(_b17(seed), seed)


def _plain(gpu, form, name, n, full):
    """the words the rotations give under the unseeded upload of full() (whole, on the module's stream); once per module and form"""
    _, _, st, made, _ = gpu
    if (name, form) not in made:
        key = _new_key(gpu, n, form)
        try:
            key.upload(st, 0, full())
            made[name, form] = _Words(_rotate(gpu, key, n))
        finally:
            key.free()
    return made[name, form].w


def _plain17(gpu, form):
    return _plain(gpu, form, "A17", N17, _full17)


# ---- lvl2 key: the chunk loop ----------------------------------------------------------------------------------------------------------

def test_lvl2_windows_at_the_chunk_edges(gpu, form):
    """n = 17 through chunk_windows(17, 8), as sent: steps [7, 16) — a whole chunk whose first step is no multiple of 8, then step 15
    alone with done = 8 — then step 16, then the head [0, 7)"""
    _, _, st, _, _ = gpu
    want, b = _plain17(gpu, form), _b17()
    key = _new_key(gpu, N17, form)
    try:
        for first, count in cases.chunk_windows(N17, cases.BK2_CHUNK):
            key.upload_seeded(st, cases.SEED_A, first, b[first:first + count])
        got = _rotate(gpu, key, N17)
    finally:
        key.free()
    _assert_words(got, want, f"{form} key seeded through {cases.chunk_windows(N17, cases.BK2_CHUNK)}")


def test_lvl2_whole_key_in_one_call(gpu, form):
    """n = 17 in one call: chunks of 8 + 8 + 1 steps, done = 0, 8, 16 in the b offset, the mask's row index and the transform's step"""
    _, _, st, _, _ = gpu
    want = _plain17(gpu, form)
    key = _new_key(gpu, N17, form)
    try:
        key.upload_seeded(st, cases.SEED_A, 0, _b17())
        got = _rotate(gpu, key, N17)
    finally:
        key.free()
    _assert_words(got, want, f"{form} key seeded whole")


@functools.lru_cache(maxsize=None)
def _uniform67(which):
    """(b halves of uniform words u64 [67][8][N2], the full steps under the seed) for key "A" / "B" """
    seed = {"A": cases.SEED_A, "B": cases.SEED_B}[which]
    b = np.random.default_rng(670 + ord(which)).integers(0, 1 << 64, size=(cases.REAL_N, 2 * cases.L2, N2), dtype=np.uint64)
    return b, cases.bk2_full_steps(b, seed)


def test_lvl2_ring_wrap_and_lifetimes(gpu, form):
    """n = 67 in one call: nine chunks (and the tables' slot ahead of them), so the last ones take slots whose expand kernel and transform
    of eight chunks earlier were enqueued in this same call.  The rotations follow with no sync; key B whole under SEED_B follows them
    with no sync, over the key they read; a second batch follows that.  The host b buffers are overwritten as each call returns.  The
    first batch sees key A, the second key B."""
    _, _, st, _, _ = gpu
    n = cases.REAL_N
    assert -(-n // cases.BK2_CHUNK) > cases.STAGE_RING
    want_a = _plain(gpu, form, "A67", n, lambda: _uniform67("A")[1])
    want_b = _plain(gpu, form, "B67", n, lambda: _uniform67("B")[1])
    assert not np.array_equal(want_a, want_b)
    key, rot = _new_key(gpu, n, form), _Rot(gpu, n, stores=2)
    try:
        host = _uniform67("A")[0].copy()
        key.upload_seeded(st, cases.SEED_A, 0, host)
        host[:] = 0xFFFFFFFFFFFFFFFF              # copied before return
        rot.run(st, key, 0)                       # no sync from here on
        host2 = _uniform67("B")[0].copy()
        key.upload_seeded(st, cases.SEED_B, 0, host2)
        host2[:] = 0
        rot.run(st, key, 1)
        got_a, got_b = rot.words(st, 0), rot.words(st, 1)
    finally:
        rot.free()
        key.free()
    _assert_words(got_a, want_a, f"{form}: the batch ahead of the second upload")
    _assert_words(got_b, want_b, f"{form}: the batch behind it")


# ---- private key: more chunks than slots -------------------------------------------------------------------------------------------------

def test_private_key_ring_wrap(gpu):
    """(3, 3, 8): 6120 rows.  Whole in one call — 12 chunks of 512 rows (the last of 488), the ninth on takes a slot of this call again —
    and on a second key through chunk_windows(6120, 512): [511, 1024) lands as a whole chunk at an unaligned row with a row left over.
    The 255 chosen-digit TLWEs under c = 0, 1 read every key row once."""
    hip, keys, st, _, _ = gpu
    shape = "ring"
    _, want = _key_a(gpu, shape)
    b = cases.privks_b(keys, shape)
    whole, windows = hip.PrivKsKey(*cases.PRIVKS_SHAPES[shape]), hip.PrivKsKey(*cases.PRIVKS_SHAPES[shape])
    try:
        assert whole.rows == b.shape[0] == 6120 and -(-whole.rows // cases.PRIVKS_CHUNK) > cases.STAGE_RING
        host = b.copy()
        whole.upload_seeded(st, cases.SEED_A, 0, host)
        host[:] = 0xFFFFFFFF
        for first, count in cases.chunk_windows(windows.rows, cases.PRIVKS_CHUNK):
            windows.upload_seeded(st, cases.SEED_A, first, b[first:first + count])
        got = [_switch(gpu, k, shape) for k in (whole, windows)]
    finally:
        whole.free()
        windows.free()
    for g, what in zip(got, ("whole in one call", "through chunk_windows")):
        _assert_rows(g, want, f"seeded ring key {what}")
        assert (g[-1] == edge.FILL).all() and not (g[:-1] == edge.FILL).all(axis=1).any()


# ---- staging growth inside an upload, streams ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("windows", [[(0, 9), (9, 8)], [(0, 1), (1, 16)]], ids=["tables-then-full-chunk", "one-step-then-two-chunks"])
def test_staging_grows_inside_a_seeded_upload(gpu, form, windows):
    """A fresh stream whose first staged call is the seeded upload (everything else is made ready on the module's stream).  [0, 9): the
    tables size the slot small, the full chunk (2 MiB of window + 1 MiB of b) reallocates the ring behind the tables' copy, then a
    one-step slot.  [0, 1) then [1, 17): the ring grows between two windows of one key.  The rotation runs on the same stream."""
    hip = gpu[0]
    want, b = _plain17(gpu, form), _b17()
    key, rot = _new_key(gpu, N17, form), _Rot(gpu, N17)
    fresh = hip.Stream(0)
    try:
        for first, count in windows:
            key.upload_seeded(fresh, cases.SEED_A, first, b[first:first + count])
        rot.run(fresh, key)
        got = rot.words(fresh)
    finally:
        rot.free()
        key.free()
        fresh.destroy()
    _assert_words(got, want, f"{form} key seeded on a fresh stream in {windows}")


@pytest.mark.parametrize("how", ["sync", "wait_stream"])
def test_another_stream_reads_the_key(gpu, form, how):
    """sync: sent on a fresh stream, that stream synchronised, read on the module's.  wait_stream: sent on the module's stream, read on a
    fresh one that waits for it on the device, the host not blocking in between."""
    hip, _, st, _, _ = gpu
    want, b = _plain17(gpu, form), _b17()
    key, rot = _new_key(gpu, N17, form), _Rot(gpu, N17)
    fresh = hip.Stream(0)
    try:
        if how == "sync":
            key.upload_seeded(fresh, cases.SEED_A, 0, b)
            fresh.sync()
            rot.run(st, key)
            got = rot.words(st)
        else:
            key.upload_seeded(st, cases.SEED_A, 0, b)
            fresh.wait_stream(st)
            rot.run(fresh, key)
            got = rot.words(fresh)
    finally:
        rot.free()
        key.free()
        fresh.destroy()
    _assert_words(got, want, f"{form} key read on another stream ({how})")


# ---- mixed windows, host views -------------------------------------------------------------------------------------------------------------

def test_seeded_and_unseeded_windows_on_one_lvl2_key(gpu, form):
    """steps [0, 9) seeded, [9, 17) unseeded from the rebuilt rows: key A.  Then [7, 10) seeded again under SEED_B with that key's b: the
    plain key whose steps 7 .. 9 are the rebuilt SEED_B rows."""
    _, _, st, _, _ = gpu
    want_a, b, full = _plain17(gpu, form), _b17(), _full17()
    b2 = _b17(cases.SEED_B)[7:10]

    def patched():
        rows = full.copy()
        rows[7:10] = cases.bk2_full_steps(b2, cases.SEED_B, first_step=7)
        return rows

    want_ab = _plain(gpu, form, "A17 with 7..9 of B", N17, patched)
    assert not np.array_equal(want_a, want_ab)
    key = _new_key(gpu, N17, form)
    try:
        key.upload_seeded(st, cases.SEED_A, 0, b[:9])
        key.upload(st, 9, full[9:])
        got_a = _rotate(gpu, key, N17)
        key.upload_seeded(st, cases.SEED_B, 7, b2)
        got_ab = _rotate(gpu, key, N17)
    finally:
        key.free()
    _assert_words(got_a, want_a, f"{form}: nine steps seeded, eight unseeded")
    _assert_words(got_ab, want_ab, f"{form}: steps 7 .. 9 seeded again under another seed")


def _views(b):
    """b as callers hand it over: at an odd u32 offset of a larger buffer (a u64 array that is only 4-byte aligned), and as every
    second row of a buffer of twice the rows"""
    flat = np.full(b.nbytes // 4 + 3, 0xDEADBEEF, dtype=np.uint32)
    odd = flat[1:1 + b.nbytes // 4].view(b.dtype).reshape(b.shape)
    odd[...] = b
    assert odd.ctypes.data % 8 == 4 and odd.flags.c_contiguous
    big = np.full((2 * b.shape[0],) + b.shape[1:], 0xDEADBEEF, dtype=b.dtype)
    big[::2] = b
    strided = big[::2]
    assert not strided.flags.c_contiguous
    return {"odd offset": odd, "every second row": strided}


def test_lvl2_host_buffers_that_are_views(gpu, form):
    _, _, st, _, _ = gpu
    want = _plain17(gpu, form)
    for what, view in _views(_b17()).items():
        key = _new_key(gpu, N17, form)
        try:
            key.upload_seeded(st, cases.SEED_A, 0, view)
            got = _rotate(gpu, key, N17)
        finally:
            key.free()
        _assert_words(got, want, f"{form} key from a view ({what})")


def test_private_key_host_buffers_that_are_views(gpu):
    hip, keys, st, _, _ = gpu
    _, want = _key_a(gpu, "small")
    for what, view in _views(cases.privks_b(keys, "small")).items():
        key = hip.PrivKsKey(*cases.PRIVKS_SHAPES["small"])
        try:
            key.upload_seeded(st, cases.SEED_A, 0, view)
            got = _switch(gpu, key, "small")
        finally:
            key.free()
        _assert_rows(got, want, f"private key from a view ({what})")
        assert (got[-1] == edge.FILL).all()


# ---- a seeded key is a key ----------------------------------------------------------------------------------------------------------------

def test_rotations_under_a_real_seeded_key_decrypt(gpu, form):
    """The real n = 67 key (cases.bk2_real: b halves from the client library, nine chunks) seeded in one call; an encrypted 1 and an
    encrypted 0 under both signs at the three mu_r of the 128-bit set through the per-digit cb_rotate_batch.  Every output decrypts to
    (bit if sign == +1 else 1 - bit) * 2 mu inside cb_rotate_edge_cases.decrypt_bound(67), and is the unseeded key's word for word.
    Measured on an MI355X: worst |phase error| of the 12 outputs 2^38.34 under either form, bound 2^39.96."""
    _, _, st, _, _ = gpu
    n = cases.REAL_N
    _, s2, b = cases.bk2_real()
    ct, jobs4, bits = cases.bk2_real_jobs()
    outs = np.random.default_rng(672).permutation(len(jobs4)).tolist()
    jobs = [j + (o,) for j, o in zip(jobs4, outs)]
    bound = cb_edge.decrypt_bound(n)
    assert all(bound < j[3] / 2 for j in jobs4)
    seeded, plain = _new_key(gpu, n, form), _new_key(gpu, n, form)
    rot = _Rot(gpu, n, stores=2, tl=ct, jobs=jobs)
    try:
        seeded.upload_seeded(st, cases.SEED_A, 0, b)
        rot.run(st, seeded, 0)
        plain.upload(st, 0, cases.bk2_full_steps(b, cases.SEED_A))
        rot.run(st, plain, 1)
        got, want = rot.words(st, 0), rot.words(st, 1)
    finally:
        rot.free()
        seeded.free()
        plain.free()
    _assert_words(got, want, f"{form}: the real key seeded against unseeded")
    errs = cb_edge.phase_errors(s2, np.ascontiguousarray(got[outs]), jobs4, bits)
    worst = max(abs(e) for e in errs)
    print(f"{form}: worst |phase error| of {len(errs)} outputs under the seeded n = {n} key 2^{math.log2(max(worst, 1)):.2f}, "
          f"bound 2^{math.log2(bound):.2f}")
    assert worst < bound, (form, worst, bound)
