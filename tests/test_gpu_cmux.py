"""GPU: iyk_hip_cmux_batch, the TRGSW selector store, index extraction and the ROM read tree (iyokan_amd/cmux.py) against the exact
reference of tests/cmux_ref.py, word for word, on both parameter sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cmux_ref
from iyokan_amd import client, cmux

pytestmark = pytest.mark.gpu

NSEL = 300
ADDR_WIDTH, LOG2_WORD_BITS = 10, 3
ADDRESSES = [0, 1, 127, 128, 1023, 600]


@pytest.fixture(scope="module", params=["128", "80"])
def gpu(request):
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + request.param)
    orc = request.getfixturevalue("oracle" + request.param)
    hip.initialize(keys, device_ids=(0,))
    yield hip, keys, orc, request.param
    hip.cleanup()


@pytest.fixture(scope="module")
def store(gpu):
    """NSEL selectors of every kind (torus domain, the reference's view) uploaded once, and rows of arbitrary TRLWE words."""
    hip, keys, _, _ = gpu
    p = keys.params
    rng = np.random.default_rng(41)
    fresh = client.encrypt_trgsw(keys, rng.integers(0, 2, size=NSEL // 5), seed=42)
    trgsw = np.zeros((NSEL, p.trgsw_rows, p.k + 1, p.N), dtype=np.uint32)
    for s in range(NSEL):
        kind = s % 5
        if kind == 1:
            trgsw[s] = 0x7FFF7FFF
        elif kind == 2:
            trgsw[s] = 0x80008000
        elif kind == 3:
            trgsw[s] = rng.integers(0, 1 << 32, size=trgsw[s].shape, dtype=np.uint64).astype(np.uint32)
        elif kind == 4:
            trgsw[s] = fresh[s // 5]
    st = hip.Stream(0)
    sel = hip.Trgsw(NSEL)
    sel.upload(st, 0, trgsw)
    st.sync()
    # anchor of the reference's product, once per module and set
    T = rng.integers(0, 1 << 32, size=(3, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    job = (3, 0, 1, 0, 2)
    assert np.array_equal(cmux_ref.cmux(p, T, trgsw, job), cmux_ref.cmux(p, T, trgsw, job, product=cmux_ref.negacyclic_schoolbook))
    yield st, sel, trgsw
    sel.free()
    st.destroy()


def _mixed_batch(p, count, rng):
    """count jobs on 3 count + 2 rows: job g reads rows g and count + g; two-row and rotate forms, written to a fresh row, over in0 or
    over in1; the last two rows belong to no job."""
    N = p.N
    rots = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    jobs = []
    for g in range(count):
        rotate = g % 3 == 2
        if rotate:
            out = g if (g // 3) % 2 else 2 * count + g
        else:
            out = (2 * count + g, g, count + g)[(g // 3 + g) % 3]
        jobs.append((g, g, -1 if rotate else count + g, rots[(g // 3) % 6] if rotate else 0, out))
    T = rng.integers(0, 1 << 32, size=(3 * count + 2, 2 * N), dtype=np.uint64).astype(np.uint32)
    if count >= 7:   # extreme digits in two of the pairs
        T[3], T[count + 3] = cmux_ref.extreme_pair(p, rng, top=False)
        T[4], T[count + 4] = cmux_ref.extreme_pair(p, rng, top=True)
    return jobs, T


@pytest.mark.parametrize("count", [1, 7, 8, 9, 300])
def test_word_equality(gpu, store, count):
    """one wave, a workgroup short by one, full, one over, many workgroups; every job its own selector"""
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    jobs, T = _mixed_batch(p, count, np.random.default_rng(count))
    trl = hip.Trlwe(T.shape[0])
    trl.upload(st, 0, T)
    st.cmux_batch(sel, trl, *zip(*jobs))
    st.sync()
    got = trl.download(st, 0, T.shape[0])
    trl.free()
    want = cmux_ref.run_jobs(p, T.copy(), trgsw, jobs)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows that differ: {bad[:10]}"
    written = {j[4] for j in jobs}
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])


def test_chained_batches_without_sync(gpu, store):
    """a 3-level tree over 8 rows, in place, three dependent batches on one stream"""
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    T = np.random.default_rng(8).integers(0, 1 << 32, size=(8, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    levels = [[(4 + i, 2 * i, 2 * i + 1, 0, 2 * i) for i in range(4)], [(9, 0, 2, 0, 0), (14, 4, 6, 0, 4)], [(19, 0, 4, 0, 0)]]
    trl = hip.Trlwe(8)
    trl.upload(st, 0, T)
    for jobs in levels:
        st.cmux_batch(sel, trl, *zip(*jobs))
    st.sync()
    got = trl.download(st, 0, 8)
    trl.free()
    want = T.copy()
    for jobs in levels:
        cmux_ref.run_jobs(p, want, trgsw, jobs)
    assert np.array_equal(got, want)


def test_selector_reupload_is_stream_ordered(gpu):
    hip, keys, _, _ = gpu
    p = keys.params
    st = hip.Stream(0)
    two = client.encrypt_trgsw(keys, [0, 1], seed=5)
    T = np.random.default_rng(6).integers(0, 1 << 32, size=(4, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    sel, trl = hip.Trgsw(1), hip.Trlwe(4)
    trl.upload(st, 0, T)
    sel.upload(st, 0, two[0:1])
    st.cmux_batch(sel, trl, [0], [0], [1], [0], [2])
    sel.upload(st, 0, two[1:2])
    st.cmux_batch(sel, trl, [0], [0], [1], [0], [3])
    st.sync()
    got = trl.download(st, 0, 4)
    sel.free()
    trl.free()
    st.destroy()
    assert np.array_equal(got[2], cmux_ref.cmux(p, T, two, (0, 0, 1, 0, 2)))
    assert np.array_equal(got[3], cmux_ref.cmux(p, T, two, (1, 0, 1, 0, 3)))
    assert not np.array_equal(got[2], got[3])


def test_rom_read_end_to_end(gpu):
    """6 reads in one Rom call: every arena word equals CMUX chain -> index extraction -> the oracle's key switch; every bit decrypts"""
    hip, keys, orc, _ = gpu
    p = keys.params
    rng = np.random.default_rng(77)
    content = rng.integers(0, 256, size=1 << ADDR_WIDTH).astype(np.uint8)
    data = client.encrypt_rom_trlwe(keys, np.unpackbits(content[:, None], axis=1, bitorder="little").ravel(), seed=31)
    R = len(ADDRESSES)
    abits = np.array([[(a >> k) & 1 for k in range(ADDR_WIDTH)] for a in ADDRESSES])
    trgsw = client.encrypt_trgsw(keys, abits.ravel(), seed=9).reshape(R, ADDR_WIDTH, p.trgsw_rows, p.k + 1, p.N)
    st = hip.Stream(0)
    rom = cmux.Rom(st, data, ADDR_WIDTH, LOG2_WORD_BITS, max_reads=R)
    arena = hip.Arena(R * 8)
    rom.read(trgsw, arena, np.arange(R * 8).reshape(R, 8))
    st.sync()
    got = st.download(arena, 0, R * 8)
    arena.free()
    rom.free()
    st.destroy()
    lay, plan = rom.layout, rom.plan
    for r in range(R):
        T = np.concatenate([data, np.zeros((lay.scratch_rows, 2 * p.N), dtype=np.uint32)])
        for jobs in plan:
            cmux_ref.run_jobs(p, T, trgsw[r], [(j.bit, j.in0, j.in1, j.rot, j.out) for j in jobs])
        for i in range(8):
            want = orc.keyswitch(cmux_ref.sample_extract_index(T[lay.result], i, p.N))
            assert np.array_equal(got[r * 8 + i], want), (r, i)
    dec = client.decrypt_bits(keys, got).reshape(R, 8)
    want_bits = np.array([[(int(content[a]) >> i) & 1 for i in range(8)] for a in ADDRESSES])
    assert np.array_equal(dec, want_bits)


def test_index_extraction(gpu):
    hip, keys, orc, _ = gpu
    p = keys.params
    T = np.random.default_rng(12).integers(0, 1 << 32, size=(3, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    hs = [0, 1, p.N // 2, p.N - 1]
    st = hip.Stream(0)
    trl, arena = hip.Trlwe(3), hip.Arena(5)
    trl.upload(st, 0, T)
    st.sample_extract_index_keyswitch_batch(trl, [1, 2, 0, 1], hs, [0, 1, 2, 3], arena)
    st.sample_extract_keyswitch_batch(trl.ptr, [1], [4], arena, trlwe_slots=3)
    st.sync()
    got = st.download(arena, 0, 5)
    trl.free()
    arena.free()
    st.destroy()
    for g, (row, h) in enumerate(zip([1, 2, 0, 1], hs)):
        assert np.array_equal(got[g], orc.keyswitch(cmux_ref.sample_extract_index(T[row], h, p.N))), h
    assert np.array_equal(got[4], got[0])   # the index-0 entry point


def test_errors_are_host_side(gpu, store):
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    T = np.random.default_rng(13).integers(0, 1 << 32, size=(6, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    trl = hip.Trlwe(6)
    trl.upload(st, 0, T)
    good = ([3], [0], [1], [0], [2])
    bad = {
        "sel": ([NSEL], [0], [1], [0], [2]), "sel<0": ([-1], [0], [1], [0], [2]),
        "in0": ([3], [6], [1], [0], [2]), "in1": ([3], [0], [6], [0], [2]), "out": ([3], [0], [1], [0], [-1]),
        "rot": ([3], [0], [-1], [2 * p.N], [2]), "rot<0": ([3], [0], [-1], [-1], [2]),
        "reads another job's out": ([3, 4], [0, 2], [1, 3], [0, 0], [2, 4]),
        "duplicate out": ([3, 4], [0, 1], [1, 0], [0, 0], [5, 5]),
    }
    for what, args in bad.items():
        with pytest.raises(hip.IykHipError, match=r"\(-1\): .+") as e:
            st.cmux_batch(sel, trl, *args)
        assert "iyk_hip_cmux_batch" in str(e.value), what
    L = hip.lib()
    one = np.zeros(1, dtype=np.int32)
    ip = one.ctypes.data_as(hip._i32p)
    assert L.iyk_hip_cmux_batch(st.h, sel.ptr, sel.slots, trl.ptr, trl.slots, 1, None, ip, ip, ip, ip) == -1
    assert L.iyk_hip_cmux_batch(st.h, None, sel.slots, trl.ptr, trl.slots, 1, ip, ip, ip, ip, ip) == -1
    assert L.iyk_hip_cmux_batch(None, sel.ptr, sel.slots, trl.ptr, trl.slots, 1, ip, ip, ip, ip, ip) == -1
    assert L.iyk_hip_last_error()
    arena = hip.Arena(1)
    with pytest.raises(hip.IykHipError, match=r"\(-1\)"):
        st.sample_extract_index_keyswitch_batch(trl, [0], [p.N], [0], arena)
    arena.free()
    # the stream still works, and nothing above touched the store
    st.cmux_batch(sel, trl, *good)
    st.sync()
    got = trl.download(st, 0, 6)
    trl.free()
    want = cmux_ref.run_jobs(p, T.copy(), trgsw, [(3, 0, 1, 0, 2)])
    assert np.array_equal(got, want)


def test_debug_round_error(gpu):
    """IYK_HIP_DEBUG=1 in a fresh process: the CHECK form of the kernel feeds iyk_hip_fft_round_error; worst-case words and digits"""
    which = gpu[3]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, IYK_HIP_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cmux_debug_child.py"), which], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("round_error")][-1]
    err = float(line.split()[2])
    print(line)
    assert 0.0 < err < 0.5
