"""GPU: iyk_hip_cmux_chain_batch, iyk_hip_trlwe_add_batch and cmux.Ram against the exact reference of tests/ram_ref.py (cmux_ref step
by step, the oracle's key switch and blind rotation), word for word, on both parameter sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cmux_ref
import ram_ref
from iyokan_amd import client, cmux

pytestmark = pytest.mark.gpu

KINDS = 5                      # fresh, zero, uniform, 0x7FFF7FFF, 0x80008000: five slots each, a chain of five steps stays in one kind
NSEL = 5 * KINDS


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
    hip, keys, _, _ = gpu
    p = keys.params
    rng = np.random.default_rng(51)
    fresh = client.encrypt_trgsw(keys, [1, 0, 1, 1, 0], seed=52)
    uniform = rng.integers(0, 1 << 32, size=fresh.shape, dtype=np.uint64).astype(np.uint32)
    trgsw = np.concatenate([fresh, np.zeros_like(fresh), uniform, np.stack([cmux_ref.worst_case_trgsw(p, 0x7FFF7FFF)] * 5),
                            np.stack([cmux_ref.worst_case_trgsw(p, 0x80008000)] * 5)])
    st = hip.Stream(0)
    sel = hip.Trgsw(NSEL)
    sel.upload(st, 0, trgsw)
    st.sync()
    yield st, sel, trgsw
    sel.free()
    st.destroy()


def _chain_batch(p, count, steps, rng):
    """count chain jobs on 4 count + 2 rows.  Row 0 is the src of every third job; job g otherwise reads src 1 + g; mem = count + 1 + g;
    out is the mem row (the RAM cell), a fresh row 2 count + 1 + g, or the job's own src.  Rows 3 count + 1 .. 4 count hold the
    accumulators of the unfused run; the last row belongs to no job."""
    ones = (1 << steps) - 1
    patterns = [0, ones, 0b01101 & ones, 0b10010 & ones]
    jobs = []
    for g in range(count):
        shared = g % 3 == 0
        src, mem = (0 if shared else 1 + g), count + 1 + g
        out = (mem, 2 * count + 1 + g, mem if shared else src)[(g // 2) % 3]
        jobs.append((5 * (g % KINDS), steps, patterns[(g + g // 4) % 4], src, mem, out))
    T = rng.integers(0, 1 << 32, size=(4 * count + 2, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    if count >= 8:   # extreme digits in the first difference of two jobs with their own src: mem - acc where pattern bit 0 is 0, else acc - mem
        for g, top in ((4, False), (5, True)):
            x, y = cmux_ref.extreme_pair(p, rng, top=top)
            T[jobs[g][3]], T[jobs[g][4]] = (y, x) if jobs[g][2] & 1 else (x, y)
    return jobs, T


@pytest.mark.parametrize("steps", [1, 2, 5])
@pytest.mark.parametrize("count", [1, 8, 9])
def test_chain_word_equality(gpu, store, count, steps):
    """one wave, a full workgroup, one over; against the step-by-step reference and against the same steps through cmux_batch"""
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    jobs, T = _chain_batch(p, count, steps, np.random.default_rng(100 * count + steps))
    fused, unfused = hip.Trlwe(T.shape[0]), hip.Trlwe(T.shape[0])
    fused.upload(st, 0, T)
    unfused.upload(st, 0, T)
    st.cmux_chain_batch(sel, fused, *zip(*jobs))
    step_jobs = [ram_ref.chain_as_cmux_jobs(j, 3 * count + 1 + g) for g, j in enumerate(jobs)]
    for s in range(steps):
        st.cmux_batch(sel, unfused, *zip(*(c[s] for c in step_jobs)))
    st.sync()
    got, got_steps = fused.download(st, 0, T.shape[0]), unfused.download(st, 0, T.shape[0])
    fused.free()
    unfused.free()
    want = ram_ref.run_chains(p, T.copy(), trgsw, jobs)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows that differ from the reference: {bad[:10]}"
    written = sorted({j[5] for j in jobs})
    assert np.array_equal(got[written], got_steps[written])
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])


def test_trlwe_add_batch(gpu):
    hip, keys, _, _ = gpu
    p = keys.params
    N = p.N
    T = np.random.default_rng(14).integers(0, 1 << 32, size=(9, 2 * N), dtype=np.uint64).astype(np.uint32)
    T[0, N] = 0xFFFFFFFF   # the offset's carry stays in the word
    a, b, out = [0, 2, 4, 4], [1, 3, 5, 2], [0, 3, 7, 8]   # out = a, out = b, a fresh row, inputs shared with other jobs
    st = hip.Stream(0)
    trl = hip.Trlwe(9)
    for off in (0, int(p.mu), 0xFFFFFFFF):
        trl.upload(st, 0, T)
        st.trlwe_add_batch(trl, a, b, out, off)
        st.sync()
        got = trl.download(st, 0, 9)
        want = T.copy()
        for x, y, o in zip(a, b, out):
            row = (T[x] + T[y]).astype(np.uint32)
            row[N] = (int(row[N]) + off) & 0xFFFFFFFF
            want[o] = row
        assert np.array_equal(got, want), off
    trl.upload(st, 0, T)
    st.trlwe_add_batch(trl, [6], [6], [6], 5)   # a = b = out
    st.sync()
    got = trl.download(st, 6, 1)[0]
    want = (T[6] + T[6]).astype(np.uint32)
    want[N] = (int(want[N]) + 5) & 0xFFFFFFFF
    assert np.array_equal(got, want)
    trl.free()
    st.destroy()


def test_errors_are_host_side(gpu, store):
    hip, keys, _, _ = gpu
    st, sel, trgsw = store
    p = keys.params
    T = np.random.default_rng(15).integers(0, 1 << 32, size=(6, 2 * p.N), dtype=np.uint64).astype(np.uint32)
    trl = hip.Trlwe(6)
    trl.upload(st, 0, T)
    # (sel0, steps, pattern, src, mem, out) per job
    bad_chain = {
        "steps = 0": [(10, 0, 0, 0, 1, 2)], "steps = 33": [(0, 33, 0, 0, 1, 2)], "steps < 0": [(10, -1, 0, 0, 1, 2)],
        "sel0 < 0": [(-1, 2, 0, 0, 1, 2)], "sel0 + steps > slots": [(NSEL - 1, 2, 0, 0, 1, 2)], "sel0 = slots": [(NSEL, 1, 0, 0, 1, 2)],
        "src": [(10, 2, 1, 6, 1, 2)], "src < 0": [(10, 2, 1, -1, 1, 2)], "mem": [(10, 2, 1, 0, 6, 2)], "mem < 0": [(10, 2, 1, 0, -1, 2)],
        "out": [(10, 2, 1, 0, 1, 6)], "out < 0": [(10, 2, 1, 0, 1, -1)],
        "out is another job's src": [(10, 2, 1, 0, 1, 1), (10, 2, 2, 2, 3, 0)],
        "out is another job's mem": [(10, 2, 1, 0, 1, 2), (10, 2, 2, 0, 3, 1)],
        "duplicate out": [(10, 2, 1, 0, 1, 4), (10, 2, 2, 0, 3, 4)],
    }
    for what, jobs in bad_chain.items():
        with pytest.raises(hip.IykHipError, match=r"\(-1\): .+") as e:
            st.cmux_chain_batch(sel, trl, *zip(*jobs))
        assert "iyk_hip_cmux_chain_batch" in str(e.value), what
    bad_add = {"a": ([6], [1], [2]), "b < 0": ([0], [-1], [2]), "out": ([0], [1], [6]), "out is another job's a": ([0, 2], [1, 3], [2, 4]),
               "out is another job's b": ([0, 2], [1, 3], [4, 1]), "duplicate out": ([0, 2], [1, 3], [5, 5])}
    for what, args in bad_add.items():
        with pytest.raises(hip.IykHipError, match=r"\(-1\): .+") as e:
            st.trlwe_add_batch(trl, *args, 0)
        assert "iyk_hip_trlwe_add_batch" in str(e.value), what
    L = hip.lib()
    one = np.zeros(1, dtype=np.int32)
    ip, up = one.ctypes.data_as(hip._i32p), one.view(np.uint32).ctypes.data_as(hip._u32p)
    assert L.iyk_hip_cmux_chain_batch(st.h, sel.ptr, sel.slots, trl.ptr, trl.slots, 1, ip, None, up, ip, ip, ip) == -1
    assert L.iyk_hip_cmux_chain_batch(st.h, sel.ptr, sel.slots, None, trl.slots, 1, ip, ip, up, ip, ip, ip) == -1
    assert L.iyk_hip_cmux_chain_batch(None, sel.ptr, sel.slots, trl.ptr, trl.slots, 1, ip, ip, up, ip, ip, ip) == -1
    assert L.iyk_hip_trlwe_add_batch(st.h, trl.ptr, trl.slots, 1, ip, None, ip, 0) == -1
    assert L.iyk_hip_last_error()
    st.sync()
    assert np.array_equal(trl.download(st, 0, 6), T)   # nothing above was launched
    # what the contract allows: a shared src, a job over its own mem and another over its own src; the stream still works
    good = [(10, 2, 1, 0, 1, 1), (10, 2, 2, 0, 2, 2), (10, 1, 0, 3, 4, 3)]
    st.cmux_chain_batch(sel, trl, *zip(*good))
    st.sync()
    got = trl.download(st, 0, 6)
    trl.free()
    assert np.array_equal(got, ram_ref.run_chains(p, T.copy(), trgsw, good))


ADDR_WIDTH, DATA_WIDTH = 3, 2
# (address, wren, wdata): write, read back, a wren = 0 clock at another address with wdata that must not land, overwrite
CLOCKS = [(5, 1, 0b10), (5, 0, 0b01), (2, 0, 0b11), (5, 1, 0b01)]
WREN, WDATA, RDATA = 0, 1, 1 + DATA_WIDTH


@pytest.fixture(scope="module")
def ram_reference(gpu):
    """The four clocks through the exact reference, once per parameter set: the inputs of every clock, rdata and the cells after it."""
    _, keys, orc, _ = gpu
    p = keys.params
    C = 1 << ADDR_WIDTH
    rng = np.random.default_rng(91)
    words = [int(x) for x in rng.integers(0, 1 << DATA_WIDTH, size=C)]
    bits = np.array([[(words[i] >> d) & 1 for i in range(C)] for d in range(DATA_WIDTH)], dtype=np.uint8)
    cells = client.encrypt_ram_trlwe(keys, bits.ravel(), seed=92).reshape(DATA_WIDTH, C, 2 * p.N)
    initial, trace = cells, []
    for n, (addr, wren, wdata) in enumerate(CLOCKS):
        trgsw = client.encrypt_trgsw(keys, [(addr >> k) & 1 for k in range(ADDR_WIDTH)], seed=200 + n)
        cts = client.encrypt_bits(keys, [wren] + [(wdata >> d) & 1 for d in range(DATA_WIDTH)], seed=300 + n)
        if n == 0:
            assert ram_ref.blind_rotate_anchor(orc, cts[0])
        rdata, _, cells = ram_ref.clock(p, orc, cells, trgsw, cts[0], cts[1:])
        read = words[addr]
        if wren:
            words[addr] = wdata
        trace.append((trgsw, cts, rdata, cells, read, list(words)))
    return initial, trace


def _run_ram(hip, p, initial, trace, fused):
    st = hip.Stream(0)
    ram = cmux.Ram(st, initial, ADDR_WIDTH, DATA_WIDTH)
    arena = hip.Arena(1 + 2 * DATA_WIDTH)
    out = []
    for trgsw, cts, _, _, _, _ in trace:
        st.upload(arena, WREN, cts)
        ram.clock(trgsw, arena, WREN, np.arange(WDATA, WDATA + DATA_WIDTH), np.arange(RDATA, RDATA + DATA_WIDTH), fused=fused)
        st.sync()
        out.append((st.download(arena, RDATA, DATA_WIDTH), ram.cells()))
    arena.free()
    ram.free()
    st.destroy()
    return out


def test_ram_end_to_end(gpu, ram_reference):
    hip, keys, _, _ = gpu
    p = keys.params
    initial, trace = ram_reference
    fused = _run_ram(hip, p, initial, trace, True)
    unfused = _run_ram(hip, p, initial, trace, False)
    C = 1 << ADDR_WIDTH
    for n, (_, _, rdata, cells, read, words) in enumerate(trace):
        for what, (got_rdata, got_cells) in (("fused", fused[n]), ("unfused", unfused[n])):
            assert np.array_equal(got_rdata, rdata), (what, n)
            bad = np.argwhere((got_cells != cells).any(axis=2))
            assert bad.size == 0, (what, n, bad[:8])
            assert [int(b) for b in client.decrypt_bits(keys, got_rdata)] == [(read >> d) & 1 for d in range(DATA_WIDTH)], (what, n)
            dec = client.decrypt_ram_trlwe(keys, got_cells.reshape(-1, 2 * p.N)).reshape(DATA_WIDTH, C)
            assert [sum(int(dec[d][i]) << d for d in range(DATA_WIDTH)) for i in range(C)] == words, (what, n)
        assert np.array_equal(fused[n][0], unfused[n][0]) and np.array_equal(fused[n][1], unfused[n][1])


def test_debug_round_error(gpu):
    """IYK_HIP_DEBUG=1 in a fresh process: the CHECK form of the chain kernel feeds iyk_hip_fft_round_error; worst-case words and
    digits; below what DESIGN.md section 2b proves for any key and digits (2^-9.0 at the 128-bit set, 2^-5.6 at the 80-bit set)"""
    which = gpu[3]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, IYK_HIP_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "ram_debug_child.py"), which], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("round_error")][-1]
    err = float(line.split()[2])
    print(line)
    assert 0.0 < err < (2.0 ** -9.0 if which == "128" else 2.0 ** -5.6)
