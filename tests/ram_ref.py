"""Exact reference of the RAM pieces (test support for test_ram_emulation / test_ram_plan / test_gpu_ram): a chain job applied step by
step with tests/cmux_ref.py, and one clock of the reference's RAM network (/root/reference/src/iyokan_tfhepp.hpp:680-731) from
cmux_ref.cmux, the oracle's key switch and the oracle's blind rotation — never the code under test."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cmux_ref
import oracle_lib

_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int32)
M32 = 0xFFFFFFFF


def chain(p, T, trgsw, job):
    """acc = T[src]; per step j the CMUX job (sel0 + j, in0 = mem, in1 = acc) where bit j of pattern is 1, (sel0 + j, in0 = acc,
    in1 = mem) where it is 0.  Returns the 2N words of the final accumulator."""
    sel0, steps, pattern, src, mem, _ = job
    two = np.stack([T[src], T[mem]])   # row 0: the accumulator, row 1: T[mem]
    for j in range(steps):
        step = (sel0 + j, 1, 0, 0, 0) if (pattern >> j) & 1 else (sel0 + j, 0, 1, 0, 0)
        two[0] = cmux_ref.cmux(p, two, trgsw, step)
    return two[0].copy()


def run_chains(p, T, trgsw, jobs):
    """The chain jobs one after the other, in place on T."""
    for job in jobs:
        T[job[5]] = chain(p, T, trgsw, job)
    return T


def chain_as_cmux_jobs(job, acc):
    """The same chain as dependent cmux jobs (sel, in0, in1, rot, out), the accumulator in row `acc` between the steps."""
    sel0, steps, pattern, src, mem, out = job
    jobs = []
    for j in range(steps):
        cur, dst = (src if j == 0 else acc), (out if j == steps - 1 else acc)
        jobs.append((sel0 + j, mem, cur, 0, dst) if (pattern >> j) & 1 else (sel0 + j, cur, mem, 0, dst))
    return jobs


def emul():
    em = cmux_ref.emul()
    em.emu_cmux_chain.argtypes = [ctypes.c_int, _u32p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double), ctypes.c_uint64, _i32p,
                                  ctypes.c_uint64]
    return em


def emu_chain_rc(em, p, T, spec, slots, jobs):
    """emu_cmux_chain in place on T; returns its status."""
    jobs = np.ascontiguousarray(np.asarray(jobs, dtype=np.int64).astype(np.uint32).view(np.int32)).reshape(-1, 6)
    return em.emu_cmux_chain(0 if p.l == 3 else 1, T.ctypes.data_as(_u32p), T.shape[0], spec.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                             slots, jobs.ctypes.data_as(_i32p), jobs.shape[0])


def emu_chain_run(em, p, T, spec, slots, jobs):
    T = np.ascontiguousarray(T, dtype=np.uint32).copy()
    assert emu_chain_rc(em, p, T, spec, slots, jobs) == 0
    return T


def _mode(orc):
    """The fastest of the oracle's exact products (word-equal to each other: blind_rotate_anchor)."""
    return orc.MODES["fft"] if orc.has_fft() else orc.MODES["goldilocks"]


def blind_rotate(orc, lin, mode=None):
    """TLWE lvl0 -> TRLWE (2N words), test vector mu: the oracle's rotation with exact integer products."""
    lin = np.ascontiguousarray(lin, dtype=np.uint32)
    acc = np.zeros(2 * orc.p.N, dtype=np.uint32)
    oracle_lib.lib().orc_blind_rotate(orc.ctx, lin.ctypes.data_as(_u32p), acc.ctypes.data_as(_u32p), _mode(orc) if mode is None else mode)
    return acc


def blind_rotate_many(orc, lins):
    """blind_rotate of every row, on a few threads (the oracle's context is read-only; ctypes releases the GIL)."""
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda lin: blind_rotate(orc, lin), lins))


def blind_rotate_anchor(orc, lin):
    """The product used above against the oracle's integer (Goldilocks) one, on one input."""
    return np.array_equal(blind_rotate(orc, lin), blind_rotate(orc, lin, orc.MODES["goldilocks"]))


def mux_wo_se(p, orc, cs, c1, c0):
    """TFHEpp::HomMUXwoSE: BlindRotate(cs + c1 - mu) + BlindRotate(-cs + c0 - mu), + mu at coefficient 0 of b."""
    t1 = (cs + c1).astype(np.uint32)
    t0 = (c0 - cs).astype(np.uint32)
    t1[-1] = (int(t1[-1]) - int(p.mu)) & M32
    t0[-1] = (int(t0[-1]) - int(p.mu)) & M32
    out = (blind_rotate(orc, t1) + blind_rotate(orc, t0)).astype(np.uint32)
    out[p.N] = (int(out[p.N]) + int(p.mu)) & M32
    return out


def read_plane(p, orc, cells, trgsw):
    """RAMUX of one bit plane (cells: [2^a][2N]; address bit b selects between rows 2 i and 2 i + 1 of level b, 1 = the odd one),
    then SEI(0) and the key switch: the TLWE lvl0 of the addressed bit."""
    cur = [c for c in cells]
    b = 0
    while len(cur) > 1:
        nxt = []
        for i in range(len(cur) // 2):
            nxt.append(cmux_ref.cmux(p, np.stack([cur[2 * i], cur[2 * i + 1]]), trgsw, (b, 0, 1, 0, 0)))
        cur, b = nxt, b + 1
    return orc.keyswitch(cmux_ref.sample_extract_index(cur[0], 0, p.N))


def clock(p, orc, cells, trgsw, wren, wdata, only_cells=None):
    """One clock on cells [w][2^a][2N] with the address selectors trgsw [a][...] and the TLWEs wren, wdata[w].
    Returns (rdata [w][n+1], chain outputs before the refresh {(plane, cell): 2N words}, the new cells); only_cells restricts the
    write-back to some cell indices (the others keep their rows)."""
    w, C = cells.shape[0], cells.shape[1]
    a = C.bit_length() - 1
    rdata = np.stack([read_plane(p, orc, cells[d], trgsw) for d in range(w)])
    new = cells.copy()
    before = {}
    for d in range(w):
        written = mux_wo_se(p, orc, wren, wdata[d], rdata[d])
        for i in (range(C) if only_cells is None else only_cells):
            before[(d, i)] = chain(p, np.stack([written, cells[d][i]]), trgsw, (0, a, i, 0, 1, 1))
    tlwes = [orc.keyswitch(cmux_ref.sample_extract_index(row, 0, p.N)) for row in before.values()]
    for (d, i), row in zip(before, blind_rotate_many(orc, tlwes)):
        new[d][i] = row
    return rdata, before, new


def run_clocks(p, orc, cells, clocks):
    """clock() for every (addr, wren, wdata, selectors, [wren, wdata] TLWEs) of memory_cases.ram_case (one bit plane), in order.
    Returns [(rdata, chain outputs before the refresh, cells after the clock)]."""
    trace = []
    for _, _, _, trgsw, cts in clocks:
        rdata, before, cells = clock(p, orc, cells, trgsw, cts[0], cts[1:2])
        trace.append((rdata, before, cells))
    return trace
