"""iyokan_amd.cmux.ram_read_plan / ram_write_jobs: structure of the launches, the plan on plaintext bits (a CMUX is a select), and one
encrypted clock of an addr_width 8 RAM computed with the exact reference (tests/cmux_ref.py, tests/ram_ref.py, the oracle; no GPU,
no emulation) — the noise check of the write-back chain."""
import numpy as np
import pytest

import cmux_ref
import memory_cases
import ram_ref
from iyokan_amd import client, cmux

N = 1024


@pytest.mark.parametrize("aw", [1, 2, 3, 5, 8])
def test_plan_structure(aw):
    lay, plan = cmux.ram_layout(aw, N), cmux.ram_read_plan(aw, N)
    C = 1 << aw
    assert lay.data_rows == C and lay.log2_words == 0 and len(plan) == aw
    written = set()
    for b, jobs in enumerate(plan):
        assert len(jobs) == C >> (b + 1)
        for j in jobs:
            assert j.bit == b and j.in1 >= 0 and j.rot == 0
            for r in (j.in0, j.in1, j.out):
                assert 0 <= r < lay.data_rows + lay.scratch_rows
            assert j.out >= C                                                     # the cells are never written by a read
            assert all(r < C or r in written for r in (j.in0, j.in1))             # cells or outputs of an EARLIER launch
            assert all(j.out not in (k.in0, k.in1, k.out) for k in jobs if k is not j)   # the contract of cmux_batch
        if b == 0:   # the even cell in in0, the odd one in in1
            assert [(j.in0, j.in1) for j in jobs] == [(2 * i, 2 * i + 1) for i in range(C // 2)]
        written.update(j.out for j in jobs)
    assert plan[-1][0].out == lay.result
    # write jobs: one per cell, in place, independent under the chain contract
    src = lay.data_rows + lay.scratch_rows
    jobs = cmux.ram_write_jobs(aw, src, first_cell=0, sel0=0)
    assert [j.pattern for j in jobs] == list(range(C))
    for j in jobs:
        assert (j.sel0, j.steps, j.src, j.mem, j.out) == (0, aw, src, j.pattern, j.pattern)
        assert all(j.out not in (k.src, k.mem, k.out) for k in jobs if k is not j)
    # the unfused form: step s of every chain in one launch, independent under the cmux_batch contract, same selector per launch
    steps = [cmux.chain_steps(j, src + 1 + g) for g, j in enumerate(jobs)]
    for s in range(aw):
        launch = [c[s] for c in steps]
        assert {k[0] for k in launch} == {s}
        for g, k in enumerate(launch):
            assert all(k[4] not in (m[1], m[2], m[4]) for h, m in enumerate(launch) if h != g)
        assert launch == [ram_ref.chain_as_cmux_jobs(tuple(j), src + 1 + g)[s] for g, j in enumerate(jobs)]


def _clear_read(aw, cells, abits):
    lay = cmux.ram_layout(aw, N)
    T = list(cells) + [None] * lay.scratch_rows
    for jobs in cmux.ram_read_plan(aw, N):
        for j in jobs:
            T[j.out] = T[j.in1] if abits[j.bit] else T[j.in0]   # a selector of 1 selects in1
    return T[lay.result]


def _clear_chain(job, T, abits):
    acc = T[job.src]
    for j in range(job.steps):
        s = abits[job.sel0 + j]
        # pattern bit 1: the job (in0 = mem, in1 = acc); pattern bit 0: the job (in0 = acc, in1 = mem)
        acc = (acc if s else T[job.mem]) if (job.pattern >> j) & 1 else (T[job.mem] if s else acc)
    return acc


@pytest.mark.parametrize("aw", [1, 2, 3, 4])
def test_plan_in_the_clear(aw):
    C = 1 << aw
    rng = np.random.default_rng(aw)
    content = [int(b) for b in rng.integers(0, 2, size=C)]
    for addr in range(C):
        abits = [(addr >> k) & 1 for k in range(aw)]
        rdata = _clear_read(aw, content, abits)
        assert rdata == content[addr]
        for wren in (0, 1):
            for wdata in (0, 1):
                written = wdata if wren else rdata        # MUXwoSE
                T = content + [written]
                new = [_clear_chain(j, T, abits) for j in cmux.ram_write_jobs(aw, C)]
                want = list(content)
                if wren:
                    want[addr] = wdata
                assert new == want, (addr, wren, wdata)


AW, ADDR = 8, 0b10010110
CELLS = [ADDR, ADDR ^ 1, ADDR ^ 2, ADDR ^ 128, 0, 255, ADDR ^ 0xFF]


def test_exact_reference_clock(keys128, oracle128):
    """One clock of a 256 x 1 RAM at the 128-bit set through the exact reference, fresh selectors, wren = 1 with wdata the complement
    of the addressed cell: read tree (8 levels), SEI + key switch, MUXwoSE, the 8-step chain of the addressed cell, its three
    bit-neighbours, cells 0, 255 and the complement address.  Measured: worst |phase error| at coefficient 0 of the chain outputs
    before the refresh = 2^23.2 (read tree output at the one address: 2^17.6) against the bound mu/2 = 2^28: a margin of 4.8 bits."""
    keys, orc, p = keys128, oracle128, keys128.params
    C = 1 << AW
    rng = np.random.default_rng(88)
    content = rng.integers(0, 2, size=C).astype(np.uint8)
    cells = client.encrypt_ram_trlwe(keys, content, seed=61)
    trgsw = client.encrypt_trgsw(keys, [(ADDR >> k) & 1 for k in range(AW)], seed=62)
    wbit = 1 - int(content[ADDR])
    wren, wdata = client.encrypt_bits(keys, [1, wbit], seed=63)
    lay = cmux.ram_layout(AW, p.N)
    T = np.concatenate([cells, np.zeros((lay.scratch_rows + 1, 2 * p.N), dtype=np.uint32)])
    for jobs in cmux.ram_read_plan(AW, p.N):
        cmux_ref.run_jobs(p, T, trgsw, [(j.bit, j.in0, j.in1, j.rot, j.out) for j in jobs])
    mu = int(p.mu)
    target = lambda bit: mu if bit else -mu
    ph = lambda row: int(client.trlwe_phases(keys, row[None])[0][:1].view(np.int32)[0])
    read_err = abs(ph(T[lay.result]) - target(content[ADDR]))
    assert read_err < mu // 2
    rdata = orc.keyswitch(cmux_ref.sample_extract_index(T[lay.result], 0, p.N))
    assert client.decrypt_bits(keys, rdata)[0] == content[ADDR]
    src = lay.data_rows + lay.scratch_rows
    T[src] = ram_ref.mux_wo_se(p, orc, wren, wdata, rdata)
    assert abs(ph(T[src]) - target(wbit)) < mu // 2
    jobs = cmux.ram_write_jobs(AW, src)
    worst = 0
    for i in CELLS:
        row = ram_ref.chain(p, T, trgsw, tuple(jobs[i]))
        want = wbit if i == ADDR else int(content[i])
        err = abs(ph(row) - target(want))
        worst = max(worst, err)
        assert err < mu // 2, (i, err)
        fresh = ram_ref.blind_rotate(orc, orc.keyswitch(cmux_ref.sample_extract_index(row, 0, p.N)))   # the refresh
        assert client.decrypt_ram_trlwe(keys, fresh[None])[0] == want, i
    print(f"RAM clock: read tree phase error 2^{np.log2(max(read_err, 1)):.2f}, worst chain output 2^{np.log2(max(worst, 1)):.2f}, "
          f"bound mu/2 = 2^{np.log2(mu // 2):.0f}")


@pytest.mark.parametrize("which", ["128", "80"])
@pytest.mark.parametrize("aw", memory_cases.RAM_SHAPES)
def test_small_and_wide_rams(request, which, aw):
    """ram_ref.clock at 2 x 1 (addr_width = 1: a one-job read tree that writes the result row directly, one-step chains) and 16 x 1,
    two clocks each: a write of the complement of the addressed bit, then a wren = 0 read of the same address.  rdata and every cell
    decrypt; the chain outputs before the refresh stay below mu/2 = 2^28.  Measured worst |phase error| at coefficient 0 of the chain
    outputs over both clocks: 2^23.7 at both shapes and both sets (2^23.8 at 16 x 1 on the 80-bit set) — the noise of MUXwoSE's two
    blind rotations in the written row, which one or four more CMUXes hardly move."""
    keys, orc = request.getfixturevalue("keys" + which), request.getfixturevalue("oracle" + which)
    p = keys.params
    mu = int(p.mu)
    content, cells, clocks = memory_cases.ram_case(keys, aw)
    words = [int(b) for b in content]
    worst = 0
    trace = ram_ref.run_clocks(p, orc, cells, clocks)
    for (addr, wren, wdata, _, _), (rdata, before, new) in zip(clocks, trace):
        assert [int(b) for b in client.decrypt_bits(keys, rdata)] == [words[addr]]
        if wren:
            words[addr] = wdata
        for (_, i), row in before.items():
            ph = int(client.trlwe_phases(keys, row[None])[0][:1].view(np.int32)[0])
            err = abs(ph - (mu if words[i] else -mu))
            worst = max(worst, err)
            assert err < mu // 2, (i, err)
        assert [int(b) for b in client.decrypt_ram_trlwe(keys, new[0])] == words
    assert words[clocks[0][0]] == 1 - int(content[clocks[0][0]])   # the write landed and the second clock's wdata did not
    print(f"RAM {1 << aw} x 1, {which}-bit set: worst chain output phase error 2^{np.log2(max(worst, 1)):.2f}, bound mu/2 = 2^{np.log2(mu // 2):.0f}")
