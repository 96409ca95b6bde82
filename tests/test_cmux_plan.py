"""iyokan_amd.cmux.rom_read_plan: structure of the launches, and one ROM read computed with the exact reference of tests/cmux_ref.py
(no GPU, no emulation) decrypting to the ROM's content — the noise check of the CMUX tree."""
import numpy as np
import pytest

import cmux_ref
import memory_cases
from iyokan_amd import client, cmux

ADDR_WIDTH, LOG2_WORD_BITS = 10, 3          # 8 TRLWEs x 1024 bits, 8-bit words: 1024 words
ADDRESSES = [0, 1, 127, 128, 1023] + [int(a) for a in np.random.default_rng(5).integers(0, 1024, size=3)]


@pytest.mark.parametrize("aw,lw", [(10, 3), (7, 3), (3, 3), (12, 0), (4, 10), (11, 5)])
def test_plan_structure(aw, lw):
    N = 1024
    lay = cmux.rom_layout(aw, lw, N)
    plan = cmux.rom_read_plan(aw, lw, N)
    W = lay.log2_words
    upper = max(aw - W, 0)
    assert lay.data_rows == 1 << upper
    written = set()
    for b, jobs in enumerate(plan):
        outs = [j.out for j in jobs]
        assert len(set(outs)) == len(outs)
        for j in jobs:
            ins = [j.in0] + ([j.in1] if j.in1 >= 0 else [])
            for r in ins + [j.out]:
                assert 0 <= r < lay.data_rows + lay.scratch_rows
            assert j.out >= lay.data_rows                                     # the ROM's rows are never written
            assert all(r < lay.data_rows or r in written for r in ins)       # data rows or outputs of an EARLIER launch
            others = [k for k in jobs if k is not j]
            assert all(j.out not in (k.in0, k.in1, k.out) for k in others)    # the independence contract of cmux_batch
            assert 0 <= j.bit < aw
        written.update(outs)
        if b < upper:   # upper tree
            assert len(jobs) == 1 << (upper - 1 - b)
            assert all(j.in1 >= 0 and j.bit == W + b for j in jobs)
        else:           # one rotate-form job per low address bit
            bit = b - upper + 1 + max(W - aw, 0)
            assert len(jobs) == 1 and jobs[0].in1 < 0 and jobs[0].rot == 2 * N - (N >> bit) and jobs[0].bit == W - bit
    assert len(plan) == upper + min(W, aw)
    if plan:
        assert plan[-1][0].out == lay.result
    assert sorted(j.bit for jobs in plan for j in jobs[:1]) == list(range(aw))


@pytest.fixture(scope="module")
def rom(keys128):
    rng = np.random.default_rng(77)
    content = rng.integers(0, 256, size=1 << ADDR_WIDTH).astype(np.uint8)
    bits = np.unpackbits(content[:, None], axis=1, bitorder="little").ravel()     # bit i of word w at coefficient 8 w + i
    return content, client.encrypt_rom_trlwe(keys128, bits, seed=31)


def test_rom_read_decrypts_with_margin(keys128, rom):
    """One read per address through the exact reference.  Measured (128-bit set, 3 CMUX levels + 7 rotate steps, fresh selectors):
    worst |phase error| over the 8 addresses x 8 bits = 2^20.8 against the bound mu/2 = 2^28: a margin of 7.2 bits."""
    p = keys128.params
    content, data = rom
    lay = cmux.rom_layout(ADDR_WIDTH, LOG2_WORD_BITS, p.N)
    plan = cmux.rom_read_plan(ADDR_WIDTH, LOG2_WORD_BITS, p.N)
    assert data.shape[0] == lay.data_rows == 8
    worst = 0
    for n, addr in enumerate(ADDRESSES):
        abits = [(addr >> k) & 1 for k in range(ADDR_WIDTH)]
        trgsw = client.encrypt_trgsw(keys128, abits, seed=100 + n)
        T = np.concatenate([data, np.zeros((lay.scratch_rows, 2 * p.N), dtype=np.uint32)])
        for jobs in plan:
            cmux_ref.run_jobs(p, T, trgsw, [(j.bit, j.in0, j.in1, j.rot, j.out) for j in jobs])
        ph = client.trlwe_phases(keys128, T[lay.result : lay.result + 1])[0][:8].view(np.int32).astype(np.int64)
        want = np.array([(int(content[addr]) >> i) & 1 for i in range(8)])
        err = np.abs(ph - np.where(want == 1, int(p.mu), -int(p.mu)))
        worst = max(worst, int(err.max()))
        assert err.max() < p.mu // 2, (addr, err.max())
        assert np.array_equal((ph > 0).astype(int), want), addr
    print(f"ROM read: worst phase error 2^{np.log2(max(worst, 1)):.2f}, bound mu/2 = 2^{np.log2(p.mu // 2):.0f}")


@pytest.mark.parametrize("which", ["128", "80"])
@pytest.mark.parametrize("aw,lw", memory_cases.ROM_SHAPES)
def test_rom_shapes_decrypt_with_margin(request, which, aw, lw):
    """Companion of test_rom_read_decrypts_with_margin at the shapes it does not run: no upper tree, a one-level tree, a two-level
    one, 1-bit words (2 levels + 10 rotate steps, the deepest plan) and 1024-bit words (no rotate step); addresses 0, 1, last and one
    from the middle, through the exact reference.  Measured worst |phase error| over the 4 addresses x word bits, bound mu/2 = 2^28:
        shape      128-bit set   80-bit set
        (3, 3)     2^20.1        2^20.3
        (8, 3)     2^20.3        2^21.0
        (9, 3)     2^20.6        2^20.9
        (12, 0)    2^19.9        2^20.9
        (2, 10)    2^20.1        2^20.8
    At (2, 10) every coefficient index h in [0, N) of cmux_ref.sample_extract_index is checked by decryption: the phase of the
    extracted TLWE under the lvl1 key is exactly coefficient h of the TRLWE's phase."""
    keys = request.getfixturevalue("keys" + which)
    p = keys.params
    bits, data, addresses, trgsw = memory_cases.rom_case(keys, aw, lw)
    wb = 1 << lw
    assert data.shape[0] == cmux.rom_layout(aw, lw, p.N).data_rows
    s1 = keys.s1.astype(np.int64)
    worst = 0
    for r, addr in enumerate(addresses):
        row = cmux_ref.rom_read(p, data, trgsw[r], aw, lw)
        ph = client.trlwe_phases(keys, row[None])[0][:wb].view(np.int32).astype(np.int64)
        want = bits[addr * wb : (addr + 1) * wb].astype(np.int64)
        err = np.abs(ph - np.where(want == 1, int(p.mu), -int(p.mu)))
        worst = max(worst, int(err.max()))
        assert err.max() < p.mu // 2, (addr, err.max())
        assert np.array_equal((ph > 0).astype(np.int64), want), addr
        if wb == p.N:
            for h in range(p.N):
                t = cmux_ref.sample_extract_index(row, h, p.N).astype(np.int64)
                phase = (int(t[p.N]) - int(t[: p.N] @ s1)) & cmux_ref.M32
                assert phase == int(ph[h]) & cmux_ref.M32, (addr, h)
    print(f"ROM read ({aw}, {lw}), {which}-bit set: worst phase error 2^{np.log2(max(worst, 1)):.2f}, bound mu/2 = 2^{np.log2(p.mu // 2):.0f}")
