"""CPU: the RAM write chain under selectors made by circuit bootstrapping, real keys, 128-bit set — the smallest RAM (2-bit address, one
plane), both wren values.  Selectors: the lvl0 -> lvl2 rotation's words under a real bk2 at n = 636 (the kernel's emulation, held word for
word to cb_rotate_ref by test_cb_rotate_emul.py) through privks_ref's row selection on a real private key-switching key (n_in = 2048,
t = 10, basebit = 3, made in windows); then ram_ref.clock — exact CMUXes, the oracle's rotations and key switch.  The worst phase error of
the chain's outputs (before the refresh) and of rdata is printed; DESIGN.md section 6d's table has the figures.  What is asserted is that
nothing misreads: rdata, the chain outputs and the refreshed cells decrypt to the RAM's meaning."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cb_rotate_cases
import cb_rotate_ref
import ram_ref
from iyokan_amd import client
from test_cb_rotate_ref import _switch_windowed

A, CELLS, ADDR, WDATA = 2, [1, 0, 0, 1], 2, 1


def _err(phase, bit, mu):
    want = mu if bit else -mu
    return abs(int((int(phase) - want + (1 << 31)) % (1 << 32) - (1 << 31)))


def test_ram_clock_under_circuit_bootstrapped_selectors(keys128, oracle128):
    keys, orc, p = keys128, oracle128, keys128.params
    l, N, mu = int(p.l), int(p.N), int(p.mu)
    s2 = client.keygen_lvl2(cb_rotate_cases.N2, seed=31)
    ntt = cb_rotate_cases.key_ntt(client.bk2_rows(keys, s2, 4, 9, cb_rotate_cases.ALPHA2, seed=32))
    addr = client.encrypt_bits(keys, [(ADDR >> b) & 1 for b in range(A)], seed=61)
    jobs = [(addr[b], cb_rotate_ref.mu_of(r, p.Bgbit)) for b in range(A) for r in range(l)]
    with ThreadPoolExecutor(max_workers=6) as pool:
        tl = np.stack(list(pool.map(lambda j: cb_rotate_cases.emul_rotate(j[0], 1, 0, j[1], ntt), jobs)))
    rows = _switch_windowed(keys, s2, tl, [(i, c) for i in range(A * l) for c in range(p.k + 1)], 10, 3, seed=41)
    trgsw = rows.reshape(A, l, p.k + 1, 2, N).transpose(0, 2, 1, 3, 4).reshape(A, (p.k + 1) * l, 2, N)   # row c l + r of every bit
    cells = client.encrypt_ram_trlwe(keys, CELLS, seed=62).reshape(1, 1 << A, 2 * N)
    worst_chain = worst_rdata = worst_cell = 0
    for wren in (0, 1):
        cts = client.encrypt_bits(keys, [wren, WDATA], seed=63 + wren)
        rdata, before, new = ram_ref.clock(p, orc, cells, trgsw, cts[0], cts[1:])
        want = list(CELLS)
        if wren:
            want[ADDR] = WDATA
        assert list(client.decrypt_bits(keys, rdata)) == [CELLS[ADDR]], wren
        worst_rdata = max(worst_rdata, _err(client.phases(keys, rdata)[0], CELLS[ADDR], mu))
        chain = np.stack([before[(0, i)] for i in range(1 << A)])
        assert list(client.decrypt_ram_trlwe(keys, chain)) == want, wren
        ph = client.trlwe_phases(keys, chain)[:, 0]
        worst_chain = max([worst_chain] + [_err(ph[i], want[i], mu) for i in range(1 << A)])
        assert list(client.decrypt_ram_trlwe(keys, new[0])) == want, wren
        ph = client.trlwe_phases(keys, new[0])[:, 0]
        worst_cell = max([worst_cell] + [_err(ph[i], want[i], mu) for i in range(1 << A)])
    for what, v in (("rdata TLWE", worst_rdata), ("chain output, coefficient 0, before the refresh", worst_chain), ("cell after the refresh", worst_cell)):
        print(f"worst phase error, {what}: 2^{np.log2(max(v, 1)):.2f} of mu = 2^{np.log2(mu):.0f}: {np.log2(mu) - np.log2(max(v, 1)):.2f} bits")
