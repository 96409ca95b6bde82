"""Inputs shared by test_privks_ref (CPU: the restatement, and the noise measurement of the end-to-end case) and test_gpu_privks (the
same case on the GPU): one construction, so that what is measured is what is run."""
import numpy as np

from iyokan_amd import client

T_CB, BASEBIT_CB = 10, 3           # TFHEpp's lvl21 key-switch parameters (tests/shims/tfhe++.hpp)
ALPHA2 = 2.0 ** -44                # noise of the lvl2 inputs: TFHEpp's lvl2param alpha

E2E_N_IN, E2E_ADDR_WIDTH, E2E_LOG2_WORD_BITS = 64, 3, 10   # a ROM of 8 TRLWE rows, one word of N bits each


_CACHE = {}


def _e2e(keys):
    p = keys.params
    s2 = client.keygen_lvl2(E2E_N_IN, seed=21)
    key_rows = client.privks_key_rows(keys, s2, T_CB, BASEBIT_CB, seed=22)
    rng = np.random.default_rng(23)
    content = rng.integers(0, 2, size=(1 << E2E_ADDR_WIDTH, p.N)).astype(np.uint8)
    data = client.encrypt_rom_trlwe(keys, content.ravel(), seed=24)
    addr_bits = np.array([[(a >> b) & 1 for b in range(E2E_ADDR_WIDTH)] for a in range(1 << E2E_ADDR_WIDTH)])
    tlwe2 = client.encrypt_cb_digits(s2, addr_bits.ravel(), p, ALPHA2, seed=25)   # [address][bit][r]
    return dict(keys=keys, s2=s2, key_rows=key_rows, content=content, data=data, tlwe2=tlwe2)


def e2e_case(name, keys):
    """The end-to-end case of parameter set `name` (keys: the session's keys128 / keys80): a real lvl2 key and private key-switching key at n_in = 64, a ROM of 8 rows of N
    random bits, and for every address 0 .. 7 the 3 l lvl2 TLWEs of its bits (TLWE (address 3 + bit) l + r)."""
    if name not in _CACHE:
        _CACHE[name] = _e2e(keys)
    return _CACHE[name]


def e2e_reference_row(case, p, addr):
    """The result row of reading address `addr`: selectors restated with privks_ref from the address's lvl2 TLWEs, the read through
    cmux_ref's exact CMUX.  Cached: the CPU measurement and the GPU comparison share it."""
    import cmux_ref
    import privks_ref as ref

    memo = case.setdefault("rows", {})
    if addr not in memo:
        A, l = E2E_ADDR_WIDTH, p.l
        tl = case["tlwe2"].reshape(1 << A, A, l, E2E_N_IN + 1)
        row_fn = ref.key_rows_of(case["key_rows"])
        trgsw = np.stack([ref.selector_rows(tl[addr, b], T_CB, BASEBIT_CB, row_fn, l) for b in range(A)])
        memo[addr] = cmux_ref.rom_read(p, case["data"], trgsw, A, E2E_LOG2_WORD_BITS)
    return memo[addr]
