"""ROM and RAM shapes of the CMUX memories the other tests do not run (test support for test_cmux_plan / test_ram_plan /
test_gpu_cmux_edges): ciphertexts of the client library (encrypt_rom_trlwe / encrypt_ram_trlwe / encrypt_trgsw / encrypt_bits),
deterministically from a seed — no GPU, no emulation, no reference."""
import numpy as np

from iyokan_amd import client

# (addr_width, log2_word_bits): no upper tree (data_rows = 1, the first rotate job reads a data row); a one-level tree that writes
# the result row directly; a two-level tree; 1-bit words (ten rotate steps); no rotate steps at all (1024-bit words)
ROM_SHAPES = ((3, 3), (8, 3), (9, 3), (12, 0), (2, 10))


def rom_case(keys, addr_width, log2_word_bits, seed=7):
    """A ROM of 2^addr_width words of 2^log2_word_bits bits and four reads of it: addresses 0, 1, the last and one from the middle.
    Returns (bits of the content, data TRLWEs [data_rows][2N], addresses, selectors u32 [4][addr_width][(k+1) l][k+1][N])."""
    p = keys.params
    rng = np.random.default_rng([seed, addr_width, log2_word_bits])
    bits = rng.integers(0, 2, size=(1 << addr_width) << log2_word_bits).astype(np.uint8)
    data = client.encrypt_rom_trlwe(keys, bits, seed=seed + 10)
    last = (1 << addr_width) - 1
    addresses = [0, 1, last, int(rng.integers(2, last)) if last > 2 else 2]
    abits = [[(a >> k) & 1 for k in range(addr_width)] for a in addresses]
    trgsw = client.encrypt_trgsw(keys, np.ravel(abits), seed=seed + 11).reshape(4, addr_width, p.trgsw_rows, p.k + 1, p.N)
    return bits, data, addresses, trgsw


RAM_SHAPES = (1, 4)   # addr_width of a 2 x 1 and a 16 x 1 RAM


def ram_case(keys, addr_width, seed=7):
    """A 2^addr_width x 1 RAM and two clocks on one address: a write of the complement of the addressed bit, then a read (wren = 0,
    with a wdata that must not land).  Returns (content bits, cells [1][2^addr_width][2N], [(addr, wren, wdata, selectors
    [addr_width][...], TLWEs [wren, wdata])])."""
    p = keys.params
    C = 1 << addr_width
    rng = np.random.default_rng([seed, 0x4A, addr_width])
    content = rng.integers(0, 2, size=C).astype(np.uint8)
    cells = client.encrypt_ram_trlwe(keys, content, seed=seed + 20).reshape(1, C, 2 * p.N)
    addr = C - 1 if addr_width == 1 else 0b1011
    flipped = 1 - int(content[addr])
    clocks = []
    for n, (wren, wdata) in enumerate(((1, flipped), (0, 1 - flipped))):
        trgsw = client.encrypt_trgsw(keys, [(addr >> k) & 1 for k in range(addr_width)], seed=seed + 30 + n)
        clocks.append((addr, wren, wdata, trgsw, client.encrypt_bits(keys, [wren, wdata], seed=seed + 40 + n)))
    return content, cells, clocks
