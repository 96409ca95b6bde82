// key_expand.hpp — the masks of the seeded evaluation keys: ONE generator, compiled as the same text by the client library
// (client.cpp), the kernel's emulation (emul.cpp), the host self-test (host_selftest.cpp) and the kernel (iyokan_hip.hip).
//
// Half of every row of the private key-switching key and of the lvl2 bootstrapping key, the polynomial a, is uniformly random and
// says nothing about a secret key.  A seeded key is the b halves plus a PUBLIC 256-bit mask seed; the a halves are regenerated where
// they are needed.  The mask of a row is a pure function of (mask_seed, kind, row, word offset): the ChaCha20 block function of
// RFC 8439 (20 rounds, 32-bit block counter) on the state
//
//   words  0 ..  3   "expand 32-byte k"
//   words  4 .. 11   mask_seed, 32 bytes, as eight little-endian u32
//   word  12         block index inside the row's mask: block q gives the mask's u32 words 16 q .. 16 q + 15
//   word  13, 14     row index, low and high 32 bits
//   word  15         kind: 1 = private key-switching key, 2 = lvl2 bootstrapping key
//
// row is the HOST row index of the existing calls: ((c (n_in+1) + i) t + j) (2^basebit - 1) + u of the private key (N u32 words, 64
// blocks a row), step (k+1) l2 + r of the lvl2 key (N2 u64 words with a[m] = w[2m] | w[2m+1] << 32, which is the order of the u32 words
// in memory: 256 blocks a row).  Nothing else is drawn from this stream: noise and everything secret come from the client's private
// generator.  A mask seed is public and must be fresh per key (two keys on one seed share their masks row for row).
//
// No HIP call, no global, no include beyond <cstdint> / <cstring>: the kernel at the end is the only text under __HIPCC__.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define IYK_KX_HD __host__ __device__ inline
#else
#define IYK_KX_HD inline
#endif

namespace iyk {
namespace kx {

constexpr uint32_t KIND_PRIVKS = 1;    // state word 15
constexpr uint32_t KIND_BK2 = 2;
constexpr uint32_t BLOCK_WORDS = 16;   // u32 words of one ChaCha20 block: what one lane writes

IYK_KX_HD uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }   // v_alignbit_b32 on the device

// out = ChaCha20 block function of the state `in` (RFC 8439 §2.3); out may not alias in
IYK_KX_HD void chacha20_block(const uint32_t in[16], uint32_t out[16])
{
    uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7];
    uint32_t x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
#define IYK_KX_QR(a, b, c, d)                                                   \
    a += b; d = rotl32(d ^ a, 16); c += d; b = rotl32(b ^ c, 12);               \
    a += b; d = rotl32(d ^ a, 8);  c += d; b = rotl32(b ^ c, 7);
    for (int r = 0; r < 10; ++r) {
        IYK_KX_QR(x0, x4, x8, x12) IYK_KX_QR(x1, x5, x9, x13) IYK_KX_QR(x2, x6, x10, x14) IYK_KX_QR(x3, x7, x11, x15)
        IYK_KX_QR(x0, x5, x10, x15) IYK_KX_QR(x1, x6, x11, x12) IYK_KX_QR(x2, x7, x8, x13) IYK_KX_QR(x3, x4, x9, x14)
    }
#undef IYK_KX_QR
    out[0] = x0 + in[0], out[1] = x1 + in[1], out[2] = x2 + in[2], out[3] = x3 + in[3];
    out[4] = x4 + in[4], out[5] = x5 + in[5], out[6] = x6 + in[6], out[7] = x7 + in[7];
    out[8] = x8 + in[8], out[9] = x9 + in[9], out[10] = x10 + in[10], out[11] = x11 + in[11];
    out[12] = x12 + in[12], out[13] = x13 + in[13], out[14] = x14 + in[14], out[15] = x15 + in[15];
}

// state of (key, counter, three nonce words): the layout of RFC 8439 §2.3
IYK_KX_HD void chacha20_state(const uint32_t key[8], uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t st[16])
{
    st[0] = 0x61707865u, st[1] = 0x3320646eu, st[2] = 0x79622d32u, st[3] = 0x6b206574u;
    for (int i = 0; i < 8; ++i) st[4 + i] = key[i];
    st[12] = counter, st[13] = n0, st[14] = n1, st[15] = n2;
}

struct MaskKey {
    uint32_t w[8];   // the mask seed as eight little-endian u32
};

inline MaskKey mask_key_of(const uint8_t seed[32])
{
    MaskKey k;
    for (int i = 0; i < 8; ++i)
        k.w[i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 | (uint32_t)seed[4 * i + 3] << 24;
    return k;
}

// mask words 16 block .. 16 block + 15 of row `row` of a key of kind `kind`
IYK_KX_HD void mask_block(const MaskKey& key, uint32_t kind, uint64_t row, uint32_t block, uint32_t out[16])
{
    uint32_t st[16];
    chacha20_state(key.w, block, (uint32_t)row, (uint32_t)(row >> 32), kind, st);
    chacha20_block(st, out);
}

// words [0, words) of the mask of one row: the host side (client.cpp); a last block may be cut
inline void mask_row(const MaskKey& key, uint32_t kind, uint64_t row, uint64_t words, uint32_t* out)
{
    uint32_t blk[16];
    for (uint64_t q = 0; q * BLOCK_WORDS < words; ++q) {
        mask_block(key, kind, row, (uint32_t)q, blk);
        const uint64_t n = words - q * BLOCK_WORDS < BLOCK_WORDS ? words - q * BLOCK_WORDS : BLOCK_WORDS;
        std::memcpy(out + q * BLOCK_WORDS, blk, n * sizeof(uint32_t));
    }
}

// ---- the kernel's lane -----------------------------------------------------------------------------------------------------------
// A window of row_count rows whose polynomials lie row_stride u32 words apart in the destination, a first: lane g writes block
// g % blocks_per_row of the mask of row first_row + g / blocks_per_row as four 16-byte stores to consecutive addresses, and moves the
// same 64 bytes of the window's b halves (src_b: u32 [row_count][16 blocks_per_row], as the client sent them) to b_offset words behind
// them.  Every address is inside [dst, dst + row_count row_stride): g < row_count blocks_per_row is the caller's loop bound, and
// 16 blocks_per_row + b_offset <= row_stride is checked where the arguments are made (expand_args_ok).
struct ExpandArgs {
    MaskKey key;
    uint32_t kind;
    uint32_t blocks_per_row;
    uint64_t first_row;     // HOST row index of the window's first row
    uint64_t row_count;
    uint64_t row_stride;    // u32 words from one destination row to the next
    uint64_t b_offset;      // u32 words from a row's a to its b
};

inline bool expand_args_ok(const ExpandArgs& A)
{
    const uint64_t poly = (uint64_t)A.blocks_per_row * BLOCK_WORDS;
    return A.blocks_per_row > 0 && A.row_count > 0 && A.row_stride % 4 == 0 && A.b_offset % 4 == 0 && A.b_offset >= poly &&
           A.b_offset + poly <= A.row_stride && A.row_count <= UINT64_MAX / A.row_stride;
}

// rows [first_row, first_row + row_count) of the private key-switching key in its device layout, u32 [rows][a: N][b: N]
inline ExpandArgs privks_expand_args(const MaskKey& key, uint64_t first_row, uint64_t row_count, uint32_t N)
{
    return ExpandArgs{key, KIND_PRIVKS, N / BLOCK_WORDS, first_row, row_count, 2ull * N, N};
}
// rows [first_row, ...) of the lvl2 bootstrapping key's staged torus-domain window, u64 [rows][a: N2][b: N2], in u32 words
inline ExpandArgs bk2_expand_args(const MaskKey& key, uint64_t first_row, uint64_t row_count, uint32_t N2)
{
    return ExpandArgs{key, KIND_BK2, 2 * N2 / BLOCK_WORDS, first_row, row_count, 4ull * N2, 2ull * N2};
}

struct alignas(16) W4 {
    uint32_t x, y, z, w;
};
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t w4_vec __attribute__((ext_vector_type(4)));   // one value to the compiler: a 16-byte access stays one, and aligned
#endif
IYK_KX_HD void store4(uint32_t* p, const W4& v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<w4_vec*>(p) = w4_vec{v.x, v.y, v.z, v.w};
#else
    std::memcpy(p, &v, sizeof v);
#endif
}
IYK_KX_HD W4 load4(const uint32_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const w4_vec v = *reinterpret_cast<const w4_vec*>(p);
    return W4{v.x, v.y, v.z, v.w};
#else
    W4 v;
    std::memcpy(&v, p, sizeof v);
    return v;
#endif
}

IYK_KX_HD void expand_lane(const ExpandArgs& A, uint64_t g, uint32_t* dst, const uint32_t* src_b)
{
    const uint64_t r = g / A.blocks_per_row;
    const uint32_t q = (uint32_t)(g - r * A.blocks_per_row);
    uint32_t w[16];
    mask_block(A.key, A.kind, A.first_row + r, q, w);
    uint32_t* a = dst + r * A.row_stride + (uint64_t)q * BLOCK_WORDS;
    const uint32_t* s = src_b + g * BLOCK_WORDS;
    const W4 b0 = load4(s), b1 = load4(s + 4), b2 = load4(s + 8), b3 = load4(s + 12);
    store4(a, W4{w[0], w[1], w[2], w[3]});
    store4(a + 4, W4{w[4], w[5], w[6], w[7]});
    store4(a + 8, W4{w[8], w[9], w[10], w[11]});
    store4(a + 12, W4{w[12], w[13], w[14], w[15]});
    uint32_t* b = a + A.b_offset;
    store4(b, b0), store4(b + 4, b1), store4(b + 8, b2), store4(b + 12, b3);
}

constexpr int EXPAND_THREADS = 256;
constexpr int EXPAND_WG_PER_CU = 16;   // the grid's cap: a longer window strides

// workgroups of a launch over `blocks` lanes on a device of `cus` compute units
inline uint32_t expand_grid(uint64_t blocks, int cus)
{
    const uint64_t want = (blocks + EXPAND_THREADS - 1) / EXPAND_THREADS;
    const uint64_t cap = (uint64_t)EXPAND_WG_PER_CU * (uint64_t)(cus > 0 ? cus : 1);
    return (uint32_t)(want < cap ? want : cap);
}

#if defined(__HIPCC__)
// One lane per 64-byte block of the window's masks, grid-stride.  dst: the window's first destination row (the key's store, or the
// staged torus-domain window of the lvl2 key); src_b: the window's b halves on the device.  A streaming write of as many bytes as the
// transfer it replaces: no LDS, no barrier.
__global__ __launch_bounds__(EXPAND_THREADS) void key_mask_expand_kernel(const ExpandArgs A, uint32_t* __restrict__ dst,
                                                                         const uint32_t* __restrict__ src_b)
{
    const uint64_t total = A.row_count * A.blocks_per_row;
    const uint64_t step = (uint64_t)gridDim.x * EXPAND_THREADS;
    for (uint64_t g = (uint64_t)blockIdx.x * EXPAND_THREADS + threadIdx.x; g < total; g += step) expand_lane(A, g, dst, src_b);
}
#endif

}  // namespace kx
}  // namespace iyk
