// keyswitch_mfma.hpp — the wide-batch identity key switch as an integer matrix product on the matrix cores.
//
//   out = (0,..,0,b') - sum_{i<N} sum_{j<t} KSK[i][j][v_ij - 1]  =  (0,..,0,b') - A x B   (mod 2^32)
// A[gate][k] is 1 where digit (i, j) of the gate has the value v, k = 4 (i t + j) + v (one byte of four per digit: the digit's
// one-hot form, v = 0 a padding column), B[k][word] the key rows.  A 32-bit word of B is four signed base-256 planes
// (dispatch.hpp: ks_signed_plane), so the product runs on v_mfma_i32_32x32x32_i8; per plane |sum| <= 1024 t 128 < 2^21, nothing
// overflows or is rounded, and the planes recombine with three shift-adds: every output word stays the oracle's.
// The operand B is built once per key (ks_matrix_build_kernel) in the layout of dispatch.hpp: ks_matrix_offset_k.
//
// keyswitch_mfma_kernel: a workgroup owns 256 gates (four waves of 64), 32 words (x 4 planes) and the WHOLE k range: no atomics,
// no initialisation launch.  A wave holds 2 (gate tiles) x 4 (planes) accumulator tiles; the four planes of a word are four tiles
// of the same wave, so the same lane and register hold all four.  B is streamed through LDS, two k-steps (8 KB) per barrier, read
// as one 16-byte fragment per lane; a gate's digits are staged per block of 16 coefficients in the wave's own LDS slice, four
// digits per byte, and expanded to one-hot bytes in registers (1 << 8 v per digit).  The instruction's k order inside a step
// never matters: both operands are laid out by the same (lane half, element) -> k map.
#pragma once
#include <hip/hip_runtime.h>

#include "dispatch.hpp"
#include "kernels.hpp"

namespace iyk {

typedef int ksm_i32x4 __attribute__((ext_vector_type(4)));
typedef int ksm_i32x16 __attribute__((ext_vector_type(16)));

static constexpr int KSM_IB = 16;        // coefficients per digit block: 4 groups of 4 per gate, one (gate, group) per lane and pass
static constexpr int KSM_DIG_ROW = 36;   // bytes per gate of a digit block: 4 t digit bytes, padded to an odd number of dwords (banks)
static constexpr int KSM_PHASE_BYTES = 2 * (int)dispatch::KS_MATRIX_CHUNK_BYTES;   // two k-steps of B per barrier
static constexpr size_t KSM_LDS_BYTES = 2 * (size_t)KSM_PHASE_BYTES + (size_t)dispatch::KS_MATRIX_GATES * KSM_DIG_ROW;

// One workgroup per chunk of the operand (word group, k-step), one thread per 16 bytes: plane = thread / 64, lane = thread % 64.
// Padding (v = 0, words past the row) is written as zeros, so the operand needs no memset.
template <int T>
__global__ __launch_bounds__(256) void ks_matrix_build_kernel(const u32* __restrict__ ksk, unsigned char* __restrict__ mat, u32 stride)
{
    constexpr int STEPS = dispatch::ks_matrix_ksteps(T);
    const int wg = blockIdx.x / STEPS, s = blockIdx.x % STEPS;
    const int p = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5;
    const u32 word = (u32)wg * dispatch::KS_MATRIX_WORDS + (u32)(lane & 31);
    const int k0 = 32 * s + 16 * h;
    u32 out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int k = k0 + e, v = k & 3, f = k >> 2;   // f = i t + j
        int b = 0;
        if (v != 0 && word < stride) b = dispatch::ks_signed_plane(ksk[((size_t)f * 3 + (size_t)(v - 1)) * stride + word], p);
        out[e >> 2] |= ((u32)b & 0xFFu) << (8 * (e & 3));
    }
    static_assert(dispatch::ks_matrix_offset_k(T, 16, 0, 0) % 16 == 0 && dispatch::ks_matrix_offset_k(T, 17, 5, 2) == dispatch::ks_matrix_offset_k(T, 16, 5, 2) + 1,
                  "16 consecutive k of a column are 16 consecutive bytes");
    *reinterpret_cast<uint4*>(mat + dispatch::ks_matrix_offset_k(T, k0, (int)word, p)) = make_uint4(out[0], out[1], out[2], out[3]);
}

template <int T, int NC>
__global__ __launch_bounds__(256, 2) void keyswitch_mfma_kernel(const u32* __restrict__ rot, const KsJob* __restrict__ jobs, int njobs,
                                                                const unsigned char* __restrict__ mat, u32* __restrict__ arena, u32 n)
{
    using namespace dispatch;
    constexpr u32 dbits = 2u * T, prec = 1u << (32 - (1 + dbits));
    constexpr int PH = T;                            // phases (pairs of k-steps) per digit block: KSM_IB t digits / 16
    constexpr int BLOCKS = NTT_N / KSM_IB;
    constexpr int PHASES = ks_matrix_ksteps(T) / 2;
    constexpr int ITEMS = 64 * (KSM_IB / 4) / 64;    // (gate, group of 4 coefficients) per lane and block
    static_assert(KS_MATRIX_GATES == 256 && KS_MATRIX_WAVE_GATES == 64 && KS_MATRIX_WORDS == 32, "the kernel's tiling");
    static_assert(PH * BLOCKS == PHASES && 4 * T <= KSM_DIG_ROW - 4 && (KSM_DIG_ROW / 4) % 2 == 1, "digit blocks");
    static_assert(ks_matrix_word_groups(NC) * KS_MATRIX_WORDS == NC * 128, "word groups cover the padded row");
    // the fragment a lane reads below is what the layout function says: plane tiles of 1 KB, 16 bytes per lane, chunks in k order
    static_assert(ks_matrix_offset_k(T, 32 + 16, 32 + 5, 3) == ks_matrix_chunk_offset(T, 1, 1) + 3 * KS_MATRIX_TILE_BYTES + (32 + 5) * 16 &&
                      ks_matrix_chunk_offset(T, 0, 1) == KS_MATRIX_CHUNK_BYTES,
                  "layout of the operand");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ksm[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    unsigned char* s_dig = smem_ksm + 2 * KSM_PHASE_BYTES + wave * (KS_MATRIX_WAVE_GATES * KSM_DIG_ROW);   // this wave's [64][KSM_DIG_ROW]
    const int gbase = blockIdx.x * KS_MATRIX_GATES + wave * KS_MATRIX_WAVE_GATES;
    const uint4* src = reinterpret_cast<const uint4*>(mat + ks_matrix_chunk_offset(T, (int)blockIdx.y, 0)) + threadIdx.x;

    // digit staging: item `it` of a lane is gate it * 16 + lane / 4 of the wave, coefficients 4 (lane % 4) .. + 3 of the block
    int row_a[ITEMS], row_b[ITEMS];   // rows of `rot`; row_b = -1: no second row; row_a = -1: no such gate (digits 0)
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int gi = gbase + it * 16 + (lane >> 2);
        const KsJob jb = jobs[gi < njobs ? gi : njobs - 1];
        row_a[it] = gi < njobs ? jb.ra : -1;
        row_b[it] = gi < njobs ? jb.rb : -1;
    }
    u32 pa[ITEMS][4], pb[ITEMS][4];
    auto dig_load = [&](int blk) {
        const u32 i = (u32)(blk < BLOCKS ? blk : BLOCKS - 1) * KSM_IB + 4u * (u32)(lane & 3);
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const u32* qa = rot + (size_t)(row_a[it] >= 0 ? row_a[it] : 0) * (NTT_N + 1) + i;
            const u32* qb = rot + (size_t)(row_b[it] >= 0 ? row_b[it] : 0) * (NTT_N + 1) + i;
#pragma unroll
            for (int c = 0; c < 4; ++c) pa[it][c] = qa[c], pb[it][c] = qb[c];
        }
    };
    auto dig_store = [&]() {
        lds_sync();
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            unsigned long long x = 0;   // the 4 x 2 t digit bits, most significant first: t bytes of 4 digits
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const u32 a = pa[it][c] + (row_b[it] >= 0 ? pb[it][c] : 0u) + prec;
                x = (x << dbits) | (unsigned long long)(row_a[it] >= 0 ? a >> (32 - dbits) : 0u);
            }
            unsigned char* q = s_dig + (it * 16 + (lane >> 2)) * KSM_DIG_ROW + (lane & 3) * T;
#pragma unroll
            for (int m = 0; m < T; ++m) q[m] = (unsigned char)(x >> (8 * (T - 1 - m)));
        }
        lds_sync();
    };

    uint4 pf0, pf1;
    auto b_load = [&](int q) {
        const uint4* s = src + (size_t)(q < PHASES ? q : PHASES - 1) * (KSM_PHASE_BYTES / 16);
        pf0 = s[0], pf1 = s[256];
    };
    auto b_store = [&](int q) {
        uint4* d = reinterpret_cast<uint4*>(smem_ksm + (q & 1) * KSM_PHASE_BYTES) + threadIdx.x;
        d[0] = pf0, d[256] = pf1;
    };

    ksm_i32x16 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mt][p][e] = 0;

    b_load(0);
    dig_load(0);
    b_store(0);
    b_load(1);
    dig_store();
    wg_barrier_lds();

    int q = 0;
#pragma unroll 1
    for (int blk = 0; blk < BLOCKS; ++blk) {
        dig_load(blk + 1);   // consumed at the end of this block
#pragma unroll 1
        for (int ph = 0; ph < PH; ++ph, ++q) {
            const unsigned char* bq = smem_ksm + (q & 1) * KSM_PHASE_BYTES + lane * 16;
            u32 d[2];   // bytes 2 ss + h: the four digits of this lane's half of k-step ss, for the gates r and 32 + r
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) d[mt] = *reinterpret_cast<const u32*>(s_dig + (mt * 32 + r) * KSM_DIG_ROW + 4 * ph);
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                ksm_i32x4 a[2];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const u32 b = d[mt] >> (8 * (2 * ss + h));
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[mt][e] = (int)(1u << (((b >> (6 - 2 * e)) & 3u) << 3));
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const ksm_i32x4 bf = *reinterpret_cast<const ksm_i32x4*>(bq + ss * (int)KS_MATRIX_CHUNK_BYTES + p * (int)KS_MATRIX_TILE_BYTES);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[mt][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[mt], bf, acc[mt][p], 0, 0, 0);
                }
            }
            b_store(q + 1);   // into the buffer everybody left at the previous barrier
            b_load(q + 2);
            wg_barrier_lds();
        }
        dig_store();
    }

    // C/D map of the 32 x 32 tile: column (word) = lane % 32, row (gate) = (reg % 4) + 8 (reg / 4) + 4 (lane / 32)
    const u32 word = blockIdx.y * (u32)KS_MATRIX_WORDS + (u32)r;
    if (word > n) return;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int gi = gbase + mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (gi >= njobs) continue;
            const KsJob jb = jobs[gi];
            u32 base = 0u;
            if (word == n)
                base = rot[(size_t)jb.ra * (NTT_N + 1) + NTT_N] + (jb.rb >= 0 ? rot[(size_t)jb.rb * (NTT_N + 1) + NTT_N] : 0u) + jb.off;
            const u32 sum = (u32)acc[mt][0][e] + ((u32)acc[mt][1][e] << 8) + ((u32)acc[mt][2][e] << 16) + ((u32)acc[mt][3][e] << 24);
            arena[(size_t)jb.out * ((size_t)n + 1) + word] = base - sum;
        }
}

}  // namespace iyk
