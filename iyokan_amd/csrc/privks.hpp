// privks.hpp — private functional key switch of lvl2 TLWEs (64-bit torus) into lvl1 TRLWE rows: the second half of circuit
// bootstrapping, whose (k+1) l output rows per address bit are the rows of a TRGSW selector (iyk_hip_trgsw_from_rows).
//
// A job {in, c, out} on a lvl2 TLWE store W (u64 [slots][n_in + 1]: a[0 .. n_in-1], then b), the key K and a TRLWE store T:
//     wbar_i   = W[in][i] + 2^(63 - basebit t)                                   (mod 2^64: round to t digits)
//     d_j(i)   = (wbar_i >> (64 - (j+1) basebit)) & (2^basebit - 1)               j < t
//     T[out]   = - sum_{i <= n_in} sum_{j < t, d_j(i) != 0} K[c][i][j][d_j(i) - 1]   (mod 2^32, all 2N words)
// K: u32 [k+1][n_in+1][t][2^basebit - 1][2N], row K[c][i][j][u] a TRLWE whose phase is (u+1) 2^(32 - (j+1) basebit) sigma_i f_c(X)
// (sigma_i = s2[i], sigma_{n_in} = -1; f_1 = 1, f_0 = -s1(X)), so that T[out] has the phase f_c (b - <a, s2>) / 2^32.
//
// Integer only: every word of T[out] is a sum mod 2^32 of key words chosen by the digits, so it does not depend on the order of the
// additions — the i range of a job is split over several workgroups whose partial sums meet in T[out] by integer atomics
// (privks_zero_kernel sets the rows to 0 first, on the same stream), and the result is word for word the restatement's.
//
// privks_kernel: a workgroup of 256 lanes owns the 2N words of one (job, split), 8 words per lane as two 16-byte loads per key row —
// a row read is 8 KiB, fully coalesced.  The words of W and the digits are wave-uniform (scalar loads, scalar address math).  The rows
// of one i are fetched PRIVKS_UNROLL at a time without a branch between the loads: a zero digit reads the first row of its i again
// (a cache hit after the first) and is masked to zero — a branch around each load would make the compiler wait for every row before
// it asks for the next.  No LDS, no barrier.
//
// Replaces the key-switching half of TFHEpp's circuit bootstrapping in front of the reference's ROM / RAM ports (TaskTFHEppCB*,
// /root/reference/src/iyokan_tfhepp.hpp:194-236), restated from the published algorithm.
#pragma once
#include "goldilocks.hpp"   // IYK_HD, u32 / u64
#include "jobs.hpp"         // PrivksJob

namespace iyk {

static constexpr int PRIVKS_UNROLL = 5;    // key rows of one input word in flight per lane pair of loads (t = 10: two rounds)
static constexpr int PRIVKS_ROW_WORDS = 2 * 1024;   // 2N, N = 1024 (static_assert against NTT_N where the kernels are compiled)

// w + 2^(63 - basebit t); basebit t <= 63 (checked where a key is created)
IYK_HD u64 privks_round(u64 w, u32 t, u32 basebit) { return w + (1ull << (63u - basebit * t)); }
// digit j < t of a rounded word, most significant first
IYK_HD u32 privks_digit(u64 wbar, u32 j, u32 basebit) { return (u32)(wbar >> (64u - (j + 1u) * basebit)) & ((1u << basebit) - 1u); }

#if defined(__HIPCC__)
static_assert(PRIVKS_ROW_WORDS == 2 * NTT_N, "privks.hpp is written for N = 1024");

// T[out] = 0 for every job: the target of privks_kernel's atomics
__global__ __launch_bounds__(256) void privks_zero_kernel(const PrivksJob* __restrict__ jobs, u32* __restrict__ trlwe)
{
    uint4* row = reinterpret_cast<uint4*>(trlwe + (size_t)jobs[blockIdx.x].out * PRIVKS_ROW_WORDS);
    row[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    row[threadIdx.x + 256] = make_uint4(0u, 0u, 0u, 0u);
}

// grid: njobs * splits workgroups, workgroup b = split b % splits of job b / splits (dispatch.hpp: privks_plan)
__global__ __launch_bounds__(256) void privks_kernel(const PrivksJob* __restrict__ jobs, int splits, int i_per_split,
                                                     const u64* __restrict__ tlwe2, u32 n_words, u32 t, u32 basebit,
                                                     const u32* __restrict__ key, u32* __restrict__ trlwe)
{
    const int job = (int)(blockIdx.x / (u32)splits), split = (int)(blockIdx.x - (u32)job * (u32)splits);
    const int j_in = __builtin_amdgcn_readfirstlane(jobs[job].in), j_c = __builtin_amdgcn_readfirstlane(jobs[job].c);
    const int j_out = __builtin_amdgcn_readfirstlane(jobs[job].out);
    const u32 nb = (1u << basebit) - 1u;
    const u32 i0 = (u32)split * (u32)i_per_split, i1 = min(i0 + (u32)i_per_split, n_words);
    const u64* w = tlwe2 + (size_t)j_in * n_words;
    const size_t rows_per_i = (size_t)t * nb;                      // rows of one input word; 512 uint4 per row, 64-bit offsets throughout
    const uint4* kc = reinterpret_cast<const uint4*>(key) + (size_t)j_c * n_words * rows_per_i * 512u + threadIdx.x;

    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;               // words 4 lane .. 4 lane + 3 and 1024 + the same
    for (u32 i = i0; i < i1; ++i) {
        const u64 wi = w[i];
        const u64 wbar = privks_round(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(wi >> 32)) << 32) |
                                          (u32)__builtin_amdgcn_readfirstlane((int)(u32)wi), t, basebit);
        const uint4* ki = kc + (size_t)i * rows_per_i * 512u;
        for (u32 j0 = 0; j0 < t; j0 += PRIVKS_UNROLL) {
            uint4 a[PRIVKS_UNROLL], b[PRIVKS_UNROLL];
            u32 keep[PRIVKS_UNROLL];
#pragma unroll
            for (int u = 0; u < PRIVKS_UNROLL; ++u) {
                const u32 j = j0 + (u32)u;
                const u32 d = j < t ? privks_digit(wbar, j, basebit) : 0u;
                const size_t row = d ? (size_t)j * nb + (d - 1u) : 0;   // d == 0: row 0 of this i again, masked below
                keep[u] = d ? 0xFFFFFFFFu : 0u;
                a[u] = ki[row * 512u];
                b[u] = ki[row * 512u + 256u];
            }
#pragma unroll
            for (int u = 0; u < PRIVKS_UNROLL; ++u) {
                lo.x += a[u].x & keep[u], lo.y += a[u].y & keep[u], lo.z += a[u].z & keep[u], lo.w += a[u].w & keep[u];
                hi.x += b[u].x & keep[u], hi.y += b[u].y & keep[u], hi.z += b[u].z & keep[u], hi.w += b[u].w & keep[u];
            }
        }
    }
    u32* out = trlwe + (size_t)j_out * PRIVKS_ROW_WORDS + 4u * threadIdx.x;
    atomicAdd(out + 0, 0u - lo.x), atomicAdd(out + 1, 0u - lo.y), atomicAdd(out + 2, 0u - lo.z), atomicAdd(out + 3, 0u - lo.w);
    atomicAdd(out + 1024, 0u - hi.x), atomicAdd(out + 1025, 0u - hi.y), atomicAdd(out + 1026, 0u - hi.z), atomicAdd(out + 1027, 0u - hi.w);
}

// Scratch row g = row rows[g] of a TRLWE store: the (k+1) l rows of every selector side by side, as bk_fft_kernel reads a key step
__global__ __launch_bounds__(256) void trlwe_gather_rows_kernel(const u32* __restrict__ trlwe, const int32_t* __restrict__ rows,
                                                                u32* __restrict__ dst)
{
    const uint4* src = reinterpret_cast<const uint4*>(trlwe + (size_t)rows[blockIdx.x] * PRIVKS_ROW_WORDS);
    uint4* out = reinterpret_cast<uint4*>(dst + (size_t)blockIdx.x * PRIVKS_ROW_WORDS);
    out[threadIdx.x] = src[threadIdx.x];
    out[threadIdx.x + 256] = src[threadIdx.x + 256];
}
#endif

}  // namespace iyk
