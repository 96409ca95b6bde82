// cb_rotate_lat.hpp — the narrow-batch (latency) form of the lvl0 -> lvl2 blind rotation of cb_rotate.hpp: the same job, the same key
// (u64 [n][2 halves][8 rows][2][N2], natural order), the same arithmetic in Z_P and therefore the same output words, bit for bit.
// cb_rotate_kernel stays the wide-batch form and the cross-check; dispatch::cb_plan chooses per batch.
//
// What differs is the schedule.  One workgroup of 512 lanes (8 waves, two per SIMD) per rotation:
//   forward   wave v owns digit polynomial v = 4 h + lvl (accumulator polynomial h, digit level lvl) and LDS slot v.  Pass 1 (lane = j1 <
//             64, the 32-point negacyclic pass over j2), the exchange and pass 2 all stay inside the wave: a wave-level ordering point,
//             no workgroup barrier.  Pass 2 is the 64-point pass over j1 with its first butterfly stage folded into the read: lane
//             (k2, half) reads Y[j1] and Y[j1 + 32], keeps Y[j1] + Y[j1 + 32] (half 0: the even k1) or (Y[j1] - Y[j1 + 32]) 2^(3 j1)
//             (half 1: the odd k1) and runs ntt32_dif<6> — 64 lanes x 32 points, every lane busy, shifts only.
//   multiply  all 8 spectra are live in LDS (slot v, natural order): every lane takes 4 points (k = 2 lane + 1024 q + e) of the 8 rows
//             into 16 running sums (2 output polynomials x 2 key halves x 4 points).
//   inverse   product o = 2 c + half is owned by wave o < 4 (one per SIMD) and slot o: pass 1' (the 64-point pass over k1 with the same
//             folded first stage), the exchange and pass 2' inside the wave; then the lifted words are added into the accumulator by
//             64-bit LDS atomics (the lo and the hi << 32 part of a word come from two waves; integer adds commute).
//   key       the 8 operands of row 0 of the NEXT step (32 VGPRs) are requested before the inverse transforms and consumed by the next
//             multiply; abar of the next step is read one step ahead.
// Workgroup barriers per step: 4 (spectra complete / spectra consumed / sums in their slots / accumulator complete), against 14.
// LDS: acc 32 KiB + 8 slots x 2048 u64 (128 KiB) = 160 KiB of 160.  The slots carry no padding: the exchanges are XOR-swizzled
// (forward Y[j1][k2] at k2 * 64 + (j1 ^ k2), inverse Z[k2][j1] at j1 * 32 + (k2 ^ (j1 & 31))), conflict-free on both sides.  The
// transform's tables (32 KiB) are read from global memory behind the key, abar_i is recomputed from the lvl0 word: neither is in LDS.
#pragma once
#include "cb_rotate.hpp"

namespace iyk {

// Keeps the instruction scheduler from moving loads across: the passes below read 64 words per lane, and with all of them hoisted ahead
// of the first butterfly a lane would hold more than the 256 registers two waves per SIMD leave it.
#if defined(__HIP_DEVICE_COMPILE__)
#define CBL_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define CBL_SCHED_FENCE() ((void)0)
#endif

static constexpr int CBL_LANES = 512;
static constexpr int CBL_SLOT = CB_N;                                       // u64 words of one slot: no padding
static constexpr size_t CBL_LDS_WORDS = 2 * CB_N + (size_t)CB_ROWS * CBL_SLOT;   // u64: acc, 8 slots
static constexpr size_t CBL_LDS_BYTES = CBL_LDS_WORDS * sizeof(u64);
static constexpr int CBL_PF = 8;                                            // prefetched operand pairs per lane: row 0, 2 q x 4 products
static_assert(CBL_LDS_BYTES <= 160 * 1024, "one workgroup per CU: the whole LDS and no more");

// ---- the transform's passes; bp = one slot -----------------------------------------------------------------------------------------
// pass 1 forward, lane j1 < 64: x[j2] already twisted by zeta^j2.  Leaves Y[j1][k2] at bp[k2 * 64 + (j1 ^ k2)].
IYK_HD void cbl_pass1_fwd(int j1, u64 (&x)[32], const u64* twf, u64* bp)
{
    ntt32_dif<LOG_W32>(x);
#pragma unroll
    for (int p = 0; p < 32; ++p) bp[brv5(p) * 64 + (j1 ^ brv5(p))] = gl_mul(x[p], twf[brv5(p) * 64 + j1]);
}
// pass 2 forward, lane u = k2 + 32 half < 64: on return position p holds X[k2 + 32 (2 brv5(p) + half)]
IYK_HD void cbl_pass2_fwd_read(int u, const u64* bp, u64 (&x)[32])
{
    const int k2 = u & 31, half = u >> 5;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const u64 a = bp[k2 * 64 + (j ^ k2)], b = bp[k2 * 64 + ((j + 32) ^ k2)];
        x[j] = half ? gl_mul_pow2(gl_sub(a, b), LOG_ZETA * j) : gl_add(a, b);
        if (j % 8 == 7) CBL_SCHED_FENCE();
    }
    ntt32_dif<LOG_W32>(x);
}
IYK_HD void cbl_pass2_fwd_write(int u, const u64 (&x)[32], u64* dst)   // natural order: dst[k], k = u + 64 brv5(p)
{
#pragma unroll
    for (int p = 0; p < 32; ++p) dst[u + 64 * brv5(p)] = x[p];
}
// pass 1' inverse, lane u = k2 + 32 half: bp[k] natural.  On return position p holds Z[k2][j1 = 2 brv5(p) + half], twiddled and scaled by 1 / N2.
IYK_HD void cbl_pass1_inv_read(int u, const u64* bp, const u64* twi, u64 (&x)[32])
{
    const int k2 = u & 31, half = u >> 5;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const u64 a = bp[k2 + 32 * j], b = bp[k2 + 32 * (j + 32)];
        x[j] = half ? gl_mul_pow2(gl_sub(a, b), ((192u - LOG_ZETA) * (unsigned)j) % 192u) : gl_add(a, b);
        if (j % 8 == 7) CBL_SCHED_FENCE();
    }
    ntt32_dif<192 - LOG_W32>(x);
#pragma unroll
    for (int p = 0; p < 32; ++p) x[p] = gl_mul(x[p], twi[(2 * brv5(p) + half) * 32 + k2]);
}
IYK_HD void cbl_pass1_inv_write(int u, const u64 (&x)[32], u64* bp)
{
    const int k2 = u & 31, half = u >> 5;
#pragma unroll
    for (int p = 0; p < 32; ++p) {
        const int j1 = 2 * brv5(p) + half;
        bp[j1 * 32 + (k2 ^ (j1 & 31))] = x[p];
    }
}
// pass 2' inverse, lane j1 < 64: on return position p holds coefficient j1 + 64 brv5(p), canonical
IYK_HD void cbl_pass2_inv(int j1, const u64* bp, u64 (&y)[32])
{
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) y[k2] = bp[j1 * 32 + (k2 ^ (j1 & 31))];
    ntt32_dif<192 - LOG_W32>(y);
#pragma unroll
    for (int p = 0; p < 32; ++p) y[p] = gl_mul_pow2(y[p], (192u - LOG_ZETA * (unsigned)brv5(p)) % 192u);
}

// ---- the phases of one rotation, per lane < 512 -------------------------------------------------------------------------------------
// abar of step i < n, and the rotation of the test vector (i == n): recomputed from the lvl0 word (cb_abar), there is no LDS array
IYK_HD u32 cbl_abar(const CbJob& jb, const u32* w, u32 n, u32 i) { return cb_abar(jb, w, n, i); }
// the initial accumulator
template <class Job, class... Shared>
IYK_HD void cbl_prologue(int lane, const Job& jb, const u32* w, u32 n, u64* acc, const Shared&... k)
{
    const u32 rot = cb_abar(jb, w, n, n, k...);
#pragma unroll
    for (int q = 0; q < CB_N / CBL_LANES; ++q) {
        const int j = lane + CBL_LANES * q;
        const u32 idx = ((u32)j - rot) & (2 * CB_N - 1);
        const u64 t = cb_tv(jb, idx & (CB_N - 1), k...);
        acc[j] = 0;
        acc[CB_N + j] = (idx & CB_N) ? 0ull - t : t;
    }
}

// forward pass 1 of digit polynomial v = lane >> 6 = 4 h + lvl into slot v: the rotated difference is re-derived from the accumulator
template <int L2, int BGBIT2>
IYK_HD void cbl_fwd1(int lane, u32 abar, const u64* acc, const u64* twf, u64* buf)
{
    typedef CbConsts<L2, BGBIT2> C;
    const int v = lane >> 6, lvl = v % L2, j1 = lane & 63;
    const u64* acc_h = acc + (v / L2) * CB_N;
    u64 x[32];
#pragma unroll
    for (int j2 = 0; j2 < 32; ++j2) {
        const u32 idx = ((u32)(j1 + 64 * j2) - abar) & (2 * CB_N - 1);
        u64 t = acc_h[idx & (CB_N - 1)];
        t = (idx & CB_N) ? 0ull - t : t;
        const u64 td = t - acc_h[j1 + 64 * j2];
        const u32 u = cb_digit_u<L2, BGBIT2>(td, lvl);
        x[j2] = gl_sub(gl_mul_small(u, C::tw.c[j2]), C::twk.c[j2]);
        if (j2 % 8 == 7) CBL_SCHED_FENCE();
    }
    cbl_pass1_fwd(j1, x, twf, buf + v * CBL_SLOT);
}
// forward pass 2 of the same polynomial by the same wave, in place
IYK_HD void cbl_fwd2_read(int lane, const u64* buf, u64 (&x)[32]) { cbl_pass2_fwd_read(lane & 63, buf + (lane >> 6) * CBL_SLOT, x); }
IYK_HD void cbl_fwd2_write(int lane, const u64 (&x)[32], u64* buf) { cbl_pass2_fwd_write(lane & 63, x, buf + (lane >> 6) * CBL_SLOT); }

// the operands of row 0 (h = 0, digit level 0) of a key step: pf[4 q + o] = BK2[half][0][c][k .. k + 1], o = 2 c + half, k = 2 lane + 1024 q
IYK_HD void cbl_prefetch(int lane, const u64* bk_step, CbPair (&pf)[CBL_PF])
{
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int o = 0; o < 4; ++o)
            pf[4 * q + o] = *reinterpret_cast<const CbPair*>(bk_step + ((size_t)(((o & 1) * CB_ROWS) * 2 + (o >> 1))) * CB_N + 2 * lane + 1024 * q);
}

// accum[o * 4 + 2 q + e] = sum over the 8 rows of D_row[k] * BK2[half][row][c][k], o = 2 c + half, k = 2 lane + 1024 q + e; row 0 from pf
IYK_HD void cbl_mac(int lane, const u64* buf, const u64* bk_step, const CbPair (&pf)[CBL_PF], u64 (&accum)[16])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) accum[t] = 0;
    CbPair cur[CBL_PF], nxt[CBL_PF];
#pragma unroll
    for (int t = 0; t < CBL_PF; ++t) cur[t] = nxt[t] = pf[t];
    // one row's operands in registers while the next row's are in flight; the loop stays rolled so that no more than two rows are held
#pragma unroll 1
    for (int row = 0; row < CB_ROWS; ++row) {
        if (row + 1 < CB_ROWS) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    nxt[4 * q + o] = *reinterpret_cast<const CbPair*>(bk_step + ((size_t)(((o & 1) * CB_ROWS + row + 1) * 2 + (o >> 1))) * CB_N + 2 * lane + 1024 * q);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const CbPair d = *reinterpret_cast<const CbPair*>(buf + row * CBL_SLOT + 2 * lane + 1024 * q);
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int e = 0; e < 2; ++e) accum[o * 4 + 2 * q + e] = gl_add(accum[o * 4 + 2 * q + e], gl_mul_weak(d.v[e], cur[4 * q + o].v[e]));
        }
#pragma unroll
        for (int t = 0; t < CBL_PF; ++t) cur[t] = nxt[t];
    }
}

// the sums of product o into slot o, natural order
IYK_HD void cbl_inv_write(int lane, const u64 (&accum)[16], u64* buf)
{
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            CbPair d;
            d.v[0] = accum[o * 4 + 2 * q], d.v[1] = accum[o * 4 + 2 * q + 1];
            *reinterpret_cast<CbPair*>(buf + o * CBL_SLOT + 2 * lane + 1024 * q) = d;
        }
}

// inverse of product o = lane >> 6 < 4 by wave o, in slot o
IYK_HD void cbl_inv1_read(int lane, const u64* buf, const u64* twi, u64 (&x)[32]) { cbl_pass1_inv_read(lane & 63, buf + (lane >> 6) * CBL_SLOT, twi, x); }
IYK_HD void cbl_inv1_write(int lane, const u64 (&x)[32], u64* buf) { cbl_pass1_inv_write(lane & 63, x, buf + (lane >> 6) * CBL_SLOT); }
// pass 2', lifted and added into the accumulator: the hi half enters shifted by 32.  Two waves add into every word, in either order.
IYK_HD void cbl_inv2(int lane, const u64* buf, u64* acc)
{
    const int o = lane >> 6, j1 = lane & 63;
    u64 y[32];
    cbl_pass2_inv(j1, buf + o * CBL_SLOT, y);
    u64* acc_c = acc + (o >> 1) * CB_N;
#pragma unroll
    for (int p = 0; p < 32; ++p) {
        const u64 s = cb_lift(y[p]);
        const u64 add = (o & 1) ? s << 32 : s;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(reinterpret_cast<unsigned long long*>(acc_c + j1 + 64 * brv5(p)), (unsigned long long)add);
#else
        acc_c[j1 + 64 * brv5(p)] += add;
#endif
    }
}

#if defined(__HIPCC__)
// Orders the LDS accesses of one wave: what its lanes stored before is what its lanes load after.  The LDS serves a wave's
// instructions in order, so no wait is needed; the fences keep the compiler from moving an access across.
__device__ __forceinline__ void cbl_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grid: min(njobs, CUs) workgroups; workgroup b runs jobs b, b + grid, ... (rounds).  tw: twf then twi (2 x 2048 u64), in global memory.
// <L2, BGBIT2>: the per-digit form, its arguments end at tlwe2; <L2, BGBIT2, CbManyJob, CbManyMu>: the many-digit form, k = one CbManyMu.
template <int L2, int BGBIT2, class Job = CbJob, class... Shared>
__global__ __launch_bounds__(CBL_LANES) void cb_rotate_lat_kernel(const Job* __restrict__ jobs, int njobs, const u32* __restrict__ tlwe0, u32 n,
                                                                  const u64* __restrict__ bk, const u64* __restrict__ tw, u64* __restrict__ tlwe2,
                                                                  const Shared... k)
{
    static_assert(L2 * 2 == CB_ROWS, "one wave per digit polynomial");
    extern __shared__ __align__(16) u64 cbl_lds[];
    u64* acc = cbl_lds;
    u64* buf = acc + 2 * CB_N;
    const u64* twf = tw;
    const u64* twi = tw + CB_N;
    const int lane = threadIdx.x;

    for (int job = blockIdx.x; job < njobs; job += gridDim.x) {
        const Job jb = jobs[job];
        const u32* w = tlwe0 + (size_t)jb.in * (n + 1);
        cbl_prologue(lane, jb, w, n, acc, k...);
        CbPair pf[CBL_PF];
        u32 ab = cb_abar(jb, w, n, 0, k...);
        __syncthreads();
        for (u32 i = 0; i < n; ++i) {
            // The lane number as a value of the step (i < n <= CB_MAX_N0 = 2047: the term is 0).  Everything a phase derives from its lane
            // alone (addresses, twists) would otherwise be computed once in front of the loop and held in registers through all phases
            // at once: 650 registers' worth, against the 256 a lane has at two waves per SIMD.
            const int ln = lane + (int)(i >> 11);
            const u64* bk_step = bk + (size_t)i * CB_STEP_WORDS;
            const u32 ab_next = cb_abar(jb, w, n, i + 1, k...);   // word i + 1 <= n is inside the row
            if (i == 0) cbl_prefetch(ln, bk_step, pf);       // later steps: requested by the step before
            u64 x[32];
            cbl_fwd1<L2, BGBIT2>(ln, ab, acc, twf, buf);
            cbl_wave_sync();
            cbl_fwd2_read(ln, buf, x);
            cbl_wave_sync();
            cbl_fwd2_write(ln, x, buf);
            __syncthreads();   // the 8 spectra are complete
            u64 accum[16];
            cbl_mac(ln, buf, bk_step, pf, accum);
            __syncthreads();   // ... and consumed
            cbl_inv_write(ln, accum, buf);
            if (i + 1 < n) cbl_prefetch(ln, bk_step + CB_STEP_WORDS, pf);   // in flight across the inverse transforms
            __syncthreads();   // the 4 products are in their slots
            if (ln < 4 * 64) {
                cbl_inv1_read(ln, buf, twi, x);
                cbl_wave_sync();
                cbl_inv1_write(ln, x, buf);
                cbl_wave_sync();
                cbl_inv2(ln, buf, acc);
            }
            __syncthreads();   // the accumulator is complete
            ab = ab_next;
        }
        cb_epilogue<CBL_LANES>(lane, jb, acc, tlwe2, k...);
        __syncthreads();   // the next round's prologue writes acc
    }
}
#endif

}  // namespace iyk
