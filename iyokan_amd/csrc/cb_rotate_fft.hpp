// cb_rotate_fft.hpp — the exact FP64 FFT form of the lvl0 -> lvl2 blind rotation of cb_rotate.hpp: the same job, the same host key
// windows, the same output words, bit for bit.  The arithmetic is DESIGN.md §2b restated for lvl2 (its lvl2 row holds the proof):
// every key word is split once, at upload, into four signed 16-bit quarters k = q0 + 2^16 q1 + 2^32 q2 + 2^48 q3; per step and output
// polynomial the four INTEGER sums R_j = sum_r d_r (*) q_{j,r} over the 8 digit polynomials are computed in FP64 (fft1024.hpp), rounded
// to the nearest integer — |R_j| <= 8 * 2048 * 2^8 * 2^15 = 2^37, within 2^-3.8 of it for ANY key and digits — and recombined as
// R_0 + (R_1 << 16) + (R_2 << 32) + (R_3 << 48) in 64-bit integer arithmetic.  The digits, (X^abar - 1) acc, the mod-switch, the
// sample extraction and + mu stay integer: cb_rotate.hpp's and cb_rotate_lat.hpp's own functions.
//
// The key is a second FORM of the lvl2 bootstrapping key object (iyk_hip_bk2_key_create_form, form 1), because the device layout
// differs: cplx [n][4 quarters][8 rows][2 cols][1024 positions] — 1 MiB per step — with the 1/1024 of the inverse folded in, in the
// position order of fft1024.hpp; then the transform's tables.  Nothing is chosen per batch.
//
// Schedule: cb_rotate_lat.hpp's plan.  One workgroup of 512 lanes (8 waves) per rotation, rounds inside the launch:
//   forward   wave v owns digit polynomial v = 4 h + lvl and LDS slot v (1024 complex points, 16 KiB); the three passes and the two
//             exchanges of the transform stay inside the wave (wave-level ordering points, no workgroup barrier)
//   multiply  every lane takes 2 positions of the 8 spectra into 16 complex running sums (2 output polynomials x 4 quarters x 2
//             positions): 512 FMAs
//   inverse   product o = 4 c + quarter is owned by wave o and slot o; the rounded sums enter the accumulator shifted by 16 quarter
//             through 64-bit LDS atomics (four waves add into every word; integer adds commute)
// Workgroup barriers per step: 4.  LDS: acc 32 KiB + 8 slots x 16 KiB = 160 KiB of 160.  The tables (33 KiB) are read from global
// memory behind the key.  No FP64 matrix instruction, no sync between workgroups, no spin wait.
#pragma once
#include "cb_rotate_lat.hpp"   // cbl_prologue, cbl_wave_sync; cb_rotate.hpp: cb_abar, cb_epilogue
#include "fft1024.hpp"

namespace iyk {

using fft::cplx;

static constexpr int CBF_LANES = 512;
static constexpr int CBF_QUARTERS = 4;
static constexpr int CBF_SLOT = fft1k::M;                                                // complex points of one slot
static constexpr size_t CBF_LDS_BYTES = 2 * CB_N * sizeof(u64) + (size_t)CB_ROWS * CBF_SLOT * sizeof(cplx);
static constexpr size_t CBF_STEP_POINTS = (size_t)CBF_QUARTERS * CB_ROWS * 2 * fft1k::M;   // complex points of one key step
static constexpr size_t CBF_STEP_BYTES = CBF_STEP_POINTS * sizeof(cplx);
static_assert(CBF_LDS_BYTES == 160 * 1024, "one workgroup per CU: the whole LDS and no more");
static_assert(CBF_STEP_BYTES == (1u << 20), "1 MiB of key spectra per step");
static_assert(CB_ROWS == 2 * CBF_QUARTERS, "the 8 product sums reuse the 8 spectra's slots");

// ---- the phases of one rotation, per lane < 512 -------------------------------------------------------------------------------------
// the folded digit polynomial v = lane >> 6 = 4 h + lvl, lane j1 = lane & 63: x[j2] = d[j] + i d[j + 1024], j = j1 + 64 j2, signed digits
template <int L2, int BGBIT2>
IYK_HD void cbf_digits(int lane, u32 abar, const u64* acc, cplx (&x)[16])
{
    typedef CbConsts<L2, BGBIT2> C;
    const int v = lane >> 6, lvl = v % L2, j1 = lane & 63;
    const u64* acc_h = acc + (v / L2) * CB_N;
#pragma unroll
    for (int j2 = 0; j2 < 16; ++j2) {
        double part[2];
#pragma unroll
        for (int top = 0; top < 2; ++top) {
            const int j = j1 + 64 * j2 + (CB_N / 2) * top;
            const u32 idx = ((u32)j - abar) & (2 * CB_N - 1);
            u64 t = acc_h[idx & (CB_N - 1)];
            t = (idx & CB_N) ? 0ull - t : t;
            const u64 td = t - acc_h[j];
            part[top] = (double)((int32_t)cb_digit_u<L2, BGBIT2>(td, lvl) - (int32_t)C::half_bg);
        }
        x[j2] = {part[0], part[1]};
    }
}
IYK_HD cplx* cbf_slot(cplx* buf, int lane) { return buf + (lane >> 6) * CBF_SLOT; }
IYK_HD const cplx* cbf_slot(const cplx* buf, int lane) { return buf + (lane >> 6) * CBF_SLOT; }

// accum[(4 c + q) * 2 + e] = sum over the 8 rows of D_row[p] * K[q][row][c][p], p = 2 lane + e
IYK_HD void cbf_mac(int lane, const cplx* buf, const cplx* bk_step, cplx (&accum)[16])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) accum[t] = {0.0, 0.0};
    // rolled: one row's 16 key points (64 registers) beside the 16 sums (64) is what a lane can hold at two waves per SIMD
#pragma unroll 1
    for (int row = 0; row < CB_ROWS; ++row) {
        const cplx d0 = buf[row * CBF_SLOT + 2 * lane], d1 = buf[row * CBF_SLOT + 2 * lane + 1];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < CBF_QUARTERS; ++q) {
                const cplx* kp = bk_step + ((size_t)((q * CB_ROWS + row) * 2 + c)) * fft1k::M + 2 * lane;
                const cplx k0 = kp[0], k1 = kp[1];
                cplx& s0 = accum[(4 * c + q) * 2];
                cplx& s1 = accum[(4 * c + q) * 2 + 1];
                s0 = {fft::fma_(d0.re, k0.re, fft::fma_(-d0.im, k0.im, s0.re)), fft::fma_(d0.re, k0.im, fft::fma_(d0.im, k0.re, s0.im))};
                s1 = {fft::fma_(d1.re, k1.re, fft::fma_(-d1.im, k1.im, s1.re)), fft::fma_(d1.re, k1.im, fft::fma_(d1.im, k1.re, s1.im))};
            }
    }
}
// the sums of product o into slot o, position order
IYK_HD void cbf_inv_write(int lane, const cplx (&accum)[16], cplx* buf)
{
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        buf[o * CBF_SLOT + 2 * lane] = accum[2 * o];
        buf[o * CBF_SLOT + 2 * lane + 1] = accum[2 * o + 1];
    }
}
// the last inverse pass of product o = lane >> 6 (output polynomial o >> 2, quarter o & 3), rounded and added into the accumulator
// shifted by 16 quarter.  Returns the largest |z - rint(z)| of the lane's 32 values where CHECK.
template <bool CHECK>
IYK_HD double cbf_inv_add(int lane, const cplx* tab, const cplx* buf, u64* acc)
{
    const int o = lane >> 6, j1 = lane & 63, shift = 16 * (o & 3);
    cplx x[16];
    fft1k::inv1(j1, tab, buf + o * CBF_SLOT, x);
    u64* acc_c = acc + (o >> 2) * CB_N;
    double err = 0.0;
#pragma unroll
    for (int j2 = 0; j2 < 16; ++j2) {
        const double part[2] = {x[j2].re, x[j2].im};
#pragma unroll
        for (int top = 0; top < 2; ++top) {
            if (CHECK) err = __builtin_fmax(err, fft::round_err(part[top]));
            const u64 add = (u64)fft1k::round_i64(part[top]) << shift;
            u64* dst = acc_c + j1 + 64 * j2 + (CB_N / 2) * top;
#if defined(__HIP_DEVICE_COMPILE__)
            atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)add);
#else
            *dst += add;
#endif
        }
    }
    return err;
}

// the key: quarter q of the folded polynomial, lane j1: x[j2] = q(w[j]) + i q(w[j + 1024])
IYK_HD void cbf_key_fold(int j1, int q, const u64* src, cplx (&x)[16])
{
#pragma unroll
    for (int j2 = 0; j2 < 16; ++j2) {
        const int j = j1 + 64 * j2;
        x[j2] = {(double)fft1k::key_quarter(src[j], q), (double)fft1k::key_quarter(src[j + CB_N / 2], q)};
    }
}
IYK_HD void cbf_key_write(int L, const cplx (&x)[16], cplx* dst)   // the 1 / 1024 of the inverse transform: a power of two, exact
{
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[L + 64 * r] = {x[r].re * (1.0 / fft1k::M), x[r].im * (1.0 / fft1k::M)};
}
// where the spectrum of (step, quarter, rc = row * 2 + col) starts, in complex points
IYK_HD size_t cbf_key_offset(size_t step, int q, int rc) { return step * CBF_STEP_POINTS + ((size_t)q * CB_ROWS * 2 + rc) * fft1k::M; }

#if defined(__HIPCC__)
// Key transform: torus-domain polynomials u64 [steps][8 rows][2 cols][N2] -> the four quarters' spectra.  One workgroup of one wave per
// (polynomial, quarter).
__global__ __launch_bounds__(64) void bk2_fft_kernel(const u64* __restrict__ torus, cplx* __restrict__ dst, const cplx* __restrict__ tab)
{
    __shared__ cplx sp[fft1k::M];
    const int lane = threadIdx.x;
    const u32 poly = blockIdx.x >> 2, q = blockIdx.x & 3;
    const u32 step = poly / (CB_ROWS * 2), rc = poly % (CB_ROWS * 2);
    cplx x[16];
    cbf_key_fold(lane, (int)q, torus + (size_t)poly * CB_N, x);
    fft1k::fwd1(lane, x, tab, sp);
    cbl_wave_sync();
    fft1k::fwd2_read(lane, tab, sp, x);
    cbl_wave_sync();
    fft1k::fwd2_write(lane, x, sp);
    cbl_wave_sync();
    fft1k::fwd3_read(lane, sp, x);
    cbf_key_write(lane, x, dst + cbf_key_offset(step, (int)q, (int)rc));
}

// grid: dispatch::cb_fft_grid workgroups; workgroup b runs jobs b, b + grid, ... (rounds, indexed by the job number).
// tab: fft1k::make_tables', in global memory.
// <L2, BGBIT2, CHECK>: the per-digit form, its arguments end at max_err_bits; <.., CbManyJob, CbManyMu>: the many-digit form, k = one CbManyMu.
template <int L2, int BGBIT2, bool CHECK, class Job = CbJob, class... Shared>
__global__ __launch_bounds__(CBF_LANES) void cb_rotate_fft_kernel(const Job* __restrict__ jobs, int njobs, const u32* __restrict__ tlwe0, u32 n,
                                                                  const cplx* __restrict__ bk, const cplx* __restrict__ tab, u64* __restrict__ tlwe2,
                                                                  unsigned long long* __restrict__ max_err_bits, const Shared... k)
{
    static_assert(L2 * 2 == CB_ROWS, "one wave per digit polynomial");
    extern __shared__ __align__(16) u64 cbf_lds[];
    u64* acc = cbf_lds;
    cplx* buf = reinterpret_cast<cplx*>(acc + 2 * CB_N);
    const int lane = threadIdx.x;
    double err = 0.0;

    for (int job = blockIdx.x; job < njobs; job += gridDim.x) {
        const Job jb = jobs[job];
        const u32* w = tlwe0 + (size_t)jb.in * (n + 1);
        cbl_prologue(lane, jb, w, n, acc, k...);
        __syncthreads();
        for (u32 i = 0; i < n; ++i) {
            // The lane number as a value of the step (i < n <= CB_MAX_N0 = 2047: the term is 0), as in cb_rotate_lat_kernel: what a phase
            // derives from its lane alone (addresses, and here the 48 table constants of the transforms) would otherwise be fetched once
            // in front of the loop and held in registers through all phases at once.
            const int ln = lane + (int)(i >> 11);
            const u32 ab = cb_abar(jb, w, n, i, k...);
            const cplx* bk_step = bk + (size_t)i * CBF_STEP_POINTS;
            cplx* sp = cbf_slot(buf, ln);
            const int L = ln & 63;
            cplx x[16];
            cbf_digits<L2, BGBIT2>(ln, ab, acc, x);
            fft1k::fwd1(L, x, tab, sp);
            cbl_wave_sync();
            fft1k::fwd2_read(L, tab, sp, x);
            cbl_wave_sync();
            fft1k::fwd2_write(L, x, sp);
            cbl_wave_sync();
            fft1k::fwd3_read(L, sp, x);
            cbl_wave_sync();
            fft1k::spec_write(L, x, sp);
            __syncthreads();   // the 8 spectra are complete
            cplx accum[16];
            cbf_mac(ln, buf, bk_step, accum);
            __syncthreads();   // ... and consumed
            cbf_inv_write(ln, accum, buf);
            __syncthreads();   // the 8 products are in their slots
            fft1k::inv3_read(L, sp, x);
            cbl_wave_sync();
            fft1k::inv3_write(L, x, sp);
            cbl_wave_sync();
            fft1k::inv2_read(L, tab, sp, x);
            cbl_wave_sync();
            fft1k::inv2_write(L, x, sp);
            cbl_wave_sync();
            const double e = cbf_inv_add<CHECK>(ln, tab, buf, acc);
            if (CHECK) err = __builtin_fmax(err, e);
            __syncthreads();   // the accumulator is complete
        }
        cb_epilogue<CBF_LANES>(lane, jb, acc, tlwe2, k...);
        __syncthreads();   // the next round's prologue writes acc
    }
    if (CHECK && max_err_bits) {   // non-negative doubles order like their bit patterns
        unsigned long long b;
        __builtin_memcpy(&b, &err, 8);
        atomicMax(max_err_bits, b);
    }
}
#endif

}  // namespace iyk
