// cmux_fft.hpp — one CMUX (TRGSW selector x TRLWE) per 64-lane wavefront on the complex-FFT path: the CMUX tree of Iyokan's ROM / RAM.
//
// A job {sel, in0, in1, rot, out} on a TRLWE store T (rows of 2N words: a(X), then b(X)) and a selector store S:
//     D   = (in1 >= 0) ? T[in1] - T[in0] : (X^rot - 1) T[in0]            (both polynomials, mod 2^32, rot in [0, 2N))
//     out = T[in0] + sum_r digits_r(D) (*) S[sel][r]                       (r over the (k+1) l rows, Gadget<L, BGBIT> digits)
// i.e. ONE step of the blind rotation (blind_rotate_fft.hpp) whose difference comes from two rows instead of a rotation of the
// accumulator, and whose key row is the caller's TRGSW instead of BK[i].  sel = 1 selects in1.  A selector slot has the layout of
// one step of the key spectra: cplx [(k+1) l][k+1][2][512], scaled by 1/512 (bk_fft_kernel makes both).  The product is the exact
// schoolbook one mod 2^32: the rounding bound of DESIGN.md section 2b holds for any key words and any digits.
//
// Per job: T[in0] -> the wave's LDS accumulator (so that out may be in0 or in1), u[16] per polynomial, 2 L rows of digits ->
// forward transform -> MAC into four spectra, two inverse transforms per output polynomial, rounded and added, accumulator -> T[out].
//
// Replaces TFHEpp::CMUXFFT<Lvl1>(res, cs, c1, c0) (res = c0 + cs [.] (c1 - c0)) and trgswfftExternalProduct after
// PolynomialMulByXaiMinusOne in TaskTFHEppROMUX / TaskTFHEppRAMUX / TaskTFHEppRAMCMUXs
// (/root/reference/src/iyokan_tfhepp.hpp:267,282-291,426-443,627); TFHEpp's product is an inexact FP64 FFT, this one is exact.
#pragma once
#include "blind_rotate_fft.hpp"
#include "jobs.hpp"   // CmuxJob, CmuxChainJob, CMUX_CHAIN_MAX_STEPS, CmuxRotChainJob, CmuxRotStep, CmuxTreeJob

namespace iyk {

namespace fft {

// cplx per selector slot: (k+1) l rows of (k+1) polynomials of two half spectra
template <class G>
constexpr u32 trgsw_slot_cplx() { return (u32)(2 * G::L) * 4u * (u32)M; }

// T[in0] -> accumulator: word L + 64 e, e < 32
IYK_HD void cmux_load_acc(int L, const u32* t_in0, u32* acc)
{
#pragma unroll
    for (int e = 0; e < 32; ++e) acc[L + 64 * e] = t_in0[L + 64 * e];
}
IYK_HD void cmux_store_acc(int L, const u32* acc, u32* t_out)
{
#pragma unroll
    for (int e = 0; e < 32; ++e) t_out[L + 64 * e] = acc[L + 64 * e];
}
// u[q] = prepare((T[in1]_c - T[in0]_c)[L + 64 q]), q < 16; in1_c = polynomial c of T[in1] in global memory, acc_c = of T[in0] in LDS
template <class G>
IYK_HD void cmux_diff16(int L, const u32* in1_c, const u32* acc_c, u32 (&u)[16])
{
    u32 w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = in1_c[L + 64 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) u[q] = G::prepare(w[q] - acc_c[L + 64 * q]);
}


// ---- chain of CMUXes on one accumulator (RAM write-back, cmux_chain_kernel below) ----
// Step j of a chain job, selector slot sel0 + j, against the row T[mem] in global memory:
//     pattern bit j = 0:  acc = acc    + S [.] (T[mem] - acc)      the CMUX job (in0 = acc, in1 = mem): cmux_diff16 + acc_update16
//     pattern bit j = 1:  acc = T[mem] + S [.] (acc - T[mem])      the CMUX job (in0 = mem, in1 = acc): the two functions below
// u[q] = prepare((acc_c - T[mem]_c)[L + 64 q]), q < 16: the difference the other way round
template <class G>
IYK_HD void cmux_diff16_rev(int L, const u32* mem_c, const u32* acc_c, u32 (&u)[16])
{
    u32 w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = mem_c[L + 64 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) u[q] = G::prepare(acc_c[L + 64 * q] - w[q]);
}
// acc_c[L + 64 q] = T[mem]_c[L + 64 q] + rounded product word: acc_update16 with the accumulator REPLACED by the row first.  A lane
// touches the words it owns in cmux_diff16 / acc_update16 only, and both polynomials' differences are taken before the first call.
IYK_HD void cmux_acc_replace16(int L, const u32* mem_c, const cplx (&hi)[8], const u32 (&lo)[16], u32* acc_c)
{
    u32 w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = mem_c[L + 64 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc_c[L + 64 * q] = w[q] + lo[q] + (round_u32(q < 8 ? hi[q].re : hi[q - 8].im) << 16);
}

}  // namespace fft

// A chain job (jobs.hpp: CmuxChainJob): acc = T[src]; steps CMUXes against T[mem] with selector slots sel0 .. sel0 + steps - 1, oriented
// by the bits of pattern; T[out] = acc

#if defined(__HIPCC__)
// One wavefront per job, BR_WAVES jobs per workgroup, the LDS map of blind_rotate_fft_kernel (kernels_fft.hpp, included first).  The
// waves of a workgroup are independent (own selector, form, rot); idle waves of the last workgroup recompute the last job and
// discard it.  The buffer descriptor is built per job on the selector's own base: its 32-bit offsets never limit the store's size.
template <class G, bool CHECK>
__global__ __launch_bounds__(64 * BR_WAVES, 2) void cmux_fft_kernel(const CmuxJob* __restrict__ jobs, int njobs,
                                                                    const fft::cplx* __restrict__ trgsw, u32* trlwe,
                                                                    const fft::Consts* __restrict__ Cp,
                                                                    unsigned long long* __restrict__ max_err_bits)
{
    const fft::Consts& C = *Cp;
    constexpr int L = G::L;
    extern __shared__ __attribute__((aligned(4096))) unsigned char smem[];
    fft::cplx* s_t1 = reinterpret_cast<fft::cplx*>(smem);                                   // [k0][lane]
    u32* s_acc = reinterpret_cast<u32*>(smem + BR_FFT_T1_BYTES);                            // [BR_WAVES][2][NTT_N]
    fft::cplx* s_xb = reinterpret_cast<fft::cplx*>(smem + BR_FFT_T1_BYTES + (size_t)BR_WAVES * 2 * NTT_N * sizeof(u32));
    fft::cplx* s_t2 = s_xb + (size_t)BR_WAVES * (fft::XCHG_BYTES / sizeof(fft::cplx));      // [b][a]
    fft::Lf* s_lf3 = reinterpret_cast<fft::Lf*>(s_t2 + 64);   // [which][lane'']
    fft::Lf* s_lf2 = s_lf3 + 4 * 64;                           // [which][k0]
    for (int e = threadIdx.x; e < 8 * 64; e += 64 * BR_WAVES) s_t1[e] = C.t1[e >> 6][e & 63];
    if (threadIdx.x < 64) s_t2[threadIdx.x] = C.t2t[threadIdx.x >> 3][threadIdx.x & 7];
    if (threadIdx.x < 4 * 64) s_lf3[threadIdx.x] = C.lf3[threadIdx.x >> 6][threadIdx.x & 63];
    if (threadIdx.x < 4 * 8) s_lf2[threadIdx.x] = C.lf2[threadIdx.x >> 3][threadIdx.x & 7];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    int job = blockIdx.x * BR_WAVES + wave;
    const bool live = job < njobs;
    if (!live) job = njobs - 1;
    // the job's five words are wave-uniform: said so to the compiler (scalar registers, a provably uniform descriptor)
    const int j_sel = __builtin_amdgcn_readfirstlane(jobs[job].sel), j_in0 = __builtin_amdgcn_readfirstlane(jobs[job].in0);
    const int j_in1 = __builtin_amdgcn_readfirstlane(jobs[job].in1), j_out = __builtin_amdgcn_readfirstlane(jobs[job].out);
    const u32 j_rot = (u32)__builtin_amdgcn_readfirstlane(jobs[job].rot);

    u32* acc_lds = s_acc + wave * 2 * NTT_N;
    fft::cplx* xb = s_xb + (size_t)wave * (fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cmux_load_acc(lane0, trlwe + (size_t)j_in0 * (2 * NTT_N), acc_lds);
    lds_sync();

    constexpr u32 SLOT = fft::trgsw_slot_cplx<G>();
    const fft::Keys keys(trgsw + (size_t)j_sel * SLOT, SLOT * (u32)sizeof(fft::cplx), lane0);
    fft::Twist U = C.u;
    asm volatile("" : "+s"(U.c1), "+s"(U.s1), "+s"(U.c2), "+s"(U.s2), "+s"(U.c3), "+s"(U.s3));
    fft::LfU LU = C.lu;
    asm volatile("" : "+s"(LU.t2), "+s"(LU.c2), "+s"(LU.t1), "+s"(LU.c1), "+s"(LU.t1w), "+s"(LU.c1w));

    fft::cplx S[2][2][8];   // [c'][half][k2]
    u32 u[16];
#pragma unroll
    for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][e & 7] = {0.0, 0.0};
#pragma unroll 1
    for (int r = 0; r < 2 * L; ++r) {
        const int lane = fft_lane_id(lane0);   // recomputed where it is needed, as in blind_rotate_fft_kernel: never worth a spill
        const int c = r >= L ? 1 : 0, lvl = r - c * L;
        if (lvl == 0) {
            if (j_in1 >= 0) fft::cmux_diff16<G>(lane, trlwe + (size_t)j_in1 * (2 * NTT_N) + c * NTT_N, acc_lds + c * NTT_N, u);
            else fft::diff16<G>(lane, j_rot, acc_lds + c * NTT_N, u);
        }
        fft::cplx a[8];
        fft::digits8<G>(lvl, u, a);
        // the row's first key words go out before the transform and land under it; the rest a frequency block ahead of its products
        const u32 row_off = (u32)r * 4u * (u32)fft::M;
        const u32 koff = (u32)lane * 16u;
        fft::cplx k0[4], k1[4];
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) k0[pc] = keys.at_lane(koff, row_off, pc, 0);
        __builtin_amdgcn_sched_barrier(0);
        fft_forward_lf(lane, a, LU, s_lf2, s_lf3, xb);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            fft::cplx (&cur)[4] = (q & 1) ? k1 : k0;
            fft::cplx (&nxt)[4] = (q & 1) ? k0 : k1;
            __builtin_amdgcn_sched_barrier(0);   // the loads stay where they are written: hoisted, a row's 32 values do not fit
            if (q + 1 < 8) {
#pragma unroll
                for (int pc = 0; pc < 4; ++pc) nxt[pc] = keys.at_lane(koff, row_off, pc, q + 1);
            }
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][q], a[q], cur[pc]);
        }
    }
    double worst = 0.0;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const int lane = fft_lane_id(lane0);
        u32 lo[16];
        fft_inverse2(lane, S[cc][0], S[cc][1], U, s_t1 + lane, s_t2 + (lane & 7), xb);
        if (CHECK) {
            const double e0 = fft::round_err8(S[cc][0]), e1 = fft::round_err8(S[cc][1]);
            worst = e0 > worst ? e0 : worst;
            worst = e1 > worst ? e1 : worst;
        }
        fft::round16(S[cc][0], lo);
        fft::acc_update16(lane, S[cc][1], lo, acc_lds + cc * NTT_N);
    }
    set_prio<0>();
    lds_sync();
    if (CHECK && max_err_bits) {   // non-negative doubles order like their bit patterns
        unsigned long long b;
        __builtin_memcpy(&b, &worst, 8);
        atomicMax(max_err_bits, b);
    }
    if (live) fft::cmux_store_acc(lane0, acc_lds, trlwe + (size_t)j_out * (2 * NTT_N));
}

// A chain of CMUXes per wavefront (CmuxChainJob): the RAM write-back of one cell, TaskTFHEppRAMCMUXs
// (/root/reference/src/iyokan_tfhepp.hpp:622-628: *output_ = written; CMUXFFT(*output_, normal or inverted selector j, *output_, *mem_)
// for every address bit j).  The same workgroup shape, LDS map and row loop as cmux_fft_kernel; the accumulator stays in the wave's
// LDS for all steps, T[mem] is re-read from global memory in every step (L2 serves it), and the selector's descriptor is rebuilt per
// step on that slot's own base.  The words are those of `steps` cmux_fft_kernel jobs one after the other: the product is exact.
// Where pattern bit j is 1 the step is the job (in0 = mem, in1 = acc): both polynomials' differences acc - T[mem] are taken in the
// row loop, before the update replaces the accumulator by T[mem] and adds the rounded product.
template <class G, bool CHECK>
__global__ __launch_bounds__(64 * BR_WAVES, 2) void cmux_chain_kernel(const CmuxChainJob* __restrict__ jobs, int njobs,
                                                                      const fft::cplx* __restrict__ trgsw, u32* trlwe,
                                                                      const fft::Consts* __restrict__ Cp,
                                                                      unsigned long long* __restrict__ max_err_bits)
{
    const fft::Consts& C = *Cp;
    constexpr int L = G::L;
    extern __shared__ __attribute__((aligned(4096))) unsigned char smem[];
    fft::cplx* s_t1 = reinterpret_cast<fft::cplx*>(smem);                                   // [k0][lane]
    u32* s_acc = reinterpret_cast<u32*>(smem + BR_FFT_T1_BYTES);                            // [BR_WAVES][2][NTT_N]
    fft::cplx* s_xb = reinterpret_cast<fft::cplx*>(smem + BR_FFT_T1_BYTES + (size_t)BR_WAVES * 2 * NTT_N * sizeof(u32));
    fft::cplx* s_t2 = s_xb + (size_t)BR_WAVES * (fft::XCHG_BYTES / sizeof(fft::cplx));      // [b][a]
    fft::Lf* s_lf3 = reinterpret_cast<fft::Lf*>(s_t2 + 64);   // [which][lane'']
    fft::Lf* s_lf2 = s_lf3 + 4 * 64;                           // [which][k0]
    for (int e = threadIdx.x; e < 8 * 64; e += 64 * BR_WAVES) s_t1[e] = C.t1[e >> 6][e & 63];
    if (threadIdx.x < 64) s_t2[threadIdx.x] = C.t2t[threadIdx.x >> 3][threadIdx.x & 7];
    if (threadIdx.x < 4 * 64) s_lf3[threadIdx.x] = C.lf3[threadIdx.x >> 6][threadIdx.x & 63];
    if (threadIdx.x < 4 * 8) s_lf2[threadIdx.x] = C.lf2[threadIdx.x >> 3][threadIdx.x & 7];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    int job = blockIdx.x * BR_WAVES + wave;
    const bool live = job < njobs;
    if (!live) job = njobs - 1;
    // the job's six words are wave-uniform (scalar registers, a provably uniform descriptor and a scalar branch per step)
    const int j_sel0 = __builtin_amdgcn_readfirstlane(jobs[job].sel0), j_steps = __builtin_amdgcn_readfirstlane(jobs[job].steps);
    const u32 j_pattern = (u32)__builtin_amdgcn_readfirstlane((int)jobs[job].pattern);
    const int j_src = __builtin_amdgcn_readfirstlane(jobs[job].src), j_mem = __builtin_amdgcn_readfirstlane(jobs[job].mem);
    const int j_out = __builtin_amdgcn_readfirstlane(jobs[job].out);

    u32* acc_lds = s_acc + wave * 2 * NTT_N;
    fft::cplx* xb = s_xb + (size_t)wave * (fft::XCHG_BYTES / sizeof(fft::cplx));
    const u32* mem_row = trlwe + (size_t)j_mem * (2 * NTT_N);
    fft::cmux_load_acc(lane0, trlwe + (size_t)j_src * (2 * NTT_N), acc_lds);
    lds_sync();

    constexpr u32 SLOT = fft::trgsw_slot_cplx<G>();
    fft::Twist U = C.u;
    asm volatile("" : "+s"(U.c1), "+s"(U.s1), "+s"(U.c2), "+s"(U.s2), "+s"(U.c3), "+s"(U.s3));
    fft::LfU LU = C.lu;
    asm volatile("" : "+s"(LU.t2), "+s"(LU.c2), "+s"(LU.t1), "+s"(LU.c1), "+s"(LU.t1w), "+s"(LU.c1w));

    double worst = 0.0;
#pragma unroll 1
    for (int j = 0; j < j_steps; ++j) {
        const bool rev = (j_pattern >> j) & 1u;   // in0 = mem, in1 = acc
        const fft::Keys keys(trgsw + (size_t)(j_sel0 + j) * SLOT, SLOT * (u32)sizeof(fft::cplx), lane0);
        fft::cplx S[2][2][8];   // [c'][half][k2]
        u32 u[16];
#pragma unroll
        for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][e & 7] = {0.0, 0.0};
#pragma unroll 1
        for (int r = 0; r < 2 * L; ++r) {
            const int lane = fft_lane_id(lane0);
            const int c = r >= L ? 1 : 0, lvl = r - c * L;
            if (lvl == 0) {
                if (rev) fft::cmux_diff16_rev<G>(lane, mem_row + c * NTT_N, acc_lds + c * NTT_N, u);
                else fft::cmux_diff16<G>(lane, mem_row + c * NTT_N, acc_lds + c * NTT_N, u);
            }
            fft::cplx a[8];
            fft::digits8<G>(lvl, u, a);
            const u32 row_off = (u32)r * 4u * (u32)fft::M;
            const u32 koff = (u32)lane * 16u;
            fft::cplx k0[4], k1[4];
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) k0[pc] = keys.at_lane(koff, row_off, pc, 0);
            __builtin_amdgcn_sched_barrier(0);
            fft_forward_lf(lane, a, LU, s_lf2, s_lf3, xb);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                fft::cplx (&cur)[4] = (q & 1) ? k1 : k0;
                fft::cplx (&nxt)[4] = (q & 1) ? k0 : k1;
                __builtin_amdgcn_sched_barrier(0);   // as in cmux_fft_kernel: hoisted, a row's 32 values do not fit
                if (q + 1 < 8) {
#pragma unroll
                    for (int pc = 0; pc < 4; ++pc) nxt[pc] = keys.at_lane(koff, row_off, pc, q + 1);
                }
#pragma unroll
                for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][q], a[q], cur[pc]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int lane = fft_lane_id(lane0);
            u32 lo[16];
            fft_inverse2(lane, S[cc][0], S[cc][1], U, s_t1 + lane, s_t2 + (lane & 7), xb);
            if (CHECK) {
                const double e0 = fft::round_err8(S[cc][0]), e1 = fft::round_err8(S[cc][1]);
                worst = e0 > worst ? e0 : worst;
                worst = e1 > worst ? e1 : worst;
            }
            fft::round16(S[cc][0], lo);
            if (rev) fft::cmux_acc_replace16(lane, mem_row + cc * NTT_N, S[cc][1], lo, acc_lds + cc * NTT_N);
            else fft::acc_update16(lane, S[cc][1], lo, acc_lds + cc * NTT_N);
        }
        set_prio<0>();
        lds_sync();
    }
    if (CHECK && max_err_bits) {   // non-negative doubles order like their bit patterns
        unsigned long long b;
        __builtin_memcpy(&b, &worst, 8);
        atomicMax(max_err_bits, b);
    }
    if (live) fft::cmux_store_acc(lane0, acc_lds, trlwe + (size_t)j_out * (2 * NTT_N));
}

// A chain of ROTATE-form CMUXes per wavefront (CmuxRotChainJob): the lower half of a ROM read, LROMUX of TaskTFHEppROMUX
// (/root/reference/src/iyokan_tfhepp.hpp:282-291: per low address bit PolynomialMulByXaiMinusOne of the accumulator, trgswfftExternalProduct
// with that bit's selector, added to the accumulator).  Step j of job g takes the pair (sel, rot) = list[first + j] of the staged step
// list:   acc = acc + S[sel] [.] ((X^rot - 1) acc),   each the in1 < 0 job of cmux_fft_kernel with in0 = out = acc.
// The same workgroup shape, LDS map and row loop as cmux_chain_kernel; the accumulator stays in the wave's LDS for all steps and a step
// reads NOTHING from the TRLWE store: the rotated difference comes from the accumulator itself (diff16, as in blind_rotate_fft_kernel,
// whose step this is with the caller's selector in place of BK[i]).  diff16 reads other lanes' accumulator words, acc_update16 writes
// the lane's own: both polynomials' differences are taken in the row loop, before the first update, and the lds_sync that ends a step
// orders its updates before the next step's reads.  The words are those of `steps` cmux_fft_kernel rotate jobs one after the other.
template <class G, bool CHECK>
__global__ __launch_bounds__(64 * BR_WAVES, 2) void cmux_rotate_chain_kernel(const CmuxRotChainJob* __restrict__ jobs, int njobs,
                                                                             const CmuxRotStep* __restrict__ list,
                                                                             const fft::cplx* __restrict__ trgsw, u32* trlwe,
                                                                             const fft::Consts* __restrict__ Cp,
                                                                             unsigned long long* __restrict__ max_err_bits)
{
    const fft::Consts& C = *Cp;
    constexpr int L = G::L;
    extern __shared__ __attribute__((aligned(4096))) unsigned char smem[];
    fft::cplx* s_t1 = reinterpret_cast<fft::cplx*>(smem);                                   // [k0][lane]
    u32* s_acc = reinterpret_cast<u32*>(smem + BR_FFT_T1_BYTES);                            // [BR_WAVES][2][NTT_N]
    fft::cplx* s_xb = reinterpret_cast<fft::cplx*>(smem + BR_FFT_T1_BYTES + (size_t)BR_WAVES * 2 * NTT_N * sizeof(u32));
    fft::cplx* s_t2 = s_xb + (size_t)BR_WAVES * (fft::XCHG_BYTES / sizeof(fft::cplx));      // [b][a]
    fft::Lf* s_lf3 = reinterpret_cast<fft::Lf*>(s_t2 + 64);   // [which][lane'']
    fft::Lf* s_lf2 = s_lf3 + 4 * 64;                           // [which][k0]
    for (int e = threadIdx.x; e < 8 * 64; e += 64 * BR_WAVES) s_t1[e] = C.t1[e >> 6][e & 63];
    if (threadIdx.x < 64) s_t2[threadIdx.x] = C.t2t[threadIdx.x >> 3][threadIdx.x & 7];
    if (threadIdx.x < 4 * 64) s_lf3[threadIdx.x] = C.lf3[threadIdx.x >> 6][threadIdx.x & 63];
    if (threadIdx.x < 4 * 8) s_lf2[threadIdx.x] = C.lf2[threadIdx.x >> 3][threadIdx.x & 7];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    int job = blockIdx.x * BR_WAVES + wave;
    const bool live = job < njobs;
    if (!live) job = njobs - 1;
    // the job's four words and every step's pair are wave-uniform (scalar registers, a provably uniform descriptor)
    const int j_first = __builtin_amdgcn_readfirstlane(jobs[job].first), j_steps = __builtin_amdgcn_readfirstlane(jobs[job].steps);
    const int j_src = __builtin_amdgcn_readfirstlane(jobs[job].src), j_out = __builtin_amdgcn_readfirstlane(jobs[job].out);

    u32* acc_lds = s_acc + wave * 2 * NTT_N;
    fft::cplx* xb = s_xb + (size_t)wave * (fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cmux_load_acc(lane0, trlwe + (size_t)j_src * (2 * NTT_N), acc_lds);
    lds_sync();

    constexpr u32 SLOT = fft::trgsw_slot_cplx<G>();
    fft::Twist U = C.u;
    asm volatile("" : "+s"(U.c1), "+s"(U.s1), "+s"(U.c2), "+s"(U.s2), "+s"(U.c3), "+s"(U.s3));
    fft::LfU LU = C.lu;
    asm volatile("" : "+s"(LU.t2), "+s"(LU.c2), "+s"(LU.t1), "+s"(LU.c1), "+s"(LU.t1w), "+s"(LU.c1w));

    double worst = 0.0;
#pragma unroll 1
    for (int j = 0; j < j_steps; ++j) {
        const int s_sel = __builtin_amdgcn_readfirstlane(list[j_first + j].sel);
        const u32 s_rot = (u32)__builtin_amdgcn_readfirstlane(list[j_first + j].rot);
        const fft::Keys keys(trgsw + (size_t)s_sel * SLOT, SLOT * (u32)sizeof(fft::cplx), lane0);
        fft::cplx S[2][2][8];   // [c'][half][k2]
        u32 u[16];
#pragma unroll
        for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][e & 7] = {0.0, 0.0};
#pragma unroll 1
        for (int r = 0; r < 2 * L; ++r) {
            const int lane = fft_lane_id(lane0);
            const int c = r >= L ? 1 : 0, lvl = r - c * L;
            if (lvl == 0) fft::diff16<G>(lane, s_rot, acc_lds + c * NTT_N, u);
            fft::cplx a[8];
            fft::digits8<G>(lvl, u, a);
            const u32 row_off = (u32)r * 4u * (u32)fft::M;
            const u32 koff = (u32)lane * 16u;
            fft::cplx k0[4], k1[4];
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) k0[pc] = keys.at_lane(koff, row_off, pc, 0);
            __builtin_amdgcn_sched_barrier(0);
            fft_forward_lf(lane, a, LU, s_lf2, s_lf3, xb);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                fft::cplx (&cur)[4] = (q & 1) ? k1 : k0;
                fft::cplx (&nxt)[4] = (q & 1) ? k0 : k1;
                __builtin_amdgcn_sched_barrier(0);   // as in cmux_fft_kernel: hoisted, a row's 32 values do not fit
                if (q + 1 < 8) {
#pragma unroll
                    for (int pc = 0; pc < 4; ++pc) nxt[pc] = keys.at_lane(koff, row_off, pc, q + 1);
                }
#pragma unroll
                for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][q], a[q], cur[pc]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int lane = fft_lane_id(lane0);
            u32 lo[16];
            fft_inverse2(lane, S[cc][0], S[cc][1], U, s_t1 + lane, s_t2 + (lane & 7), xb);
            if (CHECK) {
                const double e0 = fft::round_err8(S[cc][0]), e1 = fft::round_err8(S[cc][1]);
                worst = e0 > worst ? e0 : worst;
                worst = e1 > worst ? e1 : worst;
            }
            fft::round16(S[cc][0], lo);
            fft::acc_update16(lane, S[cc][1], lo, acc_lds + cc * NTT_N);
        }
        set_prio<0>();
        lds_sync();
    }
    if (CHECK && max_err_bits) {   // non-negative doubles order like their bit patterns
        unsigned long long b;
        __builtin_memcpy(&b, &worst, 8);
        atomicMax(max_err_bits, b);
    }
    if (live) fft::cmux_store_acc(lane0, acc_lds, trlwe + (size_t)j_out * (2 * NTT_N));
}

// A CMUX read tree per WORKGROUP (CmuxTreeJob): up to CMUX_TREE_MAX_LEVELS = log2(2 BR_WAVES) levels of the upper half of a ROM / RAM
// read, UROMUX of TaskTFHEppROMUX and TaskTFHEppRAMUX (/root/reference/src/iyokan_tfhepp.hpp:267,426-443: CMUXFFT over pairs of
// candidate rows, one address bit per level).  Unlike the three kernels above a workgroup, not a wave, owns a job.
//   level 0:       wave w < 2^(levels-1) is cmux_fft_kernel's job (sel0, in0 = T[first + 2 w], in1 = T[first + 2 w + 1]); the result
//                  stays in the wave's accumulator s_acc[w].
//   level b >= 1:  the waves with w % 2^b == 0 go on: in0 = the wave's own accumulator, in1 = the accumulator of wave w + 2^(b-1), read
//                  from LDS (cmux_diff16 on an LDS source), selector slot sel0 + b; the result stays in s_acc[w].
// Wave w + 2^(b-1) took part in level b - 1 and takes part in no later one: at level b nobody writes what another wave reads, and a
// wave reads its partner's words only after the workgroup barrier that follows level b - 1.  The barriers stand between the levels,
// outside every branch on the wave number, so all 8 waves reach each of them — the waves a short tree never uses and the ones that have
// dropped out included.  No word leaves the workgroup between the levels; wave 0 stores T[out] after the last one.  The same workgroup
// shape, LDS map, row loop and per-step descriptor on the slot's own base as cmux_fft_kernel, and the words of `levels` successive
// cmux_fft_kernel launches: the product is exact.
template <class G, bool CHECK>
__global__ __launch_bounds__(64 * BR_WAVES, 2) void cmux_tree_kernel(const CmuxTreeJob* __restrict__ jobs,
                                                                     const fft::cplx* __restrict__ trgsw, u32* trlwe,
                                                                     const fft::Consts* __restrict__ Cp,
                                                                     unsigned long long* __restrict__ max_err_bits)
{
    const fft::Consts& C = *Cp;
    constexpr int L = G::L;
    extern __shared__ __attribute__((aligned(4096))) unsigned char smem[];
    fft::cplx* s_t1 = reinterpret_cast<fft::cplx*>(smem);                                   // [k0][lane]
    u32* s_acc = reinterpret_cast<u32*>(smem + BR_FFT_T1_BYTES);                            // [BR_WAVES][2][NTT_N]
    fft::cplx* s_xb = reinterpret_cast<fft::cplx*>(smem + BR_FFT_T1_BYTES + (size_t)BR_WAVES * 2 * NTT_N * sizeof(u32));
    fft::cplx* s_t2 = s_xb + (size_t)BR_WAVES * (fft::XCHG_BYTES / sizeof(fft::cplx));      // [b][a]
    fft::Lf* s_lf3 = reinterpret_cast<fft::Lf*>(s_t2 + 64);   // [which][lane'']
    fft::Lf* s_lf2 = s_lf3 + 4 * 64;                           // [which][k0]
    for (int e = threadIdx.x; e < 8 * 64; e += 64 * BR_WAVES) s_t1[e] = C.t1[e >> 6][e & 63];
    if (threadIdx.x < 64) s_t2[threadIdx.x] = C.t2t[threadIdx.x >> 3][threadIdx.x & 7];
    if (threadIdx.x < 4 * 64) s_lf3[threadIdx.x] = C.lf3[threadIdx.x >> 6][threadIdx.x & 63];
    if (threadIdx.x < 4 * 8) s_lf2[threadIdx.x] = C.lf2[threadIdx.x >> 3][threadIdx.x & 7];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    static_assert((1 << CMUX_TREE_MAX_LEVELS) == 2 * BR_WAVES, "level 0 of the deepest tree is one CMUX per wave");
    const int job = blockIdx.x;   // the grid is the job count (dispatch.hpp: cmux_tree_grid)
    // the job's four words are uniform over the workgroup (scalar registers, a provably uniform descriptor, scalar branches per level)
    const int j_sel0 = __builtin_amdgcn_readfirstlane(jobs[job].sel0), j_levels = __builtin_amdgcn_readfirstlane(jobs[job].levels);
    const int j_first = __builtin_amdgcn_readfirstlane(jobs[job].first), j_out = __builtin_amdgcn_readfirstlane(jobs[job].out);
    const bool member = wave < (1 << (j_levels - 1));   // the wave has a CMUX of level 0: a tree of fewer than 4 levels leaves the high waves idle

    u32* acc_lds = s_acc + wave * 2 * NTT_N;
    fft::cplx* xb = s_xb + (size_t)wave * (fft::XCHG_BYTES / sizeof(fft::cplx));
    const u32* leaf1 = trlwe + (size_t)(j_first + 2 * wave + 1) * (2 * NTT_N);   // in1 of level 0; read by members only
    if (member) fft::cmux_load_acc(lane0, trlwe + (size_t)(j_first + 2 * wave) * (2 * NTT_N), acc_lds);
    lds_sync();

    constexpr u32 SLOT = fft::trgsw_slot_cplx<G>();
    fft::Twist U = C.u;
    asm volatile("" : "+s"(U.c1), "+s"(U.s1), "+s"(U.c2), "+s"(U.s2), "+s"(U.c3), "+s"(U.s3));
    fft::LfU LU = C.lu;
    asm volatile("" : "+s"(LU.t2), "+s"(LU.c2), "+s"(LU.t1), "+s"(LU.c1), "+s"(LU.t1w), "+s"(LU.c1w));

    double worst = 0.0;
#pragma unroll 1
    for (int b = 0; b < j_levels; ++b) {
        if (member && (wave & ((1 << b) - 1)) == 0) {   // wave-uniform: no barrier inside
            const u32* partner = s_acc + (wave + ((1 << b) >> 1)) * 2 * NTT_N;   // in1 of level b >= 1: a wave that has dropped out
            const fft::Keys keys(trgsw + (size_t)(j_sel0 + b) * SLOT, SLOT * (u32)sizeof(fft::cplx), lane0);
            fft::cplx S[2][2][8];   // [c'][half][k2]
            u32 u[16];
#pragma unroll
            for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][e & 7] = {0.0, 0.0};
#pragma unroll 1
            for (int r = 0; r < 2 * L; ++r) {
                const int lane = fft_lane_id(lane0);
                const int c = r >= L ? 1 : 0, lvl = r - c * L;
                if (lvl == 0) {
                    if (b == 0) fft::cmux_diff16<G>(lane, leaf1 + c * NTT_N, acc_lds + c * NTT_N, u);
                    else fft::cmux_diff16<G>(lane, partner + c * NTT_N, acc_lds + c * NTT_N, u);
                }
                fft::cplx a[8];
                fft::digits8<G>(lvl, u, a);
                const u32 row_off = (u32)r * 4u * (u32)fft::M;
                const u32 koff = (u32)lane * 16u;
                fft::cplx k0[4], k1[4];
#pragma unroll
                for (int pc = 0; pc < 4; ++pc) k0[pc] = keys.at_lane(koff, row_off, pc, 0);
                __builtin_amdgcn_sched_barrier(0);
                fft_forward_lf(lane, a, LU, s_lf2, s_lf3, xb);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    fft::cplx (&cur)[4] = (q & 1) ? k1 : k0;
                    fft::cplx (&nxt)[4] = (q & 1) ? k0 : k1;
                    __builtin_amdgcn_sched_barrier(0);   // as in cmux_fft_kernel: hoisted, a row's 32 values do not fit
                    if (q + 1 < 8) {
#pragma unroll
                        for (int pc = 0; pc < 4; ++pc) nxt[pc] = keys.at_lane(koff, row_off, pc, q + 1);
                    }
#pragma unroll
                    for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][q], a[q], cur[pc]);
                }
            }
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int lane = fft_lane_id(lane0);
                u32 lo[16];
                fft_inverse2(lane, S[cc][0], S[cc][1], U, s_t1 + lane, s_t2 + (lane & 7), xb);
                if (CHECK) {
                    const double e0 = fft::round_err8(S[cc][0]), e1 = fft::round_err8(S[cc][1]);
                    worst = e0 > worst ? e0 : worst;
                    worst = e1 > worst ? e1 : worst;
                }
                fft::round16(S[cc][0], lo);
                fft::acc_update16(lane, S[cc][1], lo, acc_lds + cc * NTT_N);
            }
            set_prio<0>();
        }
        // between two levels: the level's accumulators are written before a wave of the next level reads its partner's.  Every wave of
        // the workgroup comes here, b and j_levels are the same for all of them.
        if (b + 1 < j_levels) __syncthreads();
    }
    lds_sync();
    if (CHECK && max_err_bits) {   // non-negative doubles order like their bit patterns
        unsigned long long bits;
        __builtin_memcpy(&bits, &worst, 8);
        atomicMax(max_err_bits, bits);
    }
    if (wave == 0) fft::cmux_store_acc(lane0, acc_lds, trlwe + (size_t)j_out * (2 * NTT_N));
}
#endif

}  // namespace iyk
