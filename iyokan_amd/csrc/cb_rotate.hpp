// cb_rotate.hpp — lvl0 -> lvl2 blind rotation (N2 = 2048, k = 1, 64-bit torus): the first half of circuit bootstrapping, whose
// outputs are the lvl2 TLWEs the private key switch (privks.hpp) turns into TRGSW selector rows.
//
// A job {in, sign, off, mu, out} on a lvl0 TLWE store W0 (u32 [slots][n + 1]), the key BK2 and a lvl2 TLWE store W2 (u64 [slots][N2 + 1]):
//     lin      = sign * W0[in] + (0, .., 0, off)                                  (mod 2^32)
//     abar_i   = (lin_i + 2^19) >> 20,  rot = (2 N2 - (lin_n >> 20)) mod 2 N2     (modswitch_kernel's rounding at 2 N2 = 4096)
//     acc      = X^rot * (0, mu (1 + X + .. + X^(N2-1)));   acc += BK2_i [.] ((X^abar_i - 1) acc)  for i < n
//     W2[out]  = SampleExtractIndex(acc, 0) + (0, .., 0, mu)
// [.]: digit j <= l2 of a word x is ((x + offset + round) >> (64 - j Bgbit2) & (Bg - 1)) - Bg/2 with offset = sum_j (Bg/2) 2^(64 - j Bgbit2)
// and round = 2^(64 - l2 Bgbit2 - 1); row r = h l2 + (j-1) of the TRGSW multiplies digit j of polynomial h; orientation as the lvl1 kernels.
//
// Exactness.  Every output word is the schoolbook negacyclic product mod 2^64.  Each key word is split into two 32-bit halves and each
// half is multiplied in Z_P, P = 2^64 - 2^32 + 1: |digit| <= 2^8, half < 2^32, (k+1) l2 N2 = 2^14 terms per sum, so every integer sum
// is below 2^54 < P/2 in magnitude and its centred residue IS the integer; the product mod 2^64 is S_lo + (S_hi << 32).  No rounding
// margin is involved anywhere.
//
// Transform.  X[k] = sum_j x[j] psi^(j (2k+1)), psi a primitive 4096th root with psi^64 = 2^3.  j = j1 + 64 j2, k = k2 + 32 k1:
//     psi^(j(2k+1)) = zeta^(j2 (2 k2 + 1)) * psi^(j1 (2 k2 + 1)) * w64^(j1 k1),   zeta = w64 = psi^64 = 2^3
//   pass 1 (lane = j1 < 64): negacyclic 32-point over j2 -> k2 (twist 2^(3 j2), ntt32_dif<6>), times twf[k2][j1] = psi^(j1 (2 k2 + 1))
//   pass 2 (lane = k2 < 32): cyclic 64-point over j1 -> k1 (ntt64_dif<3>): shifts only
// and the mirror image back (64-point over k1 -> j1 with 2^-3, times twi[j1][k2] = psi^(-j1 (2 k2 + 1)) / N2, 32-point over k2 -> j2).
//
// Kernel: one workgroup of 256 lanes per rotation, the accumulator (32 KiB) in LDS for all n steps.  Per step and accumulator
// polynomial h: the l2 = 4 digit polynomials go through pass 1 on 4 x 64 lanes and pass 2 on 4 x 32 lanes, their spectra land in LDS
// in natural order, and every lane multiplies its 8 points (k = 2 lane + 512 q + e) of the 4 rows into 4 x 8 running sums (2 output
// polynomials x 2 key halves) held in registers — the eight spectra (128 KiB) never exist at once.  Then 4 inverse transforms, and
// each lane adds its lifted words into the LDS accumulator (integer adds mod 2^64: the lo and the hi << 32 part commute).
// LDS: acc 32 KiB + 4 polynomials x 2112 u64 (66 KiB) + tables 32 KiB + abar 8 KiB = 138 KiB of 160.
// Workgroups of one launch walk the key in step: a key row is fetched from HBM once and found in L2 by the others.  A batch wider
// than the grid runs in rounds: workgroup b takes jobs b, b + grid, ...
//
// Replaces TFHEpp's GateBootstrappingTLWE2TLWEFFTvariableMu inside CircuitBootstrappingFFT<lvl02param, lvl21param> in front of the
// reference's ROM / RAM ports (TaskTFHEppCB*, /root/reference/src/iyokan_tfhepp.hpp:194-236), restated from the published algorithm.
#pragma once
#include "blind_rotate_core.hpp"   // TwistTab / make_twist, ntt32.hpp, goldilocks.hpp
#include "jobs.hpp"                // CbJob, CB_MAX_N0

namespace iyk {

static constexpr int CB_N = 2048;                 // N2
static constexpr int CB_LANES = 256;
static constexpr int CB_ROWS = 8;                 // (k+1) l2
static constexpr int CB_PSTRIDE = 2112;           // u64 words of one polynomial slot of the exchange buffer: max(32*65, 64*33, 2048)
static constexpr size_t CB_STEP_WORDS = (size_t)2 * CB_ROWS * 2 * CB_N;   // u64 words of one key step: [2 halves][8 rows][2 cols][N2]
static constexpr size_t CB_TORUS_STEP_WORDS = (size_t)CB_ROWS * 2 * CB_N; // u64 words of one step of the host key
static constexpr size_t CB_LDS_WORDS = 2 * CB_N + 4 * CB_PSTRIDE + 2 * CB_N + CB_N / 2;   // u64: acc, buf, twf + twi, abar (u32 [2048])
static constexpr size_t CB_LDS_BYTES = CB_LDS_WORDS * sizeof(u64);

template <int L2, int BGBIT2>
struct CbConsts {
    static_assert(L2 == 4, "the schedule runs the l2 digit polynomials of one accumulator polynomial on the four waves");
    static_assert(L2 * BGBIT2 < 64 && BGBIT2 <= 9, "digits of at most 9 bits: the exactness bound of the header");
    static constexpr u32 half_bg = 1u << (BGBIT2 - 1);
    static constexpr u32 mask = (1u << BGBIT2) - 1;
    static constexpr u64 offset_plus_round()
    {
        u64 o = 0;
        for (int j = 1; j <= L2; ++j) o += (u64)half_bg << (64 - j * BGBIT2);
        return o + (1ull << (64 - L2 * BGBIT2 - 1));
    }
    static constexpr TwistTab tw = make_twist(1);         // zeta^j2
    static constexpr TwistTab twk = make_twist(half_bg);  // (Bg/2) zeta^j2
};

IYK_HD u32 cb_modswitch_a(u32 a) { return (u32)(a + (1u << 19)) >> 20; }               // round, -> [0, 2 N2)
IYK_HD u32 cb_modswitch_b(u32 b) { return (2u * CB_N - (b >> 20)) & (2u * CB_N - 1); }  // truncate; the rotation of the test vector
// centred lift of a field element to the integers mod 2^64: x - P = x + 2^32 - 1 (mod 2^64)
IYK_HD u64 cb_lift(u64 x) { return x > (GL_P >> 1) ? x + GL_EPS : x; }

// gadget digit lvl < l2 (most significant first) of a word, as u = digit + Bg/2 in [0, Bg)
template <int L2, int BGBIT2>
IYK_HD u32 cb_digit_u(u64 x, int lvl)
{
    typedef CbConsts<L2, BGBIT2> C;
    return (u32)((x + C::offset_plus_round()) >> (64u - (u32)(lvl + 1) * BGBIT2)) & C::mask;
}

// ---- what a job's form decides: the mod switch, the test vector and the extraction; the step loop between them is one ---------------
// The per-digit job {in, sign, off, mu, out} shares nothing with its batch.  The many-digit job {in, sign, off, out} of DESIGN.md §6d
// shares CbManyMu {mu[0..l), l, bw}: the mod switch is coarser by bw bits and its values are multiples of 2^bw, the test vector
// interleaves the l constants with period 2^bw, and coefficients 0 .. l - 1 of the one accumulator are extracted into W2[out .. out + l).
// With l = 1 (bw = 0) every function below computes what its per-digit overload computes.  The kernels and their phases take what the
// batch shares as a trailing pack `k...`: empty for CbJob — the per-digit kernels keep their argument lists — and one CbManyMu for CbManyJob.

IYK_HD u32 cb_many_modswitch_a(u32 a, u32 bw) { return ((u32)(a + (1u << (19 + bw))) >> (20 + bw)) << bw; }   // round, multiples of 2^bw in [0, 2 N2)
IYK_HD u32 cb_many_modswitch_b(u32 b, u32 bw) { return (2u * CB_N - ((b >> (20 + bw)) << bw)) & (2u * CB_N - 1); }   // truncate
// mu[c], c < 4.  All four words are read first: a choice between the fields themselves is a choice between addresses, which keeps the
// kernel argument in scratch memory.
IYK_HD u64 cb_many_mu_at(const CbManyMu& k, u32 c)
{
    const u64 m0 = k.mu0, m1 = k.mu1, m2 = k.mu2, m3 = k.mu3;
    const u64 lo = (c & 1) ? m1 : m0, hi = (c & 1) ? m3 : m2;
    return (c & 2) ? hi : lo;
}

// abar of step i < n, and the rotation of the test vector (i == n), from the lvl0 word
IYK_HD u32 cb_abar(const CbJob& jb, const u32* w, u32 n, u32 i)
{
    const u32 v = (u32)jb.sign * w[i];
    return i == n ? cb_modswitch_b(v + jb.off) : cb_modswitch_a(v);
}
IYK_HD u32 cb_abar(const CbManyJob& jb, const u32* w, u32 n, u32 i, const CbManyMu& k)
{
    const u32 v = (u32)jb.sign * w[i];
    return i == n ? cb_many_modswitch_b(v + jb.off, k.bw) : cb_many_modswitch_a(v, k.bw);
}
// coefficient c < N2 of the test vector (mu[r] = 0 for r >= l is the host's)
IYK_HD u64 cb_tv(const CbJob& jb, u32) { return jb.mu; }
IYK_HD u64 cb_tv(const CbManyJob&, u32 c, const CbManyMu& k) { return cb_many_mu_at(k, c & ((1u << k.bw) - 1)); }
// lvl2 TLWEs a job writes
IYK_HD u32 cb_outputs() { return 1; }
IYK_HD u32 cb_outputs(const CbManyMu& k) { return k.l; }

// ---- the transform's passes; bp = one polynomial slot of the exchange buffer ----------------------------------------------------
// pass 1 forward, lane j1 < 64: x[j2] already twisted by zeta^j2.  Leaves Y[j1][k2] at bp[k2 * 65 + j1].
IYK_HD void cb_pass1_fwd(int j1, u64 (&x)[32], const u64* twf, u64* bp)
{
    ntt32_dif<LOG_W32>(x);
#pragma unroll
    for (int p = 0; p < 32; ++p) bp[brv5(p) * 65 + j1] = gl_mul(x[p], twf[brv5(p) * 64 + j1]);
}
// pass 2 forward, lane k2 < 32: on return position p holds X[k2 + 32 brv6(p)]
IYK_HD void cb_pass2_fwd_read(int k2, const u64* bp, u64 (&x)[64])
{
#pragma unroll
    for (int j1 = 0; j1 < 64; ++j1) x[j1] = bp[k2 * 65 + j1];
    ntt64_dif<LOG_ZETA>(x);
}
IYK_HD void cb_pass2_fwd_write(int k2, const u64 (&x)[64], u64* dst)   // natural order: dst[k]
{
#pragma unroll
    for (int p = 0; p < 64; ++p) dst[k2 + 32 * brv6(p)] = x[p];
}
// pass 1' inverse, lane k2 < 32: bp[k] natural.  On return position p holds Z[k2][j1 = brv6(p)], twiddled and scaled by 1 / N2.
IYK_HD void cb_pass1_inv_read(int k2, const u64* bp, const u64* twi, u64 (&x)[64])
{
#pragma unroll
    for (int k1 = 0; k1 < 64; ++k1) x[k1] = bp[k2 + 32 * k1];
    ntt64_dif<192 - LOG_ZETA>(x);
#pragma unroll
    for (int p = 0; p < 64; ++p) x[p] = gl_mul(x[p], twi[brv6(p) * 32 + k2]);
}
IYK_HD void cb_pass1_inv_write(int k2, const u64 (&x)[64], u64* bp)
{
#pragma unroll
    for (int p = 0; p < 64; ++p) bp[brv6(p) * 33 + k2] = x[p];
}
// pass 2' inverse, lane j1 < 64: on return position p holds coefficient j1 + 64 brv5(p), canonical
IYK_HD void cb_pass2_inv(int j1, const u64* bp, u64 (&y)[32])
{
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) y[k2] = bp[j1 * 33 + k2];
    ntt32_dif<192 - LOG_W32>(y);
#pragma unroll
    for (int p = 0; p < 32; ++p) y[p] = gl_mul_pow2(y[p], (192u - LOG_ZETA * (unsigned)brv5(p)) % 192u);
}

// ---- the phases of one rotation, per lane < 256; a workgroup barrier stands between any two of them ------------------------------
// abar[i] for i <= n (abar[n] = the test vector's rotation) and the initial accumulator
template <class Job, class... Shared>
IYK_HD void cb_prologue(int lane, const Job& jb, const u32* w, u32 n, u32* abar, u64* acc, const Shared&... k)
{
    for (u32 i = (u32)lane; i <= n; i += CB_LANES) abar[i] = cb_abar(jb, w, n, i, k...);
    const u32 rot = cb_abar(jb, w, n, n, k...);
#pragma unroll
    for (int q = 0; q < CB_N / CB_LANES; ++q) {
        const int j = lane + CB_LANES * q;
        const u32 idx = ((u32)j - rot) & (2 * CB_N - 1);
        const u64 t = cb_tv(jb, idx & (CB_N - 1), k...);
        acc[j] = 0;
        acc[CB_N + j] = (idx & CB_N) ? 0ull - t : t;
    }
}

// forward pass 1 of digit level lane >> 6 of accumulator polynomial h: the rotated difference is re-derived from the accumulator
template <int L2, int BGBIT2>
IYK_HD void cb_fwd1(int lane, int h, u32 abar, const u64* acc, const u64* twf, u64* buf)
{
    typedef CbConsts<L2, BGBIT2> C;
    const int lvl = lane >> 6, j1 = lane & 63;
    const u64* acc_h = acc + h * CB_N;
    u64 x[32];
#pragma unroll
    for (int j2 = 0; j2 < 32; ++j2) {
        const u32 idx = ((u32)(j1 + 64 * j2) - abar) & (2 * CB_N - 1);
        u64 v = acc_h[idx & (CB_N - 1)];
        v = (idx & CB_N) ? 0ull - v : v;
        const u64 td = v - acc_h[j1 + 64 * j2];
        const u32 u = cb_digit_u<L2, BGBIT2>(td, lvl);
        x[j2] = gl_sub(gl_mul_small(u, C::tw.c[j2]), C::twk.c[j2]);
    }
    cb_pass1_fwd(j1, x, twf, buf + lvl * CB_PSTRIDE);
}

struct alignas(16) CbPair {
    u64 v[2];
};

// accum[o * 8 + 2 q + e] += D_r[k] * BK2[half][h l2 + r][c][k] over the l2 rows of h, o = 2 c + half, k = 2 lane + 512 q + e
template <int L2>
IYK_HD void cb_mac(int lane, int h, const u64* buf, const u64* bk_step, u64 (&accum)[32])
{
#pragma unroll
    for (int r = 0; r < L2; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 2 * lane + 512 * q;
            const CbPair d = *reinterpret_cast<const CbPair*>(buf + r * CB_PSTRIDE + k);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int c = o >> 1, half = o & 1;
                const CbPair b = *reinterpret_cast<const CbPair*>(bk_step + ((size_t)((half * CB_ROWS + h * L2 + r) * 2 + c)) * CB_N + k);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    accum[o * 8 + 2 * q + e] = gl_add(accum[o * 8 + 2 * q + e], gl_mul_weak(d.v[e], b.v[e]));
            }
        }
    }
}

IYK_HD void cb_inv_write(int lane, const u64 (&accum)[32], u64* buf)
{
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            CbPair d;
            d.v[0] = accum[o * 8 + 2 * q], d.v[1] = accum[o * 8 + 2 * q + 1];
            *reinterpret_cast<CbPair*>(buf + o * CB_PSTRIDE + 2 * lane + 512 * q) = d;
        }
}

// inverse pass 2' of product o = lane >> 6 (output polynomial o >> 1, key half o & 1), lifted and added into the accumulator: the hi
// half enters shifted by 32.  Two lanes add into every word, in either order: integer addition mod 2^64.
IYK_HD void cb_inv2(int lane, const u64* buf, u64* acc)
{
    const int o = lane >> 6, j1 = lane & 63;
    u64 y[32];
    cb_pass2_inv(j1, buf + o * CB_PSTRIDE, y);
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

// word j <= N2 of SampleExtractIndex(acc, 0) + (0, .., 0, mu)
IYK_HD u64 cb_extract_word(const u64* acc, int j, u64 mu)
{
    if (j == CB_N) return acc[CB_N] + mu;
    return j == 0 ? acc[0] : 0ull - acc[CB_N - j];
}
// word j <= N2 of SampleExtractIndex(acc, r) + (0, .., 0, mu): the negated, reversed part starts behind index r
IYK_HD u64 cb_extract_word_at(const u64* acc, int j, u32 r, u64 mu)
{
    if (j == CB_N) return acc[CB_N + r] + mu;
    return (u32)j <= r ? acc[r - (u32)j] : 0ull - acc[CB_N + r - (u32)j];
}
IYK_HD u64 cb_out_word(const CbJob& jb, const u64* acc, int j, u32) { return cb_extract_word(acc, j, jb.mu); }
IYK_HD u64 cb_out_word(const CbManyJob&, const u64* acc, int j, u32 r, const CbManyMu& k) { return cb_extract_word_at(acc, j, r, cb_many_mu_at(k, r)); }
// a job's outputs from the finished accumulator, per lane < LANES: W2[out + r] for r < cb_outputs
template <int LANES, class Job, class... Shared>
IYK_HD void cb_epilogue(int lane, const Job& jb, const u64* acc, u64* tlwe2, const Shared&... k)
{
    for (u32 r = 0; r < cb_outputs(k...); ++r) {
        u64* row = tlwe2 + ((size_t)jb.out + r) * (CB_N + 1);
#pragma unroll
        for (int q = 0; q < CB_N / LANES; ++q) row[lane + LANES * q] = cb_out_word(jb, acc, lane + LANES * q, r, k...);
        if (lane == 0) row[CB_N] = cb_out_word(jb, acc, CB_N, r, k...);
    }
}

// ---- host-side tables: twf[k2 * 64 + j1] = psi^(j1 (2 k2 + 1)), twi[j1 * 32 + k2] = psi^(-j1 (2 k2 + 1)) / N2; psi^64 = 2^3 --------
inline u64 cb_find_psi()
{
    const u64 psi0 = gl_pow(7, (GL_P - 1) / (2 * CB_N));
    for (u64 u = 1; u < 64; u += 2) {
        const u64 cand = gl_pow(psi0, u);
        if (gl_pow(cand, 64) == 8) return cand;
    }
    return 0;  // unreachable: x -> x^64 maps the primitive 4096th roots onto all primitive 64th roots
}
inline void cb_make_tables(u64* twf, u64* twi)
{
    const u64 psi = cb_find_psi(), ipsi = gl_inv(psi), ninv = gl_inv(CB_N);
    for (int j1 = 0; j1 < 64; ++j1)
        for (int k2 = 0; k2 < 32; ++k2) {
            const u64 e = (u64)j1 * (2 * k2 + 1);
            twf[k2 * 64 + j1] = gl_pow(psi, e);
            twi[j1 * 32 + k2] = gl_mul(gl_pow(ipsi, e), ninv);
        }
}

#if defined(__HIPCC__)
// Key transform: torus-domain polynomials u64 [steps][8 rows][2 cols][N2] -> the two halves' spectra, u64 [steps][2][8][2][N2] natural k.
// One workgroup of 64 lanes per (polynomial, half).
__global__ __launch_bounds__(64) void bk2_ntt_kernel(const u64* __restrict__ torus, u64* __restrict__ dst, const u64* __restrict__ tw)
{
    __shared__ u64 xb[32 * 65];
    const int lane = threadIdx.x;
    const u32 poly = blockIdx.x >> 1, half = blockIdx.x & 1;
    const u32 step = poly / (CB_ROWS * 2), rc = poly % (CB_ROWS * 2);
    const u64* src = torus + (size_t)poly * CB_N;
    u64 x[32];
#pragma unroll
    for (int j2 = 0; j2 < 32; ++j2) {
        const u64 w = src[lane + 64 * j2];
        x[j2] = gl_mul_pow2(half ? w >> 32 : (u64)(u32)w, LOG_ZETA * j2);
    }
    cb_pass1_fwd(lane, x, tw, xb);
    __syncthreads();
    if (lane < 32) {
        u64 y[64];
        cb_pass2_fwd_read(lane, xb, y);
        cb_pass2_fwd_write(lane, y, dst + (size_t)step * CB_STEP_WORDS + ((size_t)half * CB_ROWS * 2 + rc) * CB_N);
    }
}

// grid: min(njobs, CUs) workgroups; workgroup b runs jobs b, b + grid, ... (rounds).  tw: twf then twi (2 x 2048 u64).
// <L2, BGBIT2>: the per-digit form, its arguments end at tlwe2; <L2, BGBIT2, CbManyJob, CbManyMu>: the many-digit form, k = one CbManyMu.
template <int L2, int BGBIT2, class Job = CbJob, class... Shared>
__global__ __launch_bounds__(CB_LANES) void cb_rotate_kernel(const Job* __restrict__ jobs, int njobs, const u32* __restrict__ tlwe0, u32 n,
                                                             const u64* __restrict__ bk, const u64* __restrict__ tw, u64* __restrict__ tlwe2,
                                                             const Shared... k)
{
    extern __shared__ __align__(16) u64 cb_lds[];
    u64* acc = cb_lds;
    u64* buf = acc + 2 * CB_N;
    u64* twf = buf + 4 * CB_PSTRIDE;
    u64* twi = twf + CB_N;
    u32* abar = reinterpret_cast<u32*>(twi + CB_N);
    const int lane = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 2 * CB_N / CB_LANES; ++q) twf[lane + CB_LANES * q] = tw[lane + CB_LANES * q];   // twf and twi are adjacent

    for (int job = blockIdx.x; job < njobs; job += gridDim.x) {
        const Job jb = jobs[job];
        cb_prologue(lane, jb, tlwe0 + (size_t)jb.in * (n + 1), n, abar, acc, k...);
        __syncthreads();
        for (u32 i = 0; i < n; ++i) {
            const u32 ab = abar[i];
            const u64* bk_step = bk + (size_t)i * CB_STEP_WORDS;
            u64 accum[32];
#pragma unroll
            for (int q = 0; q < 32; ++q) accum[q] = 0;
            u64 x[64];
            for (int h = 0; h < 2; ++h) {
                cb_fwd1<L2, BGBIT2>(lane, h, ab, acc, twf, buf);
                __syncthreads();
                if (lane < 128) cb_pass2_fwd_read(lane & 31, buf + (lane >> 5) * CB_PSTRIDE, x);
                __syncthreads();
                if (lane < 128) cb_pass2_fwd_write(lane & 31, x, buf + (lane >> 5) * CB_PSTRIDE);
                __syncthreads();
                cb_mac<L2>(lane, h, buf, bk_step, accum);
                __syncthreads();
            }
            cb_inv_write(lane, accum, buf);
            __syncthreads();
            if (lane < 128) cb_pass1_inv_read(lane & 31, buf + (lane >> 5) * CB_PSTRIDE, twi, x);
            __syncthreads();
            if (lane < 128) cb_pass1_inv_write(lane & 31, x, buf + (lane >> 5) * CB_PSTRIDE);
            __syncthreads();
            cb_inv2(lane, buf, acc);
            __syncthreads();
        }
        cb_epilogue<CB_LANES>(lane, jb, acc, tlwe2, k...);
        __syncthreads();   // the next round's prologue writes acc and abar
    }
}
#endif

}  // namespace iyk
