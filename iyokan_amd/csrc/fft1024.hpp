// fft1024.hpp — the negacyclic product mod (X^2048 + 1) of integer polynomials through a 1024-point COMPLEX FP64 FFT, exact by the
// rounding bound of DESIGN.md §2b (lvl2 row), laid out for one 64-lane wavefront per polynomial with 16 complex points per lane.
// The lvl2 counterpart of fft512.hpp: the same fold, twist and cyclic DFT, one size up, for the circuit bootstrapping rotation
// (cb_rotate_fft.hpp).
//
// Mathematics.  For a real polynomial a of degree < N = 2048 put M = N/2 = 1024, psi = exp(i pi / N), W = psi^4 = exp(2 pi i / M):
//     z[j]  = a[j] + i a[j + M]                       (fold)
//     A[k]  = sum_j z[j] psi^j W^(jk) = a(psi^(4k+1)) (twist + cyclic DFT_M)
// so (a * b mod X^N + 1) <-> A[k] B[k], and back by z[j] = psi^-j (1/M) sum_k C[k] W^(-jk); the 1/M is folded into the key spectrum.
//
// Index split: j = j1 + 64 j2 (j1 < 64, j2 < 16), k = k2 + 16 k1 (k2 < 16, k1 < 64); j1 = a + 4 b (a < 4, b < 16), k1 = c + 16 d (c < 16, d < 4):
//     W^(jk) = W^(j1 k2) * W16^(j2 k2) * W64^(a c) * W16^(b c) * W4^(a d)
//   pass 1   lane j1, registers j2:            twist psi^j (TW0), DFT16 over j2 -> k2, times T1[k2][j1] = W^(j1 k2)
//   exchange 1 (LDS, inside the wave):         -> lane' = 4 k2 + a, registers b
//   pass 2   DFT16 over b -> c, times T2[c][a] = W64^(a c)
//   exchange 2:                                -> lane'' = 4 k2 + g, registers 4 cl + a with c = 4 g + cl
//   pass 3   four DFT4 over a -> d;            register r = 4 cl + d holds frequency k = k2 + 16 (4 g + cl + 16 d)
// The spectrum is stored in POSITION order, pos = lane'' + 64 r (a wave's stores are contiguous): the products are pointwise, the key
// spectra are stored by the same transform in the same order, and the inverse reads that order, so natural order is never needed
// (freq_of_pos() names the frequency of a position for the tests).  The inverse runs the network backwards with conjugated constants.
// Both exchanges happen in place in the polynomial's own slot of 1024 points; the words of one k2 form a block of 64 whose index is
// XORed with 4 k2, so that the 16 lanes of one a (or g) do not all fall on one bank group.
// Every DFT16 / DFT4 is radix-2 in registers with literal constants: per transform 10 butterfly layers and at most 7 multiplicative
// ones on any path (twist, two inside each DFT16 — the layers with w16^m and w8^m; w4^m and w2^m are +-1, +-i — T1 and T2).
//
// The same functions run lane by lane on the CPU (csrc/emul.cpp) for the GPU-less tests.
#pragma once
#include "fft512.hpp"   // cplx, cmul, cmulc, fma_, MAGIC, round_err

namespace iyk {
namespace fft1k {

using fft::cplx;

static constexpr int M = 1024;                     // complex points per polynomial
static constexpr int TAB_TW0 = 0, TAB_T1 = M, TAB_T2 = 2 * M;
static constexpr int TAB_POINTS = 2 * M + 64;      // TW0[j2 * 64 + j1], T1[k2 * 64 + j1], T2[c * 4 + a]

// exp(2 pi i m / 16), m < 8
static constexpr double C8 = 0.92387953251128675613, S8 = 0.38268343236508977173, R2 = fft::RSQRT2;
IYK_HD cplx w16(int m)
{
    switch (m) {
    case 1: return {C8, S8};
    case 2: return {R2, R2};
    case 3: return {S8, C8};
    case 5: return {-S8, C8};
    case 6: return {-R2, R2};
    default: return {-C8, S8};   // 7
    }
}

IYK_HD constexpr int brv_bits(int p, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((p >> b) & 1) << (bits - 1 - b);
    return r;
}

// n-point DFT (n = 4 or 16) in registers, natural order in and out: X[k] = sum_m x[m] e^(+-2 pi i m k / n) (+: forward, -: INV).
// Radix-2 decimation in frequency; the twiddle of a butterfly is w16^(m 8 / h): 1 and +-i cost nothing, the others one complex product.
template <int LOGN, bool INV>
IYK_HD void dft(cplx (&x)[1 << LOGN])
{
    constexpr int N = 1 << LOGN;
#pragma unroll
    for (int s = 0; s < LOGN; ++s) {
        const int h = (N / 2) >> s;   // the butterflies' span
#pragma unroll
        for (int t = 0; t < N / 2; ++t) {
            const int m = t & (h - 1), lo = ((t >> (LOGN - 1 - s)) << (LOGN - s)) + m, hi = lo + h;
            const cplx a = x[lo], b = x[hi];
            x[lo] = fft::cadd(a, b);
            const cplx d = fft::csub(a, b);
            const int e = m * (8 / h);   // of w16
            if (e == 0) x[hi] = d;
            else if (e == 4) x[hi] = INV ? cplx{d.im, -d.re} : cplx{-d.im, d.re};
            else x[hi] = INV ? fft::cmulc(d, w16(e)) : fft::cmul(d, w16(e));
        }
    }
    cplx y[N];
#pragma unroll
    for (int p = 0; p < N; ++p) y[brv_bits(p, LOGN)] = x[p];
#pragma unroll
    for (int p = 0; p < N; ++p) x[p] = y[p];
}

// host-generated in long double, rounded once
inline void make_tables(cplx* tab)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    auto e = [&](long num, long den) { return cplx{(double)cosl(pi * num / den), (double)sinl(pi * num / den)}; };   // exp(i pi num / den)
    for (int j2 = 0; j2 < 16; ++j2)
        for (int j1 = 0; j1 < 64; ++j1) tab[TAB_TW0 + j2 * 64 + j1] = e(j1 + 64 * j2, 2048);
    for (int k2 = 0; k2 < 16; ++k2)
        for (int j1 = 0; j1 < 64; ++j1) tab[TAB_T1 + k2 * 64 + j1] = e(2 * ((j1 * k2) % 1024), 1024);
    for (int c = 0; c < 16; ++c)
        for (int a = 0; a < 4; ++a) tab[TAB_T2 + c * 4 + a] = e(2 * ((a * c) % 64), 64);
}

// ---- slot indices of the two exchanges and of the spectrum ---------------------------------------------------------------------------
IYK_HD int x1_index(int k2, int j1) { return k2 * 64 + (j1 ^ (4 * k2)); }           // Y[j1][k2]
IYK_HD int x2_index(int k2, int c, int a) { return k2 * 64 + ((4 * c + a) ^ (4 * k2)); }
IYK_HD constexpr int freq_of_pos(int pos)
{
    const int L = pos & 63, r = pos >> 6;
    return (L >> 2) + 16 * (4 * (L & 3) + (r >> 2) + 16 * (r & 3));
}

// ---- forward: x[j2] = z[j1 + 64 j2] on entry of fwd1; sp = the polynomial's slot; a wave-level ordering point between any two ----------
IYK_HD void fwd1(int j1, cplx (&x)[16], const cplx* tab, cplx* sp)
{
#pragma unroll
    for (int j2 = 0; j2 < 16; ++j2) x[j2] = fft::cmul(x[j2], tab[TAB_TW0 + j2 * 64 + j1]);
    dft<4, false>(x);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) sp[x1_index(k2, j1)] = fft::cmul(x[k2], tab[TAB_T1 + k2 * 64 + j1]);
}
IYK_HD void fwd2_read(int L, const cplx* tab, const cplx* sp, cplx (&x)[16])
{
    const int k2 = L >> 2, a = L & 3;
#pragma unroll
    for (int b = 0; b < 16; ++b) x[b] = sp[x1_index(k2, a + 4 * b)];
    dft<4, false>(x);
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = fft::cmul(x[c], tab[TAB_T2 + c * 4 + a]);
}
IYK_HD void fwd2_write(int L, const cplx (&x)[16], cplx* sp)
{
    const int k2 = L >> 2, a = L & 3;
#pragma unroll
    for (int c = 0; c < 16; ++c) sp[x2_index(k2, c, a)] = x[c];
}
IYK_HD void fwd3_read(int L, const cplx* sp, cplx (&x)[16])
{
    const int k2 = L >> 2, g = L & 3;
#pragma unroll
    for (int cl = 0; cl < 4; ++cl) {
        cplx y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) y[a] = sp[x2_index(k2, 4 * g + cl, a)];
        dft<2, false>(y);
#pragma unroll
        for (int d = 0; d < 4; ++d) x[4 * cl + d] = y[d];
    }
}
IYK_HD void spec_write(int L, const cplx (&x)[16], cplx* sp)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) sp[L + 64 * r] = x[r];
}

// ---- inverse: the same network backwards, conjugated, unscaled ------------------------------------------------------------------------
IYK_HD void inv3_read(int L, const cplx* sp, cplx (&x)[16])
{
#pragma unroll
    for (int cl = 0; cl < 4; ++cl) {
        cplx y[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) y[d] = sp[L + 64 * (4 * cl + d)];
        dft<2, true>(y);
#pragma unroll
        for (int a = 0; a < 4; ++a) x[4 * cl + a] = y[a];
    }
}
IYK_HD void inv3_write(int L, const cplx (&x)[16], cplx* sp)
{
    const int k2 = L >> 2, g = L & 3;
#pragma unroll
    for (int cl = 0; cl < 4; ++cl)
#pragma unroll
        for (int a = 0; a < 4; ++a) sp[x2_index(k2, 4 * g + cl, a)] = x[4 * cl + a];
}
IYK_HD void inv2_read(int L, const cplx* tab, const cplx* sp, cplx (&x)[16])
{
    const int k2 = L >> 2, a = L & 3;
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = fft::cmulc(sp[x2_index(k2, c, a)], tab[TAB_T2 + c * 4 + a]);
    dft<4, true>(x);
}
IYK_HD void inv2_write(int L, const cplx (&x)[16], cplx* sp)
{
    const int k2 = L >> 2, a = L & 3;
#pragma unroll
    for (int b = 0; b < 16; ++b) sp[x1_index(k2, a + 4 * b)] = x[b];
}
// on return x[j2] = z[j1 + 64 j2] (times M)
IYK_HD void inv1(int j1, const cplx* tab, const cplx* sp, cplx (&x)[16])
{
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) x[k2] = fft::cmulc(sp[x1_index(k2, j1)], tab[TAB_T1 + k2 * 64 + j1]);
    dft<4, true>(x);
#pragma unroll
    for (int j2 = 0; j2 < 16; ++j2) x[j2] = fft::cmulc(x[j2], tab[TAB_TW0 + j2 * 64 + j1]);
}

// rint(x) as a signed integer for |x| < 2^51: x + 1.5 * 2^52 has the exponent of the constant, so the difference of the bit patterns
// IS the integer (the 64-bit recombination needs the signed value, not only its low 32 bits)
IYK_HD int64_t round_i64(double x)
{
    const double t = x + fft::MAGIC, m = fft::MAGIC;
    int64_t b, c;
    __builtin_memcpy(&b, &t, 8);
    __builtin_memcpy(&c, &m, 8);
    return b - c;
}

// signed 16-bit quarter j of a key word: k = q0 + 2^16 q1 + 2^32 q2 + 2^48 q3 (mod 2^64), all in [-2^15, 2^15); carries move upward
// and the one out of q3 drops out
IYK_HD int32_t key_quarter(u64 k, int j)
{
    int32_t q = 0;
    for (int t = 0; t <= j; ++t) {
        q = (int32_t)(int16_t)(k & 0xFFFFu);
        k = (k - (u64)(int64_t)q) >> 16;
    }
    return q;
}
// R_0 + (R_1 << 16) + (R_2 << 32) + (R_3 << 48) mod 2^64
IYK_HD u64 recombine(const int64_t (&R)[4]) { return (u64)R[0] + ((u64)R[1] << 16) + ((u64)R[2] << 32) + ((u64)R[3] << 48); }

}  // namespace fft1k
}  // namespace iyk
