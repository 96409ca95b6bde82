// client.cpp — key generation, bit encryption and decryption for the hot path's inputs.
//
// Role in the reference: `iyokan-packet genkey / genevalkey / enc / dec`
// (/root/reference/src/iyokan-packet.cpp:144-178) and the in-process key set-up of test0
// (/root/reference/src/test0.cpp:535-546): SecretKey, then EvalKey with iksk<lvl10> and
// bk<lvl01> (torus-domain TRGSW per lvl0 key bit).  This is NOT on the GPU hot path; it
// exists so bench.py / tests / the host runtime can make real (non-trivial) ciphertexts —
// the reference's own GPU tests use trivial ones, which skip every CMUX
// (/root/reference/src/test0.cpp:702-710).  Built as libiyokan_client.so (plain C ABI).
//
// Randomness.  Every entry point takes (seed, deterministic):
//   deterministic == 0 (the default of the Python / C++ wrappers): masks, noise and keys come from a ChaCha20
//       stream keyed with 256 bits of getrandom(2) entropy drawn FOR THIS CALL; `seed` is ignored.  Two calls
//       never share a stream, so two encryptions never reuse a mask (c1 - c2 would leak m1 - m2).
//   deterministic != 0: xoshiro256** seeded with the 64-bit `seed` — reproducible fixtures for tests and
//       benchmarks ONLY; not a cryptographic generator, and the same seed gives the same masks.
//
// Layouts (shared with include/iyokan_hip.h):
//   TLWE lvl0      u32[n+1]                      a[0..n-1], b = a[n]
//   BK (torus)     u32[n][(k+1)l][k+1][N]        row r = c*l + j: TRLWE(0) + s0[i]*2^(32-(j+1)Bgbit) on poly c, coeff 0
//   KSK            u32[kN][t][2^basebit-1][n+1]  TLWE0( s1[i] * v * 2^(32-(j+1)basebit) ), v = idx+1
//   TLWE lvl2      u64[n_in+1]                   a[0..n_in-1], b = a[n_in]: 64-bit torus (the output level of circuit bootstrapping's rotation)
//   BK lvl2 (torus) u64[n][(k+1)l2][k+1][N2]     row r = c*l2 + j: TRLWE2(0) + s0[i]*2^(64-(j+1)Bgbit2) on poly c, coeff 0 (iyk_client_bk2_rows)
//   private KSK    u32[k+1][n_in+1][t][2^basebit-1][k+1][N]   row (c, i, j, u): TRLWE(0) + sigma_i (u+1) 2^(32-(j+1)basebit) on poly c,
//                                                coeff 0; sigma_i = s2[i], sigma_{n_in} = -1 (phase: f_c = 1 for c = 1, -s1(X) for c = 0)
//   seeded keys    the b polynomials of the two keys above alone, u32 [rows][N] / u64 [n][(k+1)l2][N2], plus a public 256-bit mask seed:
//                                                the a polynomials are key_expand.hpp's masks (iyk_client_*_seeded, iyk_client_expand_key_masks)
#include <sys/random.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/iyokan_hip_params.h"
#include "key_expand.hpp"

using namespace iyk;

namespace {

// 64-bit word source: xoshiro256** (seeded, reproducible) or ChaCha20 keyed from the OS (default)
class Rng {
    bool os_;
    uint64_t s[4];           // xoshiro state
    uint32_t key_[8];        // ChaCha20 key
    uint64_t ctr_ = 0;
    uint32_t blk_[16];
    int avail_ = 0;          // unread 64-bit words in blk_

    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    void chacha_block()   // state: words 12, 13 = the 64-bit block counter, 14, 15 = 0; the block function is key_expand.hpp's
    {
        uint32_t in[16];
        kx::chacha20_state(key_, (uint32_t)ctr_, (uint32_t)(ctr_ >> 32), 0, 0, in);
        ++ctr_;
        kx::chacha20_block(in, blk_);
        avail_ = 8;
    }

public:
    Rng(uint64_t seed, int deterministic) : os_(!deterministic)
    {
        if (os_) {
            size_t got = 0;
            while (got < sizeof(key_)) {
                const ssize_t r = getrandom((char*)key_ + got, sizeof(key_) - got, 0);
                if (r <= 0) {
                    std::fprintf(stderr, "[iyokan_client] fatal: getrandom failed\n");
                    std::abort();  // never fall back to a guessable key
                }
                got += (size_t)r;
            }
            return;
        }
        for (auto& v : s) {  // splitmix64
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            v = z ^ (z >> 31);
        }
    }
    uint64_t next()
    {
        if (os_) {
            if (!avail_) chacha_block();
            --avail_;
            return ((uint64_t)blk_[2 * avail_ + 1] << 32) | blk_[2 * avail_];
        }
        const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double gauss(double sigma)
    {
        double u1 = unit(), u2 = unit();
        if (u1 < 1e-300) u1 = 1e-300;
        return sigma * std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
    }
    // modular Gaussian on the torus, TFHEpp dtot32 convention
    uint32_t gauss_torus(double sigma)
    {
        double d = gauss(sigma);
        d -= std::floor(d);
        return (uint32_t)(int64_t)(d * 4294967296.0);
    }
};

void tlwe0_encrypt(const iyk_params* p, const uint32_t* s0, uint32_t msg, Rng& rng, uint32_t* ct)
{
    uint32_t b = msg + rng.gauss_torus(p->alpha0);
    for (uint32_t i = 0; i < p->n; ++i) {
        ct[i] = rng.u32();
        b += ct[i] * s0[i];
    }
    ct[p->n] = b;
}

// (a, b = a*s1 + e) with binary s1: a*s1 = sum over set bits of X^i * a
void trlwe_encrypt_zero(const iyk_params* p, const uint32_t* s1, Rng& rng, uint32_t* a, uint32_t* b)
{
    const uint32_t N = p->N;
    for (uint32_t x = 0; x < N; ++x) {
        a[x] = rng.u32();
        b[x] = rng.gauss_torus(p->alpha1);
    }
    for (uint32_t i = 0; i < N; ++i) {
        if (!s1[i]) continue;
        for (uint32_t x = 0; x < N - i; ++x) b[x + i] += a[x];
        for (uint32_t x = N - i; x < N; ++x) b[x + i - N] -= a[x];
    }
}

// b = a*s1 + e for a GIVEN a — the expanded mask of a seeded key row (key_expand.hpp): only the noise is drawn from rng
void trlwe_zero_b_of(const iyk_params* p, const uint32_t* s1, Rng& rng, const uint32_t* a, uint32_t* b)
{
    const uint32_t N = p->N;
    for (uint32_t x = 0; x < N; ++x) b[x] = rng.gauss_torus(p->alpha1);
    for (uint32_t i = 0; i < N; ++i) {
        if (!s1[i]) continue;
        for (uint32_t x = 0; x < N - i; ++x) b[x + i] += a[x];
        for (uint32_t x = N - i; x < N; ++x) b[x + i - N] -= a[x];
    }
}

// fn(lo, hi) over [0, total) on at most min(nthreads, 16, total) threads: the rows of a key window
template <class F>
void over_rows(uint64_t total, int nthreads, F fn)
{
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nthreads, 16, (int64_t)total}));
    if (nt == 1) {
        fn(0, total);
        return;
    }
    std::vector<std::thread> pool;
    for (int k = 0; k < nt; ++k) pool.emplace_back(fn, total * k / nt, total * (k + 1) / nt);
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" {

// s0[n], s1[N] are binary secret keys (one u32 per bit); bk / ksk sized by iyk_bk_words / iyk_ksk_words
int iyk_client_keygen(const iyk_params* p, uint64_t seed, int deterministic, uint32_t* s0, uint32_t* s1, uint32_t* bk,
                      uint32_t* ksk)
{
    if (!p || p->k != 1) return -1;
    Rng rng(seed, deterministic);
    for (uint32_t i = 0; i < p->n; ++i) s0[i] = rng.u32() & 1u;
    for (uint32_t i = 0; i < p->N; ++i) s1[i] = rng.u32() & 1u;

    const uint32_t N = p->N, rows = (p->k + 1) * p->l;
    for (uint32_t i = 0; i < p->n; ++i)
        for (uint32_t r = 0; r < rows; ++r) {
            uint32_t* row = bk + ((size_t)i * rows + r) * 2 * N;
            trlwe_encrypt_zero(p, s1, rng, row, row + N);
            const uint32_t c = r / p->l, j = r % p->l;
            row[c * N] += s0[i] << (32 - (j + 1) * p->Bgbit);
        }

    const uint32_t nb = (1u << p->basebit) - 1, n1 = p->n + 1;
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t j = 0; j < p->t; ++j)
            for (uint32_t v = 1; v <= nb; ++v) {
                uint32_t* row = ksk + (((size_t)i * p->t + j) * nb + (v - 1)) * n1;
                const uint32_t msg = (s1[i] * v) << (32 - (j + 1) * p->basebit);
                tlwe0_encrypt(p, s0, msg, rng, row);
            }
    return 0;
}

// bit b -> TLWE0(+-mu) with fresh noise (TFHEpp bootsSymEncrypt, /root/reference/src/packet.hpp:68-76)
int iyk_client_encrypt_bits(const iyk_params* p, const uint32_t* s0, uint64_t seed, int deterministic,
                            const uint8_t* bits, uint64_t count, uint32_t* out)
{
    Rng rng(seed, deterministic);
    for (uint64_t g = 0; g < count; ++g)
        tlwe0_encrypt(p, s0, bits[g] ? p->mu : 0u - p->mu, rng, out + g * (p->n + 1));
    return 0;
}

// bit = (int32)(b - <a,s>) > 0   (/root/reference/src/tfhepp_cufhe_wrapper.hpp:24-27)
int iyk_client_decrypt_bits(const iyk_params* p, const uint32_t* s0, const uint32_t* ct,
                            uint64_t count, uint8_t* bits)
{
    for (uint64_t g = 0; g < count; ++g) {
        const uint32_t* c = ct + g * (p->n + 1);
        uint32_t ph = c[p->n];
        for (uint32_t i = 0; i < p->n; ++i) ph -= c[i] * s0[i];
        bits[g] = (int32_t)ph > 0;
    }
    return 0;
}

// phases, for noise-margin checks
int iyk_client_phases(const iyk_params* p, const uint32_t* s0, const uint32_t* ct, uint64_t count,
                      uint32_t* phases)
{
    for (uint64_t g = 0; g < count; ++g) {
        const uint32_t* c = ct + g * (p->n + 1);
        uint32_t ph = c[p->n];
        for (uint32_t i = 0; i < p->n; ++i) ph -= c[i] * s0[i];
        phases[g] = ph;
    }
    return 0;
}

// TRLWE lvl1 encryptions of message polynomials (count x N torus words in, count x 2N words out: a(X) then b(X)):
// TFHEpp trlweSymEncrypt<Lvl1>(pmu, alpha1, key.lvl1) as PlainPacket::encrypt uses it for the CMUX memories' `ram` (one TRLWE
// per bit: +-mu in coefficient 0) and `rom` (N bits per TRLWE) maps, /root/reference/src/packet.hpp:78-122
int iyk_client_encrypt_trlwe(const iyk_params* p, const uint32_t* s1, uint64_t seed, int deterministic,
                             const uint32_t* msg, uint64_t count, uint32_t* out)
{
    Rng rng(seed, deterministic);
    const uint32_t N = p->N;
    for (uint64_t g = 0; g < count; ++g) {
        uint32_t* a = out + g * 2 * N;
        trlwe_encrypt_zero(p, s1, rng, a, a + N);
        for (uint32_t x = 0; x < N; ++x) a[N + x] += msg[g * N + x];
    }
    return 0;
}

// phase polynomials b - a * s1 of TRLWE lvl1 ciphertexts (count x 2N in, count x N out): trlweSymDecrypt's input
int iyk_client_trlwe_phases(const iyk_params* p, const uint32_t* s1, const uint32_t* ct, uint64_t count, uint32_t* phases)
{
    const uint32_t N = p->N;
    for (uint64_t g = 0; g < count; ++g) {
        const uint32_t* a = ct + g * 2 * N;
        uint32_t* ph = phases + g * N;
        for (uint32_t x = 0; x < N; ++x) ph[x] = a[N + x];
        for (uint32_t i = 0; i < N; ++i) {
            if (!s1[i]) continue;
            for (uint32_t x = 0; x < N - i; ++x) ph[x + i] -= a[x];
            for (uint32_t x = N - i; x < N; ++x) ph[x + i - N] += a[x];
        }
    }
    return 0;
}

// trivial ciphertext (a = 0, b = +-mu): HomCONSTANTONE / ZERO
// (/root/reference/src/tfhepp_cufhe_wrapper.hpp:29-37)
int iyk_client_trivial(const iyk_params* p, int bit, uint32_t* out)
{
    std::memset(out, 0, sizeof(uint32_t) * (p->n + 1));
    out[p->n] = bit ? p->mu : 0u - p->mu;
    return 0;
}

// ---- lvl2 (64-bit torus) and the private key-switching key: the client side of circuit bootstrapping's second half ----------------

// binary lvl2 key, one u32 per bit
int iyk_client_keygen_lvl2(uint32_t n_in, uint64_t seed, int deterministic, uint32_t* s2)
{
    Rng rng(seed, deterministic);
    for (uint32_t i = 0; i < n_in; ++i) s2[i] = rng.u32() & 1u;
    return 0;
}

// TLWE lvl2 of 64-bit torus messages: b = msg + <a, s2> + e, e Gaussian of standard deviation alpha (in units of the torus)
int iyk_client_encrypt_tlwe2(uint32_t n_in, const uint32_t* s2, uint64_t seed, int deterministic, double alpha, const uint64_t* msgs,
                             uint64_t count, uint64_t* out)
{
    Rng rng(seed, deterministic);
    for (uint64_t g = 0; g < count; ++g) {
        uint64_t* ct = out + g * ((uint64_t)n_in + 1);
        double d = rng.gauss(alpha);
        d -= std::rint(d);                                                  // [-1/2, 1/2]
        uint64_t b = msgs[g] + ((uint64_t)(int64_t)std::ldexp(d, 63) << 1);   // * 2^64 without leaving int64
        for (uint32_t i = 0; i < n_in; ++i) {
            ct[i] = rng.next();
            if (s2[i]) b += ct[i];
        }
        ct[n_in] = b;
    }
    return 0;
}

int iyk_client_tlwe2_phases(uint32_t n_in, const uint32_t* s2, const uint64_t* ct, uint64_t count, uint64_t* phases)
{
    for (uint64_t g = 0; g < count; ++g) {
        const uint64_t* c = ct + g * ((uint64_t)n_in + 1);
        uint64_t ph = c[n_in];
        for (uint32_t i = 0; i < n_in; ++i)
            if (s2[i]) ph -= c[i];
        phases[g] = ph;
    }
    return 0;
}

// Rows [first_row, first_row + row_count) of the private key-switching key, host layout (row index = ((c (n_in+1) + i) t + j) nb + u,
// nb = 2^basebit - 1).  Every row draws from a generator of its own — seeded from (seed, row index), or keyed from the OS — so a window
// holds the same words however the key is cut into windows and whatever nthreads is.  Noise: alpha1.
int iyk_client_privks_key_rows(const iyk_params* p, const uint32_t* s1, uint32_t n_in, const uint32_t* s2, uint32_t t, uint32_t basebit,
                               uint64_t first_row, uint64_t row_count, uint64_t seed, int deterministic, int nthreads, uint32_t* out)
{
    if (!p || p->k != 1 || basebit < 1 || basebit > 8 || t == 0 || (uint64_t)basebit * t > 63 || n_in == 0) return -1;
    const uint64_t nb = (1u << basebit) - 1, n1 = (uint64_t)n_in + 1, total = (p->k + 1) * n1 * t * nb;
    if (first_row > total || row_count > total - first_row) return -1;
    const uint32_t N = p->N;
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t q = lo; q < hi; ++q) {
            const uint64_t R = first_row + q;
            const uint32_t u = (uint32_t)(R % nb), j = (uint32_t)(R / nb % t), i = (uint32_t)(R / nb / t % n1), c = (uint32_t)(R / nb / t / n1);
            Rng rng(seed ^ (0xD1342543DE82EF95ull * (R + 1)), deterministic);
            uint32_t* row = out + q * 2 * N;
            trlwe_encrypt_zero(p, s1, rng, row, row + N);
            const uint32_t sh = (j + 1) * basebit;                              // digits below the 32-bit torus carry no message
            const uint32_t m = sh <= 32 ? (uint32_t)(((uint64_t)(u + 1) << (32 - sh)) & 0xFFFFFFFFu) : 0u;
            if (i == n_in) row[c * N] -= m;
            else if (s2[i]) row[c * N] += m;
        }
    };
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nthreads, 16, (int64_t)row_count}));
    if (nt == 1) {
        work(0, row_count);
        return 0;
    }
    std::vector<std::thread> pool;
    for (int k = 0; k < nt; ++k) pool.emplace_back(work, row_count * k / nt, row_count * (k + 1) / nt);
    for (auto& th : pool) th.join();
    return 0;
}

// Steps [first_step, first_step + step_count) of the lvl2 bootstrapping key of circuit bootstrapping's rotation: u64 [n][(k+1) l2][k+1][N2],
// N2 = 2048 = the size of s2 (the ring key whose coefficients are the lvl2 TLWE key of iyk_client_tlwe2_phases).  Row (i, r = c l2 + j) is a
// lvl2 TRLWE of zero (noise alpha2) plus s0[i] 2^(64 - (j+1) Bgbit2) at coefficient 0 of polynomial c: TFHEpp's bkgen<lvl02param> in the
// torus domain.  Every row draws from a generator of its own — seeded from (seed, row index), or keyed from the OS — so a window holds the
// same words however the key is cut and whatever nthreads is.
int iyk_client_bk2_rows(uint32_t n, const uint32_t* s0, uint32_t N2, const uint32_t* s2, uint32_t l2, uint32_t Bgbit2, double alpha2,
                        uint64_t first_step, uint64_t step_count, uint64_t seed, int deterministic, int nthreads, uint64_t* out)
{
    if (!s0 || !s2 || !out || n == 0 || N2 == 0 || l2 == 0 || Bgbit2 == 0 || (uint64_t)l2 * Bgbit2 > 63) return -1;
    if (first_step > n || step_count > n - first_step) return -1;
    const uint64_t rows = 2ull * l2, total = step_count * rows;
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t q = lo; q < hi; ++q) {
            const uint64_t R = first_step * rows + q, i = R / rows, r = R % rows;
            Rng rng(seed ^ (0xA0761D6478BD642Full * (R + 1)), deterministic);
            uint64_t* a = out + q * 2 * N2;
            uint64_t* b = a + N2;
            for (uint32_t x = 0; x < N2; ++x) {
                a[x] = rng.next();
                double d = rng.gauss(alpha2);
                d -= std::rint(d);
                b[x] = (uint64_t)(int64_t)std::ldexp(d, 63) << 1;
            }
            for (uint32_t t = 0; t < N2; ++t) {
                if (!s2[t]) continue;
                for (uint32_t x = 0; x < N2 - t; ++x) b[x + t] += a[x];
                for (uint32_t x = N2 - t; x < N2; ++x) b[x + t - N2] -= a[x];
            }
            const uint64_t c = r / l2, j = r % l2;
            if (s0[i]) out[q * 2 * N2 + c * N2] += 1ull << (64 - (j + 1) * Bgbit2);
        }
    };
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nthreads, 16, (int64_t)total}));
    if (nt == 1) {
        work(0, total);
        return 0;
    }
    std::vector<std::thread> pool;
    for (int k = 0; k < nt; ++k) pool.emplace_back(work, total * k / nt, total * (k + 1) / nt);
    for (auto& th : pool) th.join();
    return 0;
}

// ---- seeded keys (key_expand.hpp): the client sends the b halves and a PUBLIC 256-bit mask seed, the masks are regenerated -----------
//
// A seeded row is (a', b) with a' = the expanded mask of (mask_seed, kind, host row index) and the phase of the unseeded row: a message
// v on polynomial 1 is b[0] += v as before; a message v on polynomial 0 (the unseeded row is (a + v, b), phase e - v s(X)) becomes
// b -= v s(X), since a' itself cannot move.  Noise and nothing else comes from the row's private generator, seeded as in the unseeded
// call; the mask seed must be fresh per key.

// key_expand.hpp's block function on a whole state of 16 words (RFC 8439 §2.3): the one copy every generator here runs, for tests
int iyk_client_chacha20_block(const uint32_t* state, uint32_t* out)
{
    if (!state || !out || state == out) return -1;
    kx::chacha20_block(state, out);
    return 0;
}

// The masks themselves: rows [first_row, first_row + row_count) of kind `kind`, words_per_row u32 words each (N of the private key,
// 2 N2 of the lvl2 key: a[m] = w[2m] | w[2m+1] << 32) -> out u32 [row_count][words_per_row].  first_row is any 64-bit row index.
int iyk_client_expand_key_masks(uint32_t kind, const uint8_t* mask_seed, uint64_t first_row, uint64_t row_count, uint64_t words_per_row,
                                uint32_t* out)
{
    if (!mask_seed || !out || (kind != kx::KIND_PRIVKS && kind != kx::KIND_BK2) || words_per_row == 0 ||
        words_per_row > (uint64_t)kx::BLOCK_WORDS << 32 || row_count > UINT64_MAX - first_row)
        return -1;
    const kx::MaskKey key = kx::mask_key_of(mask_seed);
    for (uint64_t q = 0; q < row_count; ++q) kx::mask_row(key, kind, first_row + q, words_per_row, out + q * words_per_row);
    return 0;
}

// iyk_client_privks_key_rows for a seeded key: out_b u32 [row_count][N], the b polynomials of the rows
int iyk_client_privks_key_rows_seeded(const iyk_params* p, const uint32_t* s1, uint32_t n_in, const uint32_t* s2, uint32_t t, uint32_t basebit,
                                      const uint8_t* mask_seed, uint64_t first_row, uint64_t row_count, uint64_t seed, int deterministic,
                                      int nthreads, uint32_t* out_b)
{
    if (!p || p->k != 1 || basebit < 1 || basebit > 8 || t == 0 || (uint64_t)basebit * t > 63 || n_in == 0 || !mask_seed || !out_b) return -1;
    const uint64_t nb = (1u << basebit) - 1, n1 = (uint64_t)n_in + 1, total = (p->k + 1) * n1 * t * nb;
    if (first_row > total || row_count > total - first_row) return -1;
    const uint32_t N = p->N;
    const kx::MaskKey key = kx::mask_key_of(mask_seed);
    over_rows(row_count, nthreads, [&](uint64_t lo, uint64_t hi) {
        std::vector<uint32_t> a(N);
        for (uint64_t q = lo; q < hi; ++q) {
            const uint64_t R = first_row + q;
            const uint32_t u = (uint32_t)(R % nb), j = (uint32_t)(R / nb % t), i = (uint32_t)(R / nb / t % n1), c = (uint32_t)(R / nb / t / n1);
            Rng rng(seed ^ (0xD1342543DE82EF95ull * (R + 1)), deterministic);
            uint32_t* b = out_b + q * N;
            kx::mask_row(key, kx::KIND_PRIVKS, R, N, a.data());
            trlwe_zero_b_of(p, s1, rng, a.data(), b);
            const uint32_t sh = (j + 1) * basebit;
            const uint32_t m = sh <= 32 ? (uint32_t)(((uint64_t)(u + 1) << (32 - sh)) & 0xFFFFFFFFu) : 0u;
            const uint32_t v = i == n_in ? 0u - m : s2[i] ? m : 0u;
            if (c == 1) b[0] += v;
            else
                for (uint32_t x = 0; x < N; ++x)
                    if (s1[x]) b[x] -= v;
        }
    });
    return 0;
}

// iyk_client_bk2_rows for a seeded key: out_b u64 [step_count][(k+1) l2][N2], the b polynomials of the rows
int iyk_client_bk2_rows_seeded(uint32_t n, const uint32_t* s0, uint32_t N2, const uint32_t* s2, uint32_t l2, uint32_t Bgbit2, double alpha2,
                               const uint8_t* mask_seed, uint64_t first_step, uint64_t step_count, uint64_t seed, int deterministic,
                               int nthreads, uint64_t* out_b)
{
    if (!s0 || !s2 || !out_b || !mask_seed || n == 0 || N2 == 0 || l2 == 0 || Bgbit2 == 0 || (uint64_t)l2 * Bgbit2 > 63) return -1;
    if (first_step > n || step_count > n - first_step) return -1;
    const uint64_t rows = 2ull * l2, total = step_count * rows;
    const kx::MaskKey key = kx::mask_key_of(mask_seed);
    over_rows(total, nthreads, [&](uint64_t lo, uint64_t hi) {
        std::vector<uint32_t> w(2 * (size_t)N2);
        std::vector<uint64_t> a(N2);
        for (uint64_t q = lo; q < hi; ++q) {
            const uint64_t R = first_step * rows + q, i = R / rows, r = R % rows;
            Rng rng(seed ^ (0xA0761D6478BD642Full * (R + 1)), deterministic);
            uint64_t* b = out_b + q * N2;
            kx::mask_row(key, kx::KIND_BK2, R, 2 * (uint64_t)N2, w.data());
            for (uint32_t x = 0; x < N2; ++x) {
                a[x] = (uint64_t)w[2 * x] | (uint64_t)w[2 * x + 1] << 32;
                double d = rng.gauss(alpha2);
                d -= std::rint(d);
                b[x] = (uint64_t)(int64_t)std::ldexp(d, 63) << 1;
            }
            for (uint32_t s = 0; s < N2; ++s) {
                if (!s2[s]) continue;
                for (uint32_t x = 0; x < N2 - s; ++x) b[x + s] += a[x];
                for (uint32_t x = N2 - s; x < N2; ++x) b[x + s - N2] -= a[x];
            }
            const uint64_t c = r / l2, j = r % l2;
            const uint64_t v = s0[i] ? 1ull << (64 - (j + 1) * Bgbit2) : 0ull;
            if (c == 1) b[0] += v;
            else
                for (uint32_t x = 0; x < N2; ++x)
                    if (s2[x]) b[x] -= v;
        }
    });
    return 0;
}

}  // extern "C"
