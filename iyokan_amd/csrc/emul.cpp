// emul.cpp — CPU lane-by-lane execution of the blind-rotate kernel's phase functions
// (blind_rotate_core.hpp).  TEST SUPPORT: lets tests/test_kernel_emulation.py check the
// kernel's exact data flow (index maps, transposes, MAC, lift) against the oracle in this
// GPU-less container.  Not loaded by the product path.  Built as libiyk_emul.so.
#include <cmath>
#include <algorithm>
#include <cstdint>
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/iyokan_hip_params.h"
#include "blind_rotate_core.hpp"
#include "blind_rotate_fp.hpp"
#include "blind_rotate_lat3.hpp"
#include "blind_rotate_t16.hpp"
#include "blind_rotate_fft.hpp"
#include "cmux_fft.hpp"
#include "fft256.hpp"
#include "batch_args.hpp"
#include "dispatch.hpp"
#include "privks.hpp"
#include "cb_rotate.hpp"
#include "cb_rotate_lat.hpp"
#include "cb_rotate_fft.hpp"
#include "key_expand.hpp"

using namespace iyk;

namespace {
struct Tables {
    std::vector<u64> fwd, inv;
    Tables() : fwd(1024), inv(1024) { ntt_make_tables(fwd.data(), inv.data()); }
};
const Tables& tables()
{
    static Tables t;
    return t;
}

// forward transform of one polynomial into the device BK layout (bk_dev_index within a polynomial)
void forward_1024_dev(const u64* in, u64* out)
{
    const Tables& T = tables();
    static thread_local u64 xbuf[32 * XB_STRIDE];
    u64 x[32];
    for (int t = 0; t < 32; ++t) {
        for (int j2 = 0; j2 < 32; ++j2) x[j2] = in[t + 32 * j2];
        ntt_fwd_pass1(x, T.fwd.data() + t * 32);
        for (int p = 0; p < 32; ++p) xbuf[brv5(p) * XB_STRIDE + t] = x[p];
    }
    for (int t = 0; t < 32; ++t) {
        for (int j1 = 0; j1 < 32; ++j1) x[j1] = xbuf[t * XB_STRIDE + j1];
        ntt_fwd_pass2(x);
        for (int p = 0; p < 32; ++p) {
            const int k1 = brv5(p);
            out[(size_t)(k1 >> 1) * 64 + t * 2 + (k1 & 1)] = x[p];
        }
    }
}

// lane-by-lane run of kernels.hpp::blind_rotate_kernel (same phase functions, same order,
// one loop over the 64 lanes wherever the kernel has an lds_sync)
template <int L, int BGBIT>
void blind_rotate(const iyk_params* p, const u32* lin, const u64* bk_ntt, u32* tlwe1)
{
    const Tables& T = tables();
    std::vector<u64> twf_t(NTT_N), twi_t(NTT_N);
    for (int e = 0; e < NTT_N; ++e) {
        const int a = e >> 5, b = e & 31;
        twf_t[b * 32 + a] = T.fwd[e];
        twi_t[b * 32 + a] = T.inv[e];
    }
    std::vector<u32> wave_lds(BR_WAVE_LDS_WORDS + 2);  // +2: keep the u64 view of xb 8-byte aligned
    u32* acc_lds = wave_lds.data() + ((reinterpret_cast<uintptr_t>(wave_lds.data()) & 7) ? 1 : 0);
    struct Lane {
        u32 lo[32];
        u64 x[32], accum[32];
    };
    std::vector<Lane> R(64);
    auto acc_h = [&](int lane) { return acc_lds + (lane >> 5) * NTT_N; };
    auto xb = [&](int lane) { return acc_lds + 2 * NTT_N + (lane >> 5) * XB_WORDS32; };
    auto xb64_own = [&](int lane) { return reinterpret_cast<u64*>(xb(lane)); };
    auto xb64_oth = [&](int lane) {
        return reinterpret_cast<const u64*>(acc_lds + 2 * NTT_N + (1 - (lane >> 5)) * XB_WORDS32);
    };
#define ALL_LANES for (int lane = 0; lane < 64; ++lane)

    const u32 bbar = br_modswitch_b(lin[p->n]);
    ALL_LANES br_init_acc(lane >> 5, lane & 31, bbar, p->mu, acc_h(lane));

    for (u32 i = 0; i < p->n; ++i) {
        const u32 abar = br_modswitch_a(lin[i]);
        const u64* bk_step = bk_ntt + (size_t)i * (2 * L) * 2 * NTT_N;
        ALL_LANES for (int q = 0; q < 32; ++q) R[lane].accum[q] = 0;
        for (int pass = 0; pass < 2 * L + 2; ++pass) {
            const int lvl = pass >> 1;
            const bool fwd = pass < 2 * L, first = (pass & 1) == 0;
            ALL_LANES
            {
                Lane& r = R[lane];
                if (first) {
                    if (fwd) br_fwd1_pre<L, BGBIT>(lane & 31, lvl, abar, acc_h(lane), r.x);
                    else
                        for (int q = 0; q < 32; ++q) r.x[q] = r.accum[q];
                }
                ntt32_dif<LOG_W32>(r.x);
            }
            if (first) {
                ALL_LANES
                {
                    if (fwd) {
                        br_fwd1_twiddle(lane & 31, R[lane].x, twf_t.data());
                        br_xpose_write<false>(lane & 31, R[lane].x, xb(lane), false);
                    }
                    else {
                        br_inv1_twiddle(lane & 31, R[lane].x, twi_t.data());
                        br_xpose_write<true>(lane & 31, R[lane].x, xb(lane), false);
                    }
                }
                ALL_LANES br_xpose_read_lo(lane & 31, R[lane].lo, xb(lane));
                ALL_LANES
                {
                    if (fwd) br_xpose_write<false>(lane & 31, R[lane].x, xb(lane), true);
                    else br_xpose_write<true>(lane & 31, R[lane].x, xb(lane), true);
                }
                ALL_LANES br_xpose_read_hi(lane & 31, R[lane].x, R[lane].lo, xb(lane));
            }
            else if (fwd) {
                for (int chunk = 0; chunk < 2; ++chunk) {
                    ALL_LANES br_share_write(lane & 31, chunk, R[lane].x, xb64_own(lane));
                    ALL_LANES
                    {
                        const int h = lane >> 5, t = lane & 31;
                        const u64* bko = bk_row_own<L>(bk_step, h, t, lvl);
                        const u64* bkt = bk_row_oth<L>(bk_step, h, t, lvl);
                        for (int m = chunk * 8; m < chunk * 8 + 8; ++m) {
                            const u64 bo[2] = {bko[m * 64], bko[m * 64 + 1]};
                            const u64 bt[2] = {bkt[m * 64], bkt[m * 64 + 1]};
                            br_mac_pair(t, m, R[lane].x, xb64_oth(lane), bo, bt, R[lane].accum);
                        }
                    }
                }
            }
            else {
                ALL_LANES br_inv2_post(lane & 31, R[lane].x, acc_h(lane));
            }
        }
    }
    tlwe1[0] = acc_lds[0];
    for (u32 j = 1; j < (u32)NTT_N; ++j) tlwe1[j] = 0u - acc_lds[NTT_N - j];
    tlwe1[NTT_N] = acc_lds[NTT_N];
#undef ALL_LANES
}
// ---------------------------------------------------------------------------------------------
// FP64 path (fp50.hpp): same lane-by-lane emulation of kernels.hpp::blind_rotate_fp_kernel
struct FpTables {
    fp::HostTables t;
    std::vector<double> twf_t, twi_t;
    FpTables() : twf_t(NTT_N), twi_t(NTT_N)
    {
        fp::make_tables(t);
        for (int e = 0; e < NTT_N; ++e) {
            const int a = e >> 5, b = e & 31;
            twf_t[b * 32 + a] = t.tw_fwd[e];
            twi_t[b * 32 + a] = t.tw_inv[e];
        }
    }
};
const FpTables& fptables()
{
    static FpTables t;
    return t;
}

double g_fp_maxabs = 0.0;  // largest |value| / p seen (magnitude discipline check)
inline void track(const double (&x)[32])
{
    for (double v : x) {
        const double a = (v < 0 ? -v : v) / fp::P;
        if (a > g_fp_maxabs) g_fp_maxabs = a;
    }
}

void forward_1024_fp_dev(const double* in, double* out)
{
    const FpTables& T = fptables();
    static thread_local double xbuf[32 * XB_STRIDE];
    double x[32];
    for (int t = 0; t < 32; ++t) {
        for (int j2 = 0; j2 < 32; ++j2) x[j2] = j2 ? fp::mulmod(in[t + 32 * j2], T.t.c.zf[j2]) : in[t];
        fp::ntt32_dif<fp::PASS1>(x, T.t.c.w);
        for (int p = 0; p < 32; ++p) xbuf[brv5(p) * XB_STRIDE + t] = fp::mulmod(x[p], T.t.tw_fwd[t * 32 + brv5(p)]);
    }
    for (int t = 0; t < 32; ++t) {
        for (int j1 = 0; j1 < 32; ++j1) x[j1] = xbuf[t * XB_STRIDE + j1];
        fp::ntt32_dif<fp::PASS2>(x, T.t.c.w);
        for (int p = 0; p < 32; ++p) {
            const int k1 = brv5(p);
            out[(size_t)(k1 >> 1) * 64 + t * 2 + (k1 & 1)] = fp::norm(x[p]);
        }
    }
}

template <class D>
void blind_rotate_fp(const iyk_params* p, const u32* lin, const double* bk_ntt, u32* tlwe1)
{
    constexpr int L = D::LV;
    const FpTables& T = fptables();
    const fp::NttConsts& C = T.t.c;
    std::vector<double> ztab(fp::ZTAB_ENTRIES);  // the workgroup's twisted-digit table (LDS on the device)
    for (int e = 0; e < fp::ZTAB_ENTRIES; ++e) ztab[e] = fp::ztab_entry(e, C.zf);
    std::vector<u32> wave_lds(BR_WAVE_LDS_WORDS + 2);
    u32* acc_lds = wave_lds.data() + ((reinterpret_cast<uintptr_t>(wave_lds.data()) & 7) ? 1 : 0);
    struct Lane {
        u32 lo[32];
        double x[32], accum[32];
    };
    std::vector<Lane> R(64);
    auto acc_h = [&](int lane) { return acc_lds + (lane >> 5) * NTT_N; };
    auto xb = [&](int lane) { return acc_lds + 2 * NTT_N + (lane >> 5) * XB_WORDS32; };
    auto xb64_own = [&](int lane) { return reinterpret_cast<double*>(xb(lane)); };
    auto xb64_oth = [&](int lane) {
        return reinterpret_cast<const double*>(acc_lds + 2 * NTT_N + (1 - (lane >> 5)) * XB_WORDS32);
    };
#define ALL_LANES for (int lane = 0; lane < 64; ++lane)
    const u32 bbar = br_modswitch_b(lin[p->n]);
    ALL_LANES br_init_acc(lane >> 5, lane & 31, bbar, p->mu, acc_h(lane));
    for (u32 i = 0; i < p->n; ++i) {
        const u32 abar = br_modswitch_a(lin[i]);
        const double* bk_step = bk_ntt + (size_t)i * (2 * L) * 2 * NTT_N;
        ALL_LANES for (int q = 0; q < 32; ++q) R[lane].accum[q] = 0.0;
        for (int pass = 0; pass < 2 * L + 2; ++pass) {
            const int lvl = pass >> 1;
            const bool fwd = pass < 2 * L, first = (pass & 1) == 0;
            ALL_LANES
            {
                Lane& r = R[lane];
                if (first) {
                    if (fwd) fp::fwd1_pre<D>(lane & 31, lvl, abar, acc_h(lane), r.x, ztab.data(), C.zf);
                    else
                        for (int q = 0; q < 32; ++q) r.x[q] = fp::norm(r.accum[q]);
                }
                track(r.x);
                if (first) fp::ntt32_dif<fp::PASS1>(r.x, C.w);
                else fp::ntt32_dif<fp::PASS2>(r.x, C.w);
                track(r.x);
            }
            if (first) {
                ALL_LANES
                {
                    if (fwd) {
                        fp::fwd1_twiddle(lane & 31, R[lane].x, T.twf_t.data());
                        fp::xpose_write<false>(lane & 31, R[lane].x, xb(lane), false);
                    }
                    else {
                        fp::inv1_twiddle(lane & 31, R[lane].x, T.twi_t.data());
                        fp::xpose_write<true>(lane & 31, R[lane].x, xb(lane), false);
                    }
                }
                ALL_LANES br_xpose_read_lo(lane & 31, R[lane].lo, xb(lane));
                ALL_LANES
                {
                    if (fwd) fp::xpose_write<false>(lane & 31, R[lane].x, xb(lane), true);
                    else fp::xpose_write<true>(lane & 31, R[lane].x, xb(lane), true);
                }
                ALL_LANES fp::xpose_read_hi(lane & 31, R[lane].x, R[lane].lo, xb(lane));
            }
            else if (fwd) {
                for (int chunk = 0; chunk < 2; ++chunk) {
                    ALL_LANES fp::share_write(lane & 31, chunk, R[lane].x, xb64_own(lane));
                    ALL_LANES
                    {
                        const int h = lane >> 5, t = lane & 31;
                        const double* bko = bk_step + (size_t)((h * L + lvl) * 2 + h) * NTT_N + (size_t)t * 2;
                        const double* bkt = bk_step + (size_t)(((1 - h) * L + lvl) * 2 + h) * NTT_N + (size_t)t * 2;
                        for (int m = chunk * 8; m < chunk * 8 + 8; ++m) {
                            const double bo[2] = {bko[m * 64], bko[m * 64 + 1]};
                            const double bt[2] = {bkt[m * 64], bkt[m * 64 + 1]};
                            fp::mac_pair(t, m, R[lane].x, xb64_oth(lane), bo, bt, R[lane].accum);
                        }
                        track(R[lane].accum);
                    }
                }
                if (L > 3 && lvl == 1) ALL_LANES for (int q = 0; q < 32; ++q) R[lane].accum[q] = fp::norm(R[lane].accum[q]);
            }
            else {
                ALL_LANES fp::inv2_post(lane & 31, R[lane].x, acc_h(lane), C.zi);
            }
        }
    }
    tlwe1[0] = acc_lds[0];
    for (u32 j = 1; j < (u32)NTT_N; ++j) tlwe1[j] = 0u - acc_lds[NTT_N - j];
    tlwe1[NTT_N] = acc_lds[NTT_N];
#undef ALL_LANES
}

// ---------------------------------------------------------------------------------------------
// Lane-by-lane emulation of kernels.hpp::blind_rotate_fp_lat3_kernel (blind_rotate_lat3.hpp): 8 waves per rotation;
// transform wave w < 2 LV = digit polynomial (w / LV, w % LV) with 16 points per lane, the two v_permlane32_swap
// rounds of every pass modelled on the lane arrays; spectra to per-wave buffers in the key's device layout; the MAC
// split by frequency over all 8 waves (lane = one adjacent pair of the layout); waves 4..7 run the two inverse
// transforms, two waves per polynomial with 8 points per lane.
template <class D>
void blind_rotate_fp_lat3(const iyk_params* p, const u32* lin, const double* bk_ntt, u32* tlwe1)
{
    constexpr int LV = D::LV, XF = 2 * LV, W = 8;
    static_assert(XF <= W, "more digit polynomials than waves");
    const FpTables& T = fptables();
    const fp::NttConsts& C = T.t.c;
    std::vector<double> ztab(fp::ZTAB_ENTRIES);
    for (int e = 0; e < fp::ZTAB_ENTRIES; ++e) ztab[e] = fp::ztab_entry(e, C.zf);
    std::vector<u32> acc(4 * NTT_N);   // [2][2048]: every polynomial followed by its negation (lat3_diff2)
    std::vector<double> sum(2 * NTT_N, 0.0), xb((size_t)XF * 32 * XB_STRIDE);
    struct Lane {
        double x[16], tw0[8], zi16[16];
    };
    std::vector<Lane> R((size_t)W * 64);
    // v_permlane32_swap on registers (a[2m], a[2m+1]) of one wave: upper half of the first <-> lower half of the second
    auto swap16 = [&](int wave) {
        for (int m = 0; m < 8; ++m)
            for (int l = 0; l < 32; ++l) std::swap(R[wave * 64 + 32 + l].x[2 * m], R[wave * 64 + l].x[2 * m + 1]);
    };
    auto track1 = [&](double v) {
        const double a = (v < 0 ? -v : v) / fp::P;
        if (a > g_fp_maxabs) g_fp_maxabs = a;
    };
    auto trackw = [&](int wave) {
        for (int lane = 0; lane < 64; ++lane)
            for (double v : R[wave * 64 + lane].x) track1(v);
    };
#define WAVE_LANES(w) for (int lane = 0; lane < 64; ++lane)
    auto dif16p = [&](int wave, int pass) {
        WAVE_LANES(wave)
        {
            Lane& r = R[wave * 64 + lane];
            if (pass == 1) fp::dif16_stage0<fp::PASS1>(r.x, lane >> 5, r.tw0);
            else fp::dif16_stage0<fp::PASS2>(r.x, lane >> 5, r.tw0);
        }
        trackw(wave);
        swap16(wave);
        WAVE_LANES(wave)
        {
            Lane& r = R[wave * 64 + lane];
            if (pass == 1) fp::dif16_stages14<fp::PASS1>(r.x, C.w);
            else fp::dif16_stages14<fp::PASS2>(r.x, C.w);
        }
        trackw(wave);
    };
    const u32 bbar = br_modswitch_b(lin[p->n]);
    for (int wave = 0; wave < W; ++wave) {
        const int c_inv = wave - (W - 2);
        WAVE_LANES(wave)
        {
            const int half = lane >> 5, t = lane & 31;
            Lane& r = R[wave * 64 + lane];
            for (int m = 0; m < 8; ++m) r.tw0[m] = C.w[2 * m + half];
            for (int q = 0; q < 16; ++q) r.zi16[q] = C.zi[fp::inv16(half, q)];
            if (c_inv >= 0)
                for (int rr = 0; rr < 16; ++rr) {
                    const int j = t + 32 * (16 * half + rr);
                    const u32 idx = ((u32)j - bbar) & (2 * NTT_N - 1);
                    const u32 v0 = c_inv ? ((idx & NTT_N) ? 0u - p->mu : p->mu) : 0u;
                    acc[c_inv * 2 * NTT_N + j] = v0;
                    acc[c_inv * 2 * NTT_N + NTT_N + j] = 0u - v0;
                }
        }
    }
    for (u32 i = 0; i < p->n; ++i) {
        const u32 ab = br_modswitch_a(lin[i]);
        const double* bk_step = bk_ntt + (size_t)i * XF * 2 * NTT_N;
        // forward phase (transform waves), up to barrier 1
        for (int wave = 0; wave < XF; ++wave) {
            const int h = wave / LV, v = wave % LV;
            double* wxb = xb.data() + (size_t)wave * 32 * XB_STRIDE;
            WAVE_LANES(wave)
            {   // digits straight into arrangement P
                u32 tb[16];
                fp::lat3_diff2<D>(lane >> 5, lane & 31, ab, acc.data() + h * 2 * NTT_N, tb);
                fp::t16_digits<D>(lane >> 5, v, tb, R[wave * 64 + lane].x, ztab.data(), C.zf);
            }
            dif16p(wave, 1);
            WAVE_LANES(wave) fp::xpose16_write<false>(lane >> 5, lane & 31, R[wave * 64 + lane].x, wxb);
            WAVE_LANES(wave)
            {   // part B: transposed read, then the inter-pass twiddle of element j1 = 16 half + r of row k2 = t
                const int half = lane >> 5, t = lane & 31;
                for (int e = 0; e < 16; ++e) {
                    const int j1 = fp::t16_pair_elem(half, e);
                    R[wave * 64 + lane].x[e] = fp::mulmod(wxb[t * XB_STRIDE + j1], T.twf_t[t * 32 + j1]);
                }
            }
            dif16p(wave, 2);
            WAVE_LANES(wave)
            {
                const int half = lane >> 5, t = lane & 31;
                for (int q = 0; q < 16; ++q) wxb[fp::brv4(q) * 64 + 2 * t + half] = R[wave * 64 + lane].x[q];
            }
        }
        // MAC phase (all waves), up to barrier 2
        for (int wave = 0; wave < W; ++wave)
            WAVE_LANES(wave)
            {
                const int pair = 2 * (64 * wave + lane);
                double s0[2] = {0, 0}, s1[2] = {0, 0};
                for (int r = 0; r < XF; ++r) {
                    const double* sp = xb.data() + (size_t)r * 32 * XB_STRIDE + pair;
                    const double* b0 = bk_step + (size_t)(r * 2 + 0) * NTT_N + pair;
                    const double* b1 = bk_step + (size_t)(r * 2 + 1) * NTT_N + pair;
                    for (int e = 0; e < 2; ++e) {
                        const double p0 = fp::mulmod(sp[e], b0[e]), p1 = fp::mulmod(sp[e], b1[e]);
                        s0[e] = r ? s0[e] + p0 : p0;
                        s1[e] = r ? s1[e] + p1 : p1;
                        track1(s0[e]);
                        track1(s1[e]);
                    }
                    if (XF > 6 && r == XF / 2 - 1)
                        for (int e = 0; e < 2; ++e) {
                            s0[e] = fp::norm(s0[e]);
                            s1[e] = fp::norm(s1[e]);
                        }
                }
                for (int e = 0; e < 2; ++e) {
                    sum[pair + e] = fp::norm(s0[e]);
                    sum[NTT_N + pair + e] = fp::norm(s1[e]);
                }
            }
        // inverse phase: polynomial c on waves (c, g), g = 0 -> waves 6, 7, g = 1 -> waves 4, 5; 8 points per lane
        struct Lane8 {
            double e[8];
        };
        std::vector<Lane8> E((size_t)W * 64);
        auto swap8 = [&](int wave) {
            for (int m = 0; m < 4; ++m)
                for (int l = 0; l < 32; ++l) std::swap(E[wave * 64 + 32 + l].e[2 * m], E[wave * 64 + l].e[2 * m + 1]);
        };
        auto dif8 = [&](int wave, int g, int pass, const std::vector<std::array<double, 16>>& in) {
            WAVE_LANES(wave)
            {
                const int half = lane >> 5;
                double u[8], vv[8], tw0g[8];
                for (int r = 0; r < 8; ++r) {
                    u[r] = in[lane][r];
                    vv[r] = in[lane][8 + r];
                    tw0g[r] = C.w[8 * half + r];
                }
                if (pass == 1) fp::dif8_stage0<fp::PASS1>(u, vv, g, half, tw0g, E[wave * 64 + lane].e);
                else fp::dif8_stage0<fp::PASS2>(u, vv, g, half, tw0g, E[wave * 64 + lane].e);
                for (double x : E[wave * 64 + lane].e) track1(x);
            }
            swap8(wave);
            WAVE_LANES(wave)
            {
                const int half = lane >> 5;
                double tw1[4];
                for (int m = 0; m < 4; ++m) tw1[m] = C.w[4 * m + 2 * half];
                if (pass == 1) fp::dif8_stage1<fp::PASS1>(E[wave * 64 + lane].e, half, tw1);
                else fp::dif8_stage1<fp::PASS2>(E[wave * 64 + lane].e, half, tw1);
                for (double x : E[wave * 64 + lane].e) track1(x);
            }
            swap8(wave);
            WAVE_LANES(wave)
            {
                if (pass == 1) fp::dif8_stages24<fp::PASS1>(E[wave * 64 + lane].e, C.w);
                else fp::dif8_stages24<fp::PASS2>(E[wave * 64 + lane].e, C.w);
                for (double x : E[wave * 64 + lane].e) track1(x);
            }
        };
        std::vector<std::array<double, 16>> in(64);
        for (int wave = 4; wave < 8; ++wave) {  // pass 1', up to barrier 3
            const int c = wave & 1, g = wave >= 6 ? 0 : 1;
            double* wxb = xb.data() + (size_t)c * 32 * XB_STRIDE;
            const double* sum_c = sum.data() + c * NTT_N;
            WAVE_LANES(wave)
            {
                const int half = lane >> 5, t = lane & 31;
                for (int rr = 0; rr < 8; rr += 2) {
                    const double* su = sum_c + (4 * half + rr / 2) * 64 + 2 * t;
                    const double* sv = su + 8 * 64;
                    in[lane][rr] = su[0];
                    in[lane][rr + 1] = su[1];
                    in[lane][8 + rr] = sv[0];
                    in[lane][8 + rr + 1] = sv[1];
                }
            }
            dif8(wave, g, 1, in);
            WAVE_LANES(wave)
            {
                const int half = lane >> 5, t = lane & 31;
                for (int q = 0; q < 8; ++q) {
                    const int j1 = fp::inv8(g, half, q);
                    wxb[j1 * XB_STRIDE + t] = fp::mulmod(E[wave * 64 + lane].e[q], T.twi_t[j1 * 32 + t]);
                }
            }
        }
        for (int wave = 4; wave < 8; ++wave) {  // pass 2', up to barrier 4
            const int c = wave & 1, g = wave >= 6 ? 0 : 1;
            const double* wxb = xb.data() + (size_t)c * 32 * XB_STRIDE;
            WAVE_LANES(wave)
            {
                const int half = lane >> 5, t = lane & 31;
                for (int rr = 0; rr < 8; ++rr) {
                    in[lane][rr] = wxb[t * XB_STRIDE + 8 * half + rr];
                    in[lane][8 + rr] = wxb[t * XB_STRIDE + 16 + 8 * half + rr];
                }
            }
            dif8(wave, g, 2, in);
            WAVE_LANES(wave)
            {
                const int half = lane >> 5, t = lane & 31;
                for (int q = 0; q < 8; ++q) {
                    const int j2 = fp::inv8(g, half, q);
                    const u32 d = fp::inv2_post16(E[wave * 64 + lane].e[q], C.zi[j2]);
                    acc[c * 2 * NTT_N + t + 32 * j2] += d;
                    acc[c * 2 * NTT_N + NTT_N + t + 32 * j2] -= d;
                }
            }
        }
    }
#undef WAVE_LANES
    tlwe1[0] = acc[0];
    for (u32 j = 1; j < (u32)NTT_N; ++j) tlwe1[j] = 0u - acc[NTT_N - j];
    tlwe1[NTT_N] = acc[2 * NTT_N];
}
// ---------------------------------------------------------------------------------------------
// ---- complex-FFT path (fft512.hpp, blind_rotate_fft.hpp): lane-by-lane run of kernels_fft.hpp -------------------------
#define ALL_LANES for (int lane = 0; lane < 64; ++lane)
const fft::Consts& fft_consts()
{
    static fft::Consts* C = [] {
        auto* c = new fft::Consts();
        fft::make_consts(*c);
        return c;
    }();
    return *C;
}
double g_fft_worst = 0.0;

// kernels_fft.hpp::fft_forward / fft_inverse with one loop over the lanes per hand-off
void fft_forward_wave(fft::cplx (*a)[8], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    ALL_LANES fft::fwd_p1(a[lane], C.u, &C.t1[0][lane]);
    ALL_LANES fft::x1_put_a(lane, a[lane], xb);
    ALL_LANES fft::x1_get_b(lane, a[lane], xb);
    ALL_LANES fft::fwd_p2(a[lane], &C.t2t[0][lane & 7]);
    ALL_LANES fft::x2_put_b(lane, a[lane], xb);
    ALL_LANES fft::x2_get_c(lane, a[lane], xb);
    ALL_LANES fft::fwd_p3(a[lane]);
}
// round 5: the forward transform of the throughput kernel and of the key spectra (three twisted DFT8 passes of Linzer-Feig
// butterflies, kernels_fft.hpp::fft_forward_lf); same arrangements, same exchanges
void fft_forward_lf_wave(fft::cplx (*a)[8], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    ALL_LANES fft::fwd_q1(a[lane], C.lu);
    ALL_LANES fft::x1_put_a(lane, a[lane], xb);
    ALL_LANES fft::x1_get_b(lane, a[lane], xb);
    ALL_LANES fft::fwd_q23(a[lane], &C.lf2[0][lane >> 3], 8);
    ALL_LANES fft::x2_put_b(lane, a[lane], xb);
    ALL_LANES fft::x2_get_c(lane, a[lane], xb);
    ALL_LANES fft::fwd_q23(a[lane], &C.lf3[0][lane], 64);
}
void fft_inverse_wave(fft::cplx (*a)[8], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    ALL_LANES fft::inv_p1(a[lane], &C.t2t[0][lane & 7]);
    ALL_LANES fft::x2_put_c(lane, a[lane], xb);
    ALL_LANES fft::x2_get_b(lane, a[lane], xb);
    ALL_LANES fft::inv_p2(a[lane]);
    ALL_LANES fft::x1_put_b(lane, a[lane], xb);
    ALL_LANES fft::x1_get_a(lane, a[lane], xb);
    ALL_LANES fft::inv_p3(a[lane], C.u, &C.t1[0][lane]);
}

// kernels_fft.hpp::fft_inverse2: the lo and hi halves of one output polynomial through ONE exchange buffer, in the kernel's issue
// order (every hand-off of A before the same hand-off of B), the lane's T2 and T1 columns fetched once and used by both halves
void fft_inverse2_wave(fft::cplx (*a)[8], fft::cplx (*b)[8], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    static thread_local fft::cplx w[64][7], tw[64][8];
    ALL_LANES fft::inv_t2_load(w[lane], &C.t2t[0][lane & 7]);
    ALL_LANES fft::inv_p1(a[lane], w[lane]);
    ALL_LANES fft::x2_put_c(lane, a[lane], xb);
    ALL_LANES fft::x2_get_b(lane, a[lane], xb);
    ALL_LANES fft::inv_p1(b[lane], w[lane]);
    ALL_LANES fft::x2_put_c(lane, b[lane], xb);
    ALL_LANES fft::x2_get_b(lane, b[lane], xb);
    ALL_LANES fft::inv_p2(a[lane]);
    ALL_LANES fft::x1_put_b(lane, a[lane], xb);
    ALL_LANES fft::x1_get_a(lane, a[lane], xb);
    ALL_LANES fft::inv_p2(b[lane]);
    ALL_LANES fft::x1_put_b(lane, b[lane], xb);
    ALL_LANES fft::x1_get_a(lane, b[lane], xb);
    ALL_LANES fft::inv_t1_load(tw[lane], &C.t1[0][lane]);
    ALL_LANES fft::inv_p3(a[lane], C.u, tw[lane]);
    ALL_LANES fft::inv_p3(b[lane], C.u, tw[lane]);
}

template <class G>
void blind_rotate_fft(const iyk_params* p, const u32* lin, const fft::cplx* bk_fft, u32* tlwe1)
{
    constexpr int L = G::L;
    std::vector<u32> acc(2 * NTT_N);
    std::vector<fft::cplx> xbuf(fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cplx* xb = xbuf.data();
    const u32 bbar = br_modswitch_b(lin[p->n]);
    ALL_LANES br_init_acc(lane >> 5, lane & 31, bbar, p->mu, acc.data() + (lane >> 5) * NTT_N);
    static thread_local fft::cplx S[2][2][64][8], a[64][8];
    static thread_local u32 u[64][16], u_b[64][16], lo[64][16];
    for (u32 i = 0; i < p->n; ++i) {
        const u32 ab = br_modswitch_a(lin[i]);
        // as the kernel: the rotated difference of both polynomials once per step, b's moves into u at row L
        ALL_LANES fft::diff16_pair<G>(lane, ab, acc.data(), u[lane], u_b[lane]);
        for (int r = 0; r < 2 * L; ++r) {
            const int c = r >= L ? 1 : 0, lvl = r - c * L;
            if (r == L) ALL_LANES std::memcpy(u[lane], u_b[lane], sizeof u[lane]);
            ALL_LANES fft::digits8<G>(lvl, u[lane], a[lane]);
            fft_forward_lf_wave(a, xb);
            const u32 row_off = (i * (u32)(2 * L) + (u32)r) * 4u * (u32)fft::M;
            ALL_LANES
            {
                const fft::Keys keys(bk_fft, 0, lane);
                for (int q = 0; q < 8; ++q)
                    for (int pc = 0; pc < 4; ++pc) {
                        if (r == 0) fft::cmac<true>(S[pc >> 1][pc & 1][lane][q], a[lane][q], keys.at(row_off, pc, q));
                        else fft::cmac<false>(S[pc >> 1][pc & 1][lane][q], a[lane][q], keys.at(row_off, pc, q));
                    }
            }
        }
        for (int cc = 0; cc < 2; ++cc) {
            fft_inverse2_wave(S[cc][0], S[cc][1], xb);
            ALL_LANES
            {
                const double e0 = fft::round_err8(S[cc][0][lane]), e1 = fft::round_err8(S[cc][1][lane]);
                g_fft_worst = std::max(g_fft_worst, std::max(e0, e1));
                fft::round16(S[cc][0][lane], lo[lane]);
            }
            ALL_LANES fft::acc_update16(lane, S[cc][1][lane], lo[lane], acc.data() + cc * NTT_N);
        }
    }
    tlwe1[0] = acc[0];
    for (u32 j = 1; j < (u32)NTT_N; ++j) tlwe1[j] = 0u - acc[NTT_N - j];
    tlwe1[NTT_N] = acc[NTT_N];
}

// lane-by-lane run of cmux_fft.hpp::cmux_fft_kernel for one job, in place on the TRLWE rows T (same phase functions, same order)
template <class G>
void cmux_fft(const CmuxJob& j, const fft::cplx* trgsw, u32* T)
{
    constexpr int L = G::L;
    std::vector<u32> acc(2 * NTT_N);
    std::vector<fft::cplx> xbuf(fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cplx* xb = xbuf.data();
    const fft::cplx* slot = trgsw + (size_t)j.sel * fft::trgsw_slot_cplx<G>();
    static thread_local fft::cplx S[2][2][64][8], a[64][8];
    static thread_local u32 u[64][16], lo[64][16];
    ALL_LANES fft::cmux_load_acc(lane, T + (size_t)j.in0 * (2 * NTT_N), acc.data());
    ALL_LANES for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][lane][e & 7] = {0.0, 0.0};
    for (int r = 0; r < 2 * L; ++r) {
        const int c = r >= L ? 1 : 0, lvl = r - c * L;
        if (lvl == 0) {
            if (j.in1 >= 0) ALL_LANES fft::cmux_diff16<G>(lane, T + (size_t)j.in1 * (2 * NTT_N) + c * NTT_N, acc.data() + c * NTT_N, u[lane]);
            else ALL_LANES fft::diff16<G>(lane, (u32)j.rot, acc.data() + c * NTT_N, u[lane]);
        }
        ALL_LANES fft::digits8<G>(lvl, u[lane], a[lane]);
        fft_forward_lf_wave(a, xb);
        const u32 row_off = (u32)r * 4u * (u32)fft::M;
        ALL_LANES
        {
            const fft::Keys keys(slot, 0, lane);
            for (int q = 0; q < 8; ++q)
                for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][lane][q], a[lane][q], keys.at(row_off, pc, q));
        }
    }
    for (int cc = 0; cc < 2; ++cc) {
        fft_inverse2_wave(S[cc][0], S[cc][1], xb);
        ALL_LANES
        {
            const double e0 = fft::round_err8(S[cc][0][lane]), e1 = fft::round_err8(S[cc][1][lane]);
            g_fft_worst = std::max(g_fft_worst, std::max(e0, e1));
            fft::round16(S[cc][0][lane], lo[lane]);
        }
        ALL_LANES fft::acc_update16(lane, S[cc][1][lane], lo[lane], acc.data() + cc * NTT_N);
    }
    ALL_LANES fft::cmux_store_acc(lane, acc.data(), T + (size_t)j.out * (2 * NTT_N));
}

// lane-by-lane run of cmux_fft.hpp::cmux_chain_kernel for one job, in place on the TRLWE rows T (same phase functions, same order)
template <class G>
void cmux_chain(const CmuxChainJob& j, const fft::cplx* trgsw, u32* T)
{
    constexpr int L = G::L;
    std::vector<u32> acc(2 * NTT_N);
    std::vector<fft::cplx> xbuf(fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cplx* xb = xbuf.data();
    const u32* mem_row = T + (size_t)j.mem * (2 * NTT_N);
    static thread_local fft::cplx S[2][2][64][8], a[64][8];
    static thread_local u32 u[64][16], lo[64][16];
    ALL_LANES fft::cmux_load_acc(lane, T + (size_t)j.src * (2 * NTT_N), acc.data());
    for (int s = 0; s < j.steps; ++s) {
        const bool rev = (j.pattern >> s) & 1u;
        const fft::cplx* slot = trgsw + (size_t)(j.sel0 + s) * fft::trgsw_slot_cplx<G>();
        ALL_LANES for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][lane][e & 7] = {0.0, 0.0};
        for (int r = 0; r < 2 * L; ++r) {
            const int c = r >= L ? 1 : 0, lvl = r - c * L;
            if (lvl == 0) {
                if (rev) ALL_LANES fft::cmux_diff16_rev<G>(lane, mem_row + c * NTT_N, acc.data() + c * NTT_N, u[lane]);
                else ALL_LANES fft::cmux_diff16<G>(lane, mem_row + c * NTT_N, acc.data() + c * NTT_N, u[lane]);
            }
            ALL_LANES fft::digits8<G>(lvl, u[lane], a[lane]);
            fft_forward_lf_wave(a, xb);
            const u32 row_off = (u32)r * 4u * (u32)fft::M;
            ALL_LANES
            {
                const fft::Keys keys(slot, 0, lane);
                for (int q = 0; q < 8; ++q)
                    for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][lane][q], a[lane][q], keys.at(row_off, pc, q));
            }
        }
        for (int cc = 0; cc < 2; ++cc) {
            fft_inverse2_wave(S[cc][0], S[cc][1], xb);
            ALL_LANES
            {
                const double e0 = fft::round_err8(S[cc][0][lane]), e1 = fft::round_err8(S[cc][1][lane]);
                g_fft_worst = std::max(g_fft_worst, std::max(e0, e1));
                fft::round16(S[cc][0][lane], lo[lane]);
            }
            if (rev) ALL_LANES fft::cmux_acc_replace16(lane, mem_row + cc * NTT_N, S[cc][1][lane], lo[lane], acc.data() + cc * NTT_N);
            else ALL_LANES fft::acc_update16(lane, S[cc][1][lane], lo[lane], acc.data() + cc * NTT_N);
        }
    }
    ALL_LANES fft::cmux_store_acc(lane, acc.data(), T + (size_t)j.out * (2 * NTT_N));
}

// lane-by-lane run of cmux_fft.hpp::cmux_rotate_chain_kernel for one job, in place on the TRLWE rows T (same phase functions, same order)
template <class G>
void cmux_rotate_chain(const CmuxRotChainJob& j, const CmuxRotStep* list, const fft::cplx* trgsw, u32* T)
{
    constexpr int L = G::L;
    std::vector<u32> acc(2 * NTT_N);
    std::vector<fft::cplx> xbuf(fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cplx* xb = xbuf.data();
    static thread_local fft::cplx S[2][2][64][8], a[64][8];
    static thread_local u32 u[64][16], lo[64][16];
    ALL_LANES fft::cmux_load_acc(lane, T + (size_t)j.src * (2 * NTT_N), acc.data());
    for (int s = 0; s < j.steps; ++s) {
        const CmuxRotStep& step = list[j.first + s];
        const fft::cplx* slot = trgsw + (size_t)step.sel * fft::trgsw_slot_cplx<G>();
        ALL_LANES for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][lane][e & 7] = {0.0, 0.0};
        for (int r = 0; r < 2 * L; ++r) {
            const int c = r >= L ? 1 : 0, lvl = r - c * L;
            if (lvl == 0) ALL_LANES fft::diff16<G>(lane, (u32)step.rot, acc.data() + c * NTT_N, u[lane]);
            ALL_LANES fft::digits8<G>(lvl, u[lane], a[lane]);
            fft_forward_lf_wave(a, xb);
            const u32 row_off = (u32)r * 4u * (u32)fft::M;
            ALL_LANES
            {
                const fft::Keys keys(slot, 0, lane);
                for (int q = 0; q < 8; ++q)
                    for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][lane][q], a[lane][q], keys.at(row_off, pc, q));
            }
        }
        for (int cc = 0; cc < 2; ++cc) {
            fft_inverse2_wave(S[cc][0], S[cc][1], xb);
            ALL_LANES
            {
                const double e0 = fft::round_err8(S[cc][0][lane]), e1 = fft::round_err8(S[cc][1][lane]);
                g_fft_worst = std::max(g_fft_worst, std::max(e0, e1));
                fft::round16(S[cc][0][lane], lo[lane]);
            }
            ALL_LANES fft::acc_update16(lane, S[cc][1][lane], lo[lane], acc.data() + cc * NTT_N);
        }
    }
    ALL_LANES fft::cmux_store_acc(lane, acc.data(), T + (size_t)j.out * (2 * NTT_N));
}

// lane-by-lane run of cmux_fft.hpp::cmux_tree_kernel for one job, in place on the TRLWE rows T (same phase functions, same order): the
// workgroup's accumulators s_acc[ROT_WAVES][2][N] as the kernel keeps them, level by level — what the barrier between two levels orders
// — and inside a level wave by wave: an active wave writes its own accumulator and reads one that no wave of the level writes.
template <class G>
void cmux_tree(const CmuxTreeJob& j, const fft::cplx* trgsw, u32* T)
{
    constexpr int L = G::L;
    std::vector<u32> s_acc((size_t)dispatch::ROT_WAVES * 2 * NTT_N);
    std::vector<fft::cplx> xbuf(fft::XCHG_BYTES / sizeof(fft::cplx));
    fft::cplx* xb = xbuf.data();
    static thread_local fft::cplx S[2][2][64][8], a[64][8];
    static thread_local u32 u[64][16], lo[64][16];
    const int members = 1 << (j.levels - 1);
    for (int w = 0; w < members; ++w) ALL_LANES fft::cmux_load_acc(lane, T + (size_t)(j.first + 2 * w) * (2 * NTT_N), s_acc.data() + (size_t)w * 2 * NTT_N);
    for (int b = 0; b < j.levels; ++b) {
        for (int w = 0; w < members; ++w) {
            if (w & ((1 << b) - 1)) continue;
            u32* acc = s_acc.data() + (size_t)w * 2 * NTT_N;
            const u32* in1 = b == 0 ? T + (size_t)(j.first + 2 * w + 1) * (2 * NTT_N) : s_acc.data() + (size_t)(w + ((1 << b) >> 1)) * 2 * NTT_N;
            const fft::cplx* slot = trgsw + (size_t)(j.sel0 + b) * fft::trgsw_slot_cplx<G>();
            ALL_LANES for (int e = 0; e < 32; ++e) S[e >> 4][(e >> 3) & 1][lane][e & 7] = {0.0, 0.0};
            for (int r = 0; r < 2 * L; ++r) {
                const int c = r >= L ? 1 : 0, lvl = r - c * L;
                if (lvl == 0) ALL_LANES fft::cmux_diff16<G>(lane, in1 + c * NTT_N, acc + c * NTT_N, u[lane]);
                ALL_LANES fft::digits8<G>(lvl, u[lane], a[lane]);
                fft_forward_lf_wave(a, xb);
                const u32 row_off = (u32)r * 4u * (u32)fft::M;
                ALL_LANES
                {
                    const fft::Keys keys(slot, 0, lane);
                    for (int q = 0; q < 8; ++q)
                        for (int pc = 0; pc < 4; ++pc) fft::cmac<false>(S[pc >> 1][pc & 1][lane][q], a[lane][q], keys.at(row_off, pc, q));
                }
            }
            for (int cc = 0; cc < 2; ++cc) {
                fft_inverse2_wave(S[cc][0], S[cc][1], xb);
                ALL_LANES
                {
                    const double e0 = fft::round_err8(S[cc][0][lane]), e1 = fft::round_err8(S[cc][1][lane]);
                    g_fft_worst = std::max(g_fft_worst, std::max(e0, e1));
                    fft::round16(S[cc][0][lane], lo[lane]);
                }
                ALL_LANES fft::acc_update16(lane, S[cc][1][lane], lo[lane], acc + cc * NTT_N);
            }
        }
    }
    ALL_LANES fft::cmux_store_acc(lane, s_acc.data(), T + (size_t)j.out * (2 * NTT_N));
}

// one inverse transform of one wave (kernels_fft.hpp::fft_inverse1)
void fft_inverse1_wave(fft::cplx (*a)[8], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    ALL_LANES fft::inv_p1(a[lane], &C.t2t[0][lane & 7]);
    ALL_LANES fft::x2_put_c(lane, a[lane], xb);
    ALL_LANES fft::x2_get_b(lane, a[lane], xb);
    ALL_LANES fft::inv_p2(a[lane]);
    ALL_LANES fft::x1_put_b(lane, a[lane], xb);
    ALL_LANES fft::x1_get_a(lane, a[lane], xb);
    ALL_LANES fft::inv_p3(a[lane], C.u, &C.t1[0][lane]);
}

const fft::Consts256& fft_consts256()
{
    static fft::Consts256* C = [] {
        auto* c = new fft::Consts256();
        fft::make_consts256(*c);
        return c;
    }();
    return *C;
}
// kernels_fft.hpp::hfft_forward / hfft_inverse (half transforms of fft256.hpp), one loop over the lanes per hand-off
template <int P>
void hfft_forward_wave(fft::cplx (*x)[4], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    const fft::Consts256& H = fft_consts256();
    ALL_LANES fft::hfwd_p1(x[lane], C.u, &H.fwd[P][0][lane]);
    ALL_LANES fft::xtop_put_other(lane, x[lane], xb);
    ALL_LANES fft::xtop_get_own(lane, x[lane], xb);
    ALL_LANES fft::hfwd_p2(x[lane], &H.fwd[P][0][lane]);
    ALL_LANES fft::xmid_put_other(lane, x[lane], xb);
    ALL_LANES fft::xmid_get_own(lane, x[lane], xb);
    ALL_LANES fft::hfwd_p3<P>(x[lane], &H.fwd[P][0][lane]);
    ALL_LANES fft::xlow_put_other(lane, x[lane], xb);
    ALL_LANES fft::xlow_get_own(lane, x[lane], xb);
    ALL_LANES fft::hfwd_p4<P>(x[lane]);
}
// c[lane][q] = C[r(lane) + 64 q] on entry (lane = (r0, r1, r2)); y[lane][n0] = z[2 lane + P + 128 n0] on exit
template <int P>
void hfft_inverse_wave(const fft::cplx (*c)[8], fft::cplx (*y)[4], fft::cplx* xb)
{
    const fft::Consts& C = fft_consts();
    const fft::Consts256& H = fft_consts256();
    ALL_LANES fft::hinv_pA<P>(c[lane], y[lane], &H.inv[P][0][lane]);
    ALL_LANES fft::xlow_put_own(lane, y[lane], xb);
    ALL_LANES fft::xlow_get_other(lane, y[lane], xb);
    ALL_LANES fft::hinv_pB(y[lane], &H.inv[P][0][lane]);
    ALL_LANES fft::xmid_put_own(lane, y[lane], xb);
    ALL_LANES fft::xmid_get_other(lane, y[lane], xb);
    ALL_LANES fft::hinv_pC(y[lane], &H.inv[P][0][lane]);
    ALL_LANES fft::xtop_put_own(lane, y[lane], xb);
    ALL_LANES fft::xtop_get_other(lane, y[lane], xb);
    ALL_LANES fft::hinv_pD(y[lane], C.u);
}

// wave-by-wave, lane-by-lane run of kernels_fft.hpp::blind_rotate_fft_lat_kernel: one rotation on 8 waves, doubled accumulator,
// spectra and sums through "LDS" arrays in the kernel's layouts, the three phases in the order the barriers impose; rows
// NFULL .. 2L-1 forward and every inverse in the halves of fft256.hpp, with the kernel's wave roles
template <class G>
void blind_rotate_fft_lat(const iyk_params* p, const u32* lin, const fft::cplx* bk_fft, u32* tlwe1)
{
    constexpr int L = G::L, XF = 2 * L, NFULL = XF == 6 ? 4 : 0;
    constexpr size_t XB = fft::XCHG_BYTES / sizeof(fft::cplx), HB = fft::XCHG256_BYTES / sizeof(fft::cplx);
    auto half_buf = [](int row, int par) { return NFULL ? 2 * (row - NFULL) + par : row + 4 * par; };
    std::vector<u32> acc2(4 * NTT_N);
    std::vector<fft::cplx> s_xb(NFULL * XB + (8 - NFULL) * HB), s_sum(4 * fft::M);
    fft::cplx* s_hb = s_xb.data() + NFULL * XB;
    const u32 bbar = br_modswitch_b(lin[p->n]);
    for (int e = 0; e < 2 * NTT_N; ++e) {
        const int c = e >> 10, j = e & (NTT_N - 1);
        const u32 idx = ((u32)j - bbar) & (2 * NTT_N - 1);
        const u32 v = c ? ((idx & NTT_N) ? 0u - p->mu : p->mu) : 0u;
        acc2[c * 2 * NTT_N + j] = v;
        acc2[c * 2 * NTT_N + NTT_N + j] = 0u - v;
    }
    static thread_local fft::cplx a[64][8], x[64][4];
    static thread_local u32 u[64][16], u8[64][8];
    for (u32 i = 0; i < p->n; ++i) {
        const u32 ab = br_modswitch_a(lin[i]);
        for (int wave = 0; wave < 8; ++wave) {   // forward
            const bool full = wave < NFULL;
            const int fr = full ? wave : (NFULL ? NFULL + ((wave - NFULL) >> 1) : (wave & 3));
            const int fp = full ? 0 : (NFULL ? ((wave - NFULL) & 1) : (wave >> 2));
            const int cF = fr / L, lvl = fr - cF * L;
            fft::cplx* xbf = full ? s_xb.data() + (size_t)wave * XB : s_hb + (size_t)(wave - NFULL) * HB;
            if (full) {
                ALL_LANES fft::diff16_doubled<G>(lane, ab, acc2.data() + cF * 2 * NTT_N, u[lane]);
                ALL_LANES fft::digits8<G>(lvl, u[lane], a[lane]);
                fft_forward_wave(a, xbf);
                ALL_LANES for (int q = 0; q < 8; ++q) xbf[q * 64 + lane] = a[lane][q];
            }
            else {
                ALL_LANES fft::diff8_doubled<G>(lane, fp, ab, acc2.data() + cF * 2 * NTT_N, u8[lane]);
                ALL_LANES fft::digits4<G>(lvl, u8[lane], x[lane]);
                if (fp) hfft_forward_wave<1>(x, xbf);
                else hfft_forward_wave<0>(x, xbf);
                ALL_LANES for (int q = 0; q < 4; ++q) xbf[q * 64 + fft::h_in_pos(lane)] = x[lane][q];
            }
        }
        for (int wave = 0; wave < 8; ++wave)      // MAC: frequency block q = wave
            ALL_LANES
            {
                const fft::Keys keys(bk_fft, 0, lane);
                fft::cplx sacc[4];
                for (int r = 0; r < XF; ++r) {
                    fft::cplx d;
                    if (r < NFULL) d = s_xb[(size_t)r * XB + wave * 64 + lane];
                    else {
                        const fft::cplx e = s_hb[(size_t)half_buf(r, 0) * HB + (wave & 3) * 64 + lane];
                        const fft::cplx o = s_hb[(size_t)half_buf(r, 1) * HB + (wave & 3) * 64 + lane];
                        const double sg = wave < 4 ? 1.0 : -1.0;
                        d = {fft::fma_(sg, o.re, e.re), fft::fma_(sg, o.im, e.im)};
                    }
                    for (int pc = 0; pc < 4; ++pc) {
                        const fft::cplx k = keys.at((i * (u32)XF + (u32)r) * 4u * (u32)fft::M, pc, 0, (u32)wave * 1024u);
                        if (r == 0) fft::cmac<true>(sacc[pc], d, k);
                        else fft::cmac<false>(sacc[pc], d, k);
                    }
                }
                for (int pc = 0; pc < 4; ++pc) s_sum[pc * fft::M + wave * 64 + lane] = sacc[pc];
            }
        for (int wave = 0; wave < 8; ++wave) {    // inverse: output parity wave >> 2 of sum (c', half) = ((wave & 3) >> 1, wave & 1)
            const int si = wave & 3, ip = wave >> 2;
            fft::cplx* xbi = wave < NFULL ? s_xb.data() + (size_t)wave * XB : s_hb + (size_t)(wave - NFULL) * HB;
            ALL_LANES for (int q = 0; q < 8; ++q) a[lane][q] = s_sum[si * fft::M + q * 64 + fft::h_in_pos(lane)];
            if (ip) hfft_inverse_wave<1>(a, x, xbi);
            else hfft_inverse_wave<0>(a, x, xbi);
            ALL_LANES
            {
                const double e = fft::round_err4(x[lane]);
                if (e > g_fft_worst) g_fft_worst = e;
                fft::acc_update8_doubled(lane, ip, x[lane], (si & 1) ? 16 : 0, acc2.data() + (si >> 1) * 2 * NTT_N);
            }
        }
    }
    tlwe1[0] = acc2[0];
    for (u32 j = 1; j < (u32)NTT_N; ++j) tlwe1[j] = acc2[NTT_N + (NTT_N - j)];
    tlwe1[NTT_N] = acc2[2 * NTT_N];
}

// iyk_emul_diff16_pair: the three forms of a step's rotated differences, all 64 lanes, out [2][64][16]
template <class G>
int diff16_pair_forms(u32 abar, const u32* acc, int form, u32* out)
{
    u32(*ua)[16] = reinterpret_cast<u32(*)[16]>(out);
    u32(*ub)[16] = reinterpret_cast<u32(*)[16]>(out + 64 * 16);
    ALL_LANES
    {
        if (form == 0) {
            fft::diff16<G>(lane, abar, acc, ua[lane]);
            fft::diff16<G>(lane, abar, acc + NTT_N, ub[lane]);
        }
        else if (form == 1) fft::diff16_pair<G>(lane, abar, acc, ua[lane], ub[lane]);
        else if (form == 2) fft::diff16_pair_device_order<G>(lane, abar, acc, ua[lane], ub[lane]);
        else return -1;
    }
    return 0;
}
}  // namespace

static int g_direct = 0;  // 80-bit set: Decomp<2, 10, 1> (IYK_HIP_DECOMP=direct on the device) instead of the split digits

extern "C" {

void iyk_emul_set_direct(int on) { g_direct = on; }

// FP64 path: NTT of every (virtual) BK row polynomial, device layout, balanced doubles.
// Output size: n * 2*LV * 2 * N doubles, LV = l (128-bit set; 80-bit set, direct) or 2l (80-bit set, split digits).
int iyk_emul_bk_ntt_fp(const iyk_params* p, const uint32_t* bk, double* bk_ntt)
{
    const int split = (p->l == 2 && p->Bgbit == 10 && !g_direct) ? 2 : 1;
    const int L = (int)p->l, LV = L * split, hb = (int)p->Bgbit / 2;
    const size_t vpolys = (size_t)p->n * 2 * LV * 2;
    std::vector<double> in(NTT_N);
    for (size_t q = 0; q < vpolys; ++q) {
        const size_t cc = q & 1, rv = (q >> 1) % (size_t)(2 * LV), i = (q >> 1) / (size_t)(2 * LV);
        const int c = (int)(rv / LV), v = (int)(rv % LV);
        const size_t src = ((i * (size_t)(2 * L) + (size_t)(c * L + v / split)) * 2 + cc) * NTT_N;
        const u32 scale = (split == 2 && (v % split) == 0) ? (1u << hb) : 1u;
        for (int x = 0; x < NTT_N; ++x) in[x] = (double)(int32_t)(bk[src + x] * scale);
        forward_1024_fp_dev(in.data(), bk_ntt + q * NTT_N);
    }
    return 0;
}

int iyk_emul_blind_rotate_fp(const iyk_params* p, const uint32_t* lin, const double* bk_ntt, uint32_t* tlwe1)
{
    if (p->N != 1024 || p->k != 1) return -1;
    if (p->l == 3 && p->Bgbit == 6) blind_rotate_fp<fp::Decomp<3, 6, 1>>(p, lin, bk_ntt, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10 && g_direct) blind_rotate_fp<fp::Decomp<2, 10, 1>>(p, lin, bk_ntt, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10) blind_rotate_fp<fp::Decomp<2, 10, 2>>(p, lin, bk_ntt, tlwe1);
    else return -1;
    return 0;
}

int iyk_emul_blind_rotate_fp_lat3(const iyk_params* p, const uint32_t* lin, const double* bk_ntt, uint32_t* tlwe1)
{
    if (p->N != 1024 || p->k != 1) return -1;
    if (p->l == 3 && p->Bgbit == 6) blind_rotate_fp_lat3<fp::Decomp<3, 6, 1>>(p, lin, bk_ntt, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10 && g_direct) blind_rotate_fp_lat3<fp::Decomp<2, 10, 1>>(p, lin, bk_ntt, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10) blind_rotate_fp_lat3<fp::Decomp<2, 10, 2>>(p, lin, bk_ntt, tlwe1);
    else return -1;
    return 0;
}

double iyk_emul_fp_max_magnitude(void) { return g_fp_maxabs; }

// complex-FFT path: spectra of the signed 16-bit halves of every BK polynomial, cplx [polys][2][512] in arrangement F,
// scaled by 1/512 (kernels_fft.hpp::bk_fft_kernel).  Output: 2 * bk_words doubles.
int iyk_emul_bk_fft(const iyk_params* p, const uint32_t* bk, double* bk_fft)
{
    const size_t polys = (size_t)iyk_bk_words(p) / p->N;
    fft::cplx* out = reinterpret_cast<fft::cplx*>(bk_fft);
    std::vector<fft::cplx> xbuf(fft::XCHG_BYTES / sizeof(fft::cplx));
    static thread_local fft::cplx a[64][8];
    for (size_t q = 0; q < 2 * polys; ++q) {
        const size_t poly = q >> 1;
        const int half = (int)(q & 1);
        ALL_LANES for (int m = 0; m < 8; ++m)
        {
            const u32 kr = bk[poly * NTT_N + lane + 64 * m], ki = bk[poly * NTT_N + lane + 64 * m + 512];
            a[lane][m] = {(double)(half ? fft::key_hi(kr) : fft::key_lo(kr)), (double)(half ? fft::key_hi(ki) : fft::key_lo(ki))};
        }
        fft_forward_lf_wave(a, xbuf.data());
        ALL_LANES for (int k2 = 0; k2 < 8; ++k2)
            out[q * fft::M + (size_t)k2 * 64 + lane] = {a[lane][k2].re * (1.0 / 512.0), a[lane][k2].im * (1.0 / 512.0)};
    }
    return 0;
}
int iyk_emul_blind_rotate_fft(const iyk_params* p, const uint32_t* lin, const double* bk_fft, uint32_t* tlwe1)
{
    if (p->N != 1024 || p->k != 1) return -1;
    const fft::cplx* k = reinterpret_cast<const fft::cplx*>(bk_fft);
    if (p->l == 3 && p->Bgbit == 6) blind_rotate_fft<fft::Gadget<3, 6>>(p, lin, k, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10) blind_rotate_fft<fft::Gadget<2, 10>>(p, lin, k, tlwe1);
    else return -1;
    return 0;
}
int iyk_emul_blind_rotate_fft_lat(const iyk_params* p, const uint32_t* lin, const double* bk_fft, uint32_t* tlwe1)
{
    if (p->N != 1024 || p->k != 1) return -1;
    const fft::cplx* k = reinterpret_cast<const fft::cplx*>(bk_fft);
    if (p->l == 3 && p->Bgbit == 6) blind_rotate_fft_lat<fft::Gadget<3, 6>>(p, lin, k, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10) blind_rotate_fft_lat<fft::Gadget<2, 10>>(p, lin, k, tlwe1);
    else return -1;
    return 0;
}
/* cmux_fft.hpp: the jobs {sel, in0, in1, rot, out} one after the other, in place on `rows` TRLWE rows of 2N words.  set: 0 = the 128-bit
 * set's Gadget<3, 6>, 1 = the 80-bit set's Gadget<2, 10>; trgsw_fft: `sels` selector slots in the device layout (iyk_emul_bk_fft of
 * one TRGSW per slot).  -1: unknown set or an index outside its store. */
int emu_cmux_fft(int set, uint32_t* trlwe, uint64_t rows, const double* trgsw_fft, uint64_t sels, const int32_t* jobs, uint64_t count)
{
    if (set != 0 && set != 1) return -1;
    const fft::cplx* k = reinterpret_cast<const fft::cplx*>(trgsw_fft);
    for (uint64_t g = 0; g < count; ++g) {
        const CmuxJob j{jobs[5 * g], jobs[5 * g + 1], jobs[5 * g + 2], jobs[5 * g + 3], jobs[5 * g + 4]};
        auto row_ok = [&](int32_t r) { return r >= 0 && (uint64_t)r < rows; };
        if (j.sel < 0 || (uint64_t)j.sel >= sels || !row_ok(j.in0) || !row_ok(j.out) || (j.in1 >= 0 && !row_ok(j.in1))) return -1;
        if (j.in1 < 0 && (j.rot < 0 || j.rot >= 2 * NTT_N)) return -1;
        if (set == 0) cmux_fft<fft::Gadget<3, 6>>(j, k, trlwe);
        else cmux_fft<fft::Gadget<2, 10>>(j, k, trlwe);
    }
    return 0;
}
/* cmux_fft.hpp::cmux_chain_kernel: the chain jobs {sel0, steps, pattern, src, mem, out} (six 32-bit words each, the pattern's bits in the
 * third) one after the other, in place on `rows` TRLWE rows.  set and trgsw_fft as for emu_cmux_fft.  -1: unknown set, steps outside
 * [1, 32], or an index outside its store. */
int emu_cmux_chain(int set, uint32_t* trlwe, uint64_t rows, const double* trgsw_fft, uint64_t sels, const int32_t* jobs6, uint64_t count)
{
    if (set != 0 && set != 1) return -1;
    const fft::cplx* k = reinterpret_cast<const fft::cplx*>(trgsw_fft);
    for (uint64_t g = 0; g < count; ++g) {
        const int32_t* w = jobs6 + 6 * g;
        const CmuxChainJob j{w[0], w[1], (uint32_t)w[2], w[3], w[4], w[5]};
        auto row_ok = [&](int32_t r) { return r >= 0 && (uint64_t)r < rows; };
        if (j.steps < 1 || j.steps > CMUX_CHAIN_MAX_STEPS || j.sel0 < 0 || (uint64_t)j.sel0 + (uint64_t)j.steps > sels) return -1;
        if (!row_ok(j.src) || !row_ok(j.mem) || !row_ok(j.out)) return -1;
        if (set == 0) cmux_chain<fft::Gadget<3, 6>>(j, k, trlwe);
        else cmux_chain<fft::Gadget<2, 10>>(j, k, trlwe);
    }
    return 0;
}
/* cmux_fft.hpp::cmux_rotate_chain_kernel: ONE job — acc = T[src]; `steps` rotate-form CMUXes with the pairs (sel[j], rot[j]); T[out] = acc
 * — in place on `rows` TRLWE rows.  set and trgsw_fft as for emu_cmux_fft; the rounding distances feed iyk_emul_fft_round_error like the
 * chain's.  -1: unknown set, steps outside [1, 32], a rot outside [0, 2N) or an index outside its store (nothing is written). */
int iyk_emul_cmux_rotate_chain(int set, uint32_t* trlwe, uint64_t rows, const double* trgsw_fft, uint64_t sels, int32_t steps, const int32_t* sel,
                               const int32_t* rot, int32_t src, int32_t out)
{
    if (set != 0 && set != 1) return -1;
    if (steps < 1 || steps > CMUX_ROT_CHAIN_MAX_STEPS) return -1;
    if (src < 0 || (uint64_t)src >= rows || out < 0 || (uint64_t)out >= rows) return -1;
    std::vector<CmuxRotStep> list((size_t)steps);
    for (int32_t j = 0; j < steps; ++j) {
        if (sel[j] < 0 || (uint64_t)sel[j] >= sels || rot[j] < 0 || rot[j] >= 2 * NTT_N) return -1;
        list[(size_t)j] = CmuxRotStep{sel[j], rot[j]};
    }
    const CmuxRotChainJob j{0, steps, src, out};
    const fft::cplx* k = reinterpret_cast<const fft::cplx*>(trgsw_fft);
    if (set == 0) cmux_rotate_chain<fft::Gadget<3, 6>>(j, list.data(), k, trlwe);
    else cmux_rotate_chain<fft::Gadget<2, 10>>(j, list.data(), k, trlwe);
    return 0;
}
/* cmux_fft.hpp::cmux_tree_kernel: ONE job — the 2^levels leaves T[first ..] halved `levels` times with selector slots sel0 .. sel0 +
 * levels - 1, T[out] = the row left — in place on `rows` TRLWE rows.  set and trgsw_fft as for emu_cmux_fft; the rounding distances feed
 * iyk_emul_fft_round_error like the chains'.  -1: unknown set, levels outside [1, 4] or an index outside its store (nothing is written). */
int iyk_emul_cmux_tree(int set, uint32_t* trlwe, uint64_t rows, const double* trgsw_fft, uint64_t sels, int32_t sel0, int32_t levels,
                       int32_t first, int32_t out)
{
    if (set != 0 && set != 1) return -1;
    if (levels < 1 || levels > CMUX_TREE_MAX_LEVELS) return -1;
    if (sel0 < 0 || (uint64_t)sel0 + (uint64_t)levels > sels) return -1;
    if (first < 0 || (uint64_t)first + (1ull << levels) > rows || out < 0 || (uint64_t)out >= rows) return -1;
    const CmuxTreeJob j{sel0, levels, first, out};
    const fft::cplx* k = reinterpret_cast<const fft::cplx*>(trgsw_fft);
    if (set == 0) cmux_tree<fft::Gadget<3, 6>>(j, k, trlwe);
    else cmux_tree<fft::Gadget<2, 10>>(j, k, trlwe);
    return 0;
}
/* kernels.hpp::sample_extract_index_kernel for one TRLWE: N + 1 words of the TLWE lvl1 at coefficient index h < N */
int emu_sample_extract_index(const uint32_t* trlwe, int h, uint32_t* tlwe1)
{
    if (h < 0 || h >= NTT_N) return -1;
    for (int j = 0; j <= NTT_N; ++j) tlwe1[j] = sample_extract_index_word(trlwe, h, j);
    return 0;
}
/* The half transforms of fft256.hpp against the full ones of fft512.hpp on the same random input: forward — F_0 +- W^k' F_1
 * against the [k2][lane''] spectrum; inverse — both parities against the full inverse's arrangement-A output.  Returns the
 * largest absolute difference relative to the largest magnitude (both networks are exact up to rounding: ~1e-15). */
double iyk_emul_fft256_selftest(unsigned seed)
{
    static thread_local fft::cplx a[64][8], b[64][8], x[2][64][4], y[64][4];
    std::vector<fft::cplx> xb(fft::XCHG_BYTES / sizeof(fft::cplx)), spec(fft::M), half(2 * fft::H);
    u64 st = 0x9E3779B97F4A7C15ull ^ seed;
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(int32_t)(st >> 40) / 256.0 - 32768.0;   // integers in [-2^15, 2^15)
    };
    std::vector<fft::cplx> z(fft::M);
    for (auto& v : z) v = {rnd(), rnd()};
    double worst = 0.0, big = 0.0;
    // forward: full
    ALL_LANES for (int m = 0; m < 8; ++m) a[lane][m] = z[lane + 64 * m];
    fft_forward_wave(a, xb.data());
    ALL_LANES for (int q = 0; q < 8; ++q) spec[q * 64 + lane] = a[lane][q];
    // forward: halves; F'_p[r + 64 a] is left by lane (r0, r1, r2), register a
    for (int p = 0; p < 2; ++p) ALL_LANES for (int n0 = 0; n0 < 4; ++n0) x[p][lane][n0] = z[2 * lane + p + 128 * n0];
    hfft_forward_wave<0>(x[0], xb.data());
    hfft_forward_wave<1>(x[1], xb.data());
    for (int p = 0; p < 2; ++p)
        ALL_LANES for (int q = 0; q < 4; ++q) half[p * fft::H + q * 64 + fft::h_in_pos(lane)] = x[p][lane][q];
    for (int q = 0; q < 8; ++q)
        ALL_LANES
        {
            const fft::cplx e = half[(q & 3) * 64 + lane], o = half[fft::H + (q & 3) * 64 + lane];
            const fft::cplx want = spec[q * 64 + lane], got = q < 4 ? fft::cadd(e, o) : fft::csub(e, o);
            worst = std::max(worst, std::max(std::fabs(got.re - want.re), std::fabs(got.im - want.im)));
            big = std::max(big, std::max(std::fabs(want.re), std::fabs(want.im)));
        }
    // inverse: full (arrangement F in, A out), then both halves from the same spectrum
    ALL_LANES for (int q = 0; q < 8; ++q) b[lane][q] = spec[q * 64 + lane];
    fft_inverse1_wave(b, xb.data());
    for (int p = 0; p < 2; ++p) {
        ALL_LANES for (int q = 0; q < 8; ++q) a[lane][q] = spec[q * 64 + fft::h_in_pos(lane)];
        if (p == 0) hfft_inverse_wave<0>(a, y, xb.data());
        else hfft_inverse_wave<1>(a, y, xb.data());
        ALL_LANES for (int n0 = 0; n0 < 4; ++n0)
        {
            const int j = 2 * lane + p + 128 * n0;
            const fft::cplx want = b[j & 63][j >> 6], got = y[lane][n0];
            worst = std::max(worst, std::max(std::fabs(got.re - want.re), std::fabs(got.im - want.im)));
            big = std::max(big, std::max(std::fabs(want.re), std::fabs(want.im)));
        }
    }
    return worst / big;
}
/* The paired inverse (fft_inverse2_wave: twiddle columns fetched once, both halves through one exchange buffer) against two
 * single inverses (fft_inverse1_wave) on the same two random spectra (integers of 16 bits times 2^scale_bits, the size of a
 * step's sums).  Returns the number of output doubles whose BIT PATTERNS differ (0: the same arithmetic in the same order). */
int iyk_emul_fft_inverse2_selftest(unsigned seed, int scale_bits)
{
    static thread_local fft::cplx a[64][8], b[64][8], ra[64][8], rb[64][8];
    std::vector<fft::cplx> xb(fft::XCHG_BYTES / sizeof(fft::cplx));
    u64 st = 0xA0761D6478BD642Full ^ seed;
    const double scale = std::ldexp(1.0, scale_bits);
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return ((double)(int32_t)(st >> 40) / 256.0 - 32768.0) * scale;
    };
    ALL_LANES for (int q = 0; q < 8; ++q) a[lane][q] = ra[lane][q] = {rnd(), rnd()};
    ALL_LANES for (int q = 0; q < 8; ++q) b[lane][q] = rb[lane][q] = {rnd(), rnd()};
    fft_inverse2_wave(a, b, xb.data());
    fft_inverse1_wave(ra, xb.data());
    fft_inverse1_wave(rb, xb.data());
    int bad = 0;
    ALL_LANES for (int q = 0; q < 8; ++q)
    {
        bad += std::memcmp(&a[lane][q].re, &ra[lane][q].re, 8) != 0;
        bad += std::memcmp(&a[lane][q].im, &ra[lane][q].im, 8) != 0;
        bad += std::memcmp(&b[lane][q].re, &rb[lane][q].re, 8) != 0;
        bad += std::memcmp(&b[lane][q].im, &rb[lane][q].im, 8) != 0;
    }
    return bad;
}
/* The rotated difference of both polynomials of one accumulator block acc [2][1024] for all 64 lanes, out [2][64][16].  form 0: two
 * calls of diff16; 1: diff16_pair's host path; 2: the host restatement of its device path's byte arithmetic
 * (diff16_pair_device_order).  set as above.  Returns 0, or -1 for an unknown set or form. */
int iyk_emul_diff16_pair(int set, uint32_t abar, const uint32_t* acc, int form, uint32_t* out)
{
    if (set == 0) return diff16_pair_forms<fft::Gadget<3, 6>>(abar, acc, form, out);
    if (set == 1) return diff16_pair_forms<fft::Gadget<2, 10>>(abar, acc, form, out);
    return -1;
}
/* The Linzer-Feig forward network (round 5) against a direct long-double evaluation A[k] = sum_j z[j] psi^(j (4 k + 1)) and
 * against the round-4 network on the same random input (integers of 16 bits).  which = 0: largest |LF - direct| relative to
 * sqrt(512) * ||z||_2 / sqrt(512) = ||z||_2 ... returned as max_abs_err / ||A||_2 * sqrt(512), i.e. in units where the proof's rho_F
 * applies (l2-relative, conservatively taken at the worst entry); which = 1: the same for the round-4 network; which = 2:
 * largest |LF - r04| / largest |A|. */
double iyk_emul_fft_lf_selftest(unsigned seed, int which)
{
    static thread_local fft::cplx a[64][8], b[64][8];
    std::vector<fft::cplx> xb(fft::XCHG_BYTES / sizeof(fft::cplx));
    u64 st = 0xD1B54A32D192ED03ull ^ seed;
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(int32_t)(st >> 40) / 256.0 - 32768.0;
    };
    std::vector<fft::cplx> z(fft::M);
    for (auto& v : z) v = {rnd(), rnd()};
    ALL_LANES for (int m = 0; m < 8; ++m) a[lane][m] = b[lane][m] = z[lane + 64 * m];
    fft_forward_lf_wave(a, xb.data());
    fft_forward_wave(b, xb.data());
    const long double pi = 3.14159265358979323846264338327950288L;
    long double norm2 = 0.0L, err_lf = 0.0L, err_old = 0.0L, diff = 0.0L, big = 0.0L;
    for (int k = 0; k < fft::M; ++k) {
        long double re = 0.0L, im = 0.0L;
        for (int j = 0; j < fft::M; ++j) {
            const long double ang = pi * (long double)(((long long)j * (4 * k + 1)) % 2048) / 1024.0L;
            const long double c = cosl(ang), sn = sinl(ang);
            re += (long double)z[j].re * c - (long double)z[j].im * sn;
            im += (long double)z[j].re * sn + (long double)z[j].im * c;
        }
        const int pos = fft::freq_pos(k);   // [k2][lane'']
        const fft::cplx g = a[pos & 63][pos >> 6], o = b[pos & 63][pos >> 6];
        norm2 += re * re + im * im;
        err_lf += (g.re - re) * (g.re - re) + (g.im - im) * (g.im - im);
        err_old += (o.re - re) * (o.re - re) + (o.im - im) * (o.im - im);
        diff = std::max(diff, std::max(fabsl((long double)g.re - o.re), fabsl((long double)g.im - o.im)));
        big = std::max(big, std::max(fabsl(re), fabsl(im)));
    }
    if (which == 0) return (double)sqrtl(err_lf / norm2);    // l2-relative error of the LF network
    if (which == 1) return (double)sqrtl(err_old / norm2);   // ... of the round-4 network
    return (double)(diff / big);
}
/* largest |z - rint(z)| over every inverse-transform output since the last reset */
double iyk_emul_fft_round_error(int reset)
{
    const double w = g_fft_worst;
    if (reset) g_fft_worst = 0.0;
    return w;
}


// ---- the host dispatch of iyokan_hip.hip (dispatch.hpp), for the tests that pin its Python mirrors -----------------------------
void iyk_emul_default_level_cost(int cus, int path, int set80, iyk_level_cost* out) { *out = dispatch::default_level_cost(cus, path, set80 != 0); }
double iyk_emul_level_cost_ms(const iyk_level_cost* c, long rot) { return dispatch::level_cost_ms(*c, rot); }
double iyk_emul_level_price_ms(const iyk_level_cost* c, long rot) { return dispatch::level_price_ms(*c, rot); }
/* out: family (0 active path, 1 FFT, 2 field), then [first, count) of the throughput and of the narrow part */
void iyk_emul_rot_split(int njobs, int round, int pass_cus, int max_passes, int forced, int out[5])
{
    const dispatch::RotSplit s = dispatch::rot_split(njobs, round, pass_cus, max_passes, forced);
    const int v[5] = {s.family, s.tp_first, s.tp_count, s.narrow_first, s.narrow_count};
    std::copy(v, v + 5, out);
}
/* ks_plan for every njobs[i], i < count: form (0 kind0, 1 shared, 2 wide, 3 table), groups, slices, i_per_slice.  A negative kind /
 * shared_max / shared_wg stands for the unset environment variable: dispatch.hpp's default. */
void iyk_emul_ks_plan(int kind, int shared_max, int shared_wg, const int* njobs, int count, int T, int nc, int cus, int* form,
                      int* groups, int* slices, int* i_per_slice)
{
    for (int i = 0; i < count; ++i) {
        const dispatch::KsPlan k = dispatch::ks_plan(kind < 0 ? dispatch::KS_KIND_DEFAULT : kind, shared_max < 0 ? dispatch::KS_SHARED_MAX_DEFAULT : shared_max,
                                                     shared_wg < 0 ? dispatch::KS_SHARED_WG_DEFAULT : shared_wg, njobs[i], T, nc, cus);
        form[i] = k.form, groups[i] = k.groups, slices[i] = k.slices, i_per_slice[i] = k.i_per_slice;
    }
}

// NTT of every polynomial q of the torus-domain BK, stored in the device layout (bk_dev_index)
int iyk_emul_bk_ntt(const iyk_params* p, const uint32_t* bk, uint64_t* bk_ntt)
{
    const size_t polys = (size_t)iyk_bk_words(p) / p->N;
    std::vector<u64> in(NTT_N);
    for (size_t q = 0; q < polys; ++q) {
        for (int x = 0; x < NTT_N; ++x) in[x] = bk[q * NTT_N + x];
        forward_1024_dev(in.data(), bk_ntt + q * NTT_N);
    }
    return 0;
}

int iyk_emul_blind_rotate(const iyk_params* p, const uint32_t* lin, const uint64_t* bk_ntt,
                          uint32_t* tlwe1)
{
    if (p->N != 1024 || p->k != 1) return -1;
    if (p->l == 3 && p->Bgbit == 6) blind_rotate<3, 6>(p, lin, bk_ntt, tlwe1);
    else if (p->l == 2 && p->Bgbit == 10) blind_rotate<2, 10>(p, lin, bk_ntt, tlwe1);
    else return -1;
    return 0;
}
/* the matrix form of the key switch (dispatch.hpp): does a batch run it (kind_env < 0: IYK_HIP_KS_KERNEL unset), the threshold, the
 * operand's size and layout (byte of (i, j, u, word, plane), u = digit value - 1; of (column k, word, plane)), the signed planes */
int iyk_emul_ks_matrix_form(int kind_env, int njobs, int T, int nc) { return dispatch::ks_matrix_form(kind_env, njobs, T, nc) ? 1 : 0; }
int iyk_emul_ks_matrix_min_jobs(void) { return dispatch::KS_MATRIX_MIN_JOBS; }
int iyk_emul_ks_matrix_gates(int per_wave) { return per_wave ? dispatch::KS_MATRIX_WAVE_GATES : dispatch::KS_MATRIX_GATES; }
int64_t iyk_emul_ks_matrix_bytes(int T, int nc) { return dispatch::ks_matrix_bytes(T, nc); }
int64_t iyk_emul_ks_matrix_offset(int T, int i, int j, int u, int word, int plane) { return dispatch::ks_matrix_offset(T, i, j, u, word, plane); }
void iyk_emul_ks_matrix_offsets_k(int T, const int* k, int word, int plane, int count, int64_t* out)
{
    for (int c = 0; c < count; ++c) out[c] = dispatch::ks_matrix_offset_k(T, k[c], word, plane);
}
void iyk_emul_ks_signed_planes(const uint32_t* w, int count, int8_t* planes /* [count][4] */)
{
    for (int c = 0; c < count; ++c)
        for (int p = 0; p < 4; ++p) planes[4 * c + p] = (int8_t)dispatch::ks_signed_plane(w[c], p);
}
/* privks_plan: splits and words per split of a private key-switch launch */
void iyk_emul_privks_plan(int njobs, int n_words, int cus, int out[2])
{
    const dispatch::PrivksPlan k = dispatch::privks_plan(njobs, n_words, cus);
    out[0] = k.splits, out[1] = k.i_per_split;
}
/* privks.hpp's digits of `count` 64-bit words as privks_kernel takes them: digits[count][t] */
void iyk_emul_privks_digits(const uint64_t* w, int count, uint32_t t, uint32_t basebit, uint32_t* digits)
{
    for (int g = 0; g < count; ++g) {
        const u64 wbar = privks_round(w[g], t, basebit);
        for (uint32_t j = 0; j < t; ++j) digits[(size_t)g * t + j] = privks_digit(wbar, j, basebit);
    }
}
}

/* ---- cb_rotate.hpp: the lvl0 -> lvl2 rotation's transform and one job, lane by lane ---------------------------------------------- */
namespace {
struct CbTables {
    std::vector<u64> tw;   // twf then twi
    CbTables() : tw(2 * CB_N) { cb_make_tables(tw.data(), tw.data() + CB_N); }
};
const CbTables& cb_tables()
{
    static CbTables t;
    return t;
}
// forward transform of field elements x[j] (natural) -> X[k] (natural), through one slot of the exchange buffer
void cb_forward(const u64* in, u64* out)
{
    const u64* twf = cb_tables().tw.data();
    std::vector<u64> bp(CB_PSTRIDE);
    for (int j1 = 0; j1 < 64; ++j1) {
        u64 x[32];
        for (int j2 = 0; j2 < 32; ++j2) x[j2] = gl_mul_pow2(in[j1 + 64 * j2], LOG_ZETA * j2);
        cb_pass1_fwd(j1, x, twf, bp.data());
    }
    std::vector<std::array<u64, 64>> X(32);
    for (int k2 = 0; k2 < 32; ++k2) cb_pass2_fwd_read(k2, bp.data(), reinterpret_cast<u64(&)[64]>(*X[k2].data()));
    for (int k2 = 0; k2 < 32; ++k2) cb_pass2_fwd_write(k2, reinterpret_cast<const u64(&)[64]>(*X[k2].data()), out);
}
void cb_inverse(const u64* in, u64* out)
{
    const u64* twi = cb_tables().tw.data() + CB_N;
    std::vector<u64> bp(in, in + CB_N);
    bp.resize(CB_PSTRIDE);
    std::vector<std::array<u64, 64>> X(32);
    for (int k2 = 0; k2 < 32; ++k2) cb_pass1_inv_read(k2, bp.data(), twi, reinterpret_cast<u64(&)[64]>(*X[k2].data()));
    for (int k2 = 0; k2 < 32; ++k2) cb_pass1_inv_write(k2, reinterpret_cast<const u64(&)[64]>(*X[k2].data()), bp.data());
    for (int j1 = 0; j1 < 64; ++j1) {
        u64 y[32];
        cb_pass2_inv(j1, bp.data(), y);
        for (int p = 0; p < 32; ++p) out[j1 + 64 * brv5(p)] = y[p];
    }
}

// lane-by-lane run of cb_rotate_kernel for one job: the same phase functions in the same order, one loop over the 256 lanes wherever
// the kernel has a barrier
// out: u64 [cb_outputs(k)][N2 + 1], the job's out taken as 0
template <int L2, int BGBIT2, class Job, class... Shared>
void cb_rotate(u32 n, const u32* w, const Job& jb, const u64* bk, u64* out, const Shared&... k)
{
    const u64* twf = cb_tables().tw.data();
    const u64* twi = twf + CB_N;
    std::vector<u64> acc(2 * CB_N), buf(4 * CB_PSTRIDE);
    std::vector<u32> abar(CB_N);
    struct Lane {
        u64 x[64], accum[32];
    };
    std::vector<Lane> R(CB_LANES);
#define CB_LANES_ALL for (int lane = 0; lane < CB_LANES; ++lane)
#define CB_LANES_HALF for (int lane = 0; lane < 128; ++lane)
    CB_LANES_ALL cb_prologue(lane, jb, w, n, abar.data(), acc.data(), k...);
    for (u32 i = 0; i < n; ++i) {
        const u32 ab = abar[i];
        const u64* bk_step = bk + (size_t)i * CB_STEP_WORDS;
        CB_LANES_ALL for (int q = 0; q < 32; ++q) R[lane].accum[q] = 0;
        for (int h = 0; h < 2; ++h) {
            CB_LANES_ALL cb_fwd1<L2, BGBIT2>(lane, h, ab, acc.data(), twf, buf.data());
            CB_LANES_HALF cb_pass2_fwd_read(lane & 31, buf.data() + (lane >> 5) * CB_PSTRIDE, R[lane].x);
            CB_LANES_HALF cb_pass2_fwd_write(lane & 31, R[lane].x, buf.data() + (lane >> 5) * CB_PSTRIDE);
            CB_LANES_ALL cb_mac<L2>(lane, h, buf.data(), bk_step, R[lane].accum);
        }
        CB_LANES_ALL cb_inv_write(lane, R[lane].accum, buf.data());
        CB_LANES_HALF cb_pass1_inv_read(lane & 31, buf.data() + (lane >> 5) * CB_PSTRIDE, twi, R[lane].x);
        CB_LANES_HALF cb_pass1_inv_write(lane & 31, R[lane].x, buf.data() + (lane >> 5) * CB_PSTRIDE);
        CB_LANES_ALL cb_inv2(lane, buf.data(), acc.data());
    }
    CB_LANES_ALL cb_epilogue<CB_LANES>(lane, jb, acc.data(), out, k...);
#undef CB_LANES_ALL
#undef CB_LANES_HALF
}
}  // namespace

extern "C" {
/* ntt64_dif on 64 field elements, result in natural order; inverse != 0: the root 2^-3 (unscaled) */
void iyk_emul_ntt64(const uint64_t* in, int inverse, uint64_t* out)
{
    u64 x[64];
    for (int j = 0; j < 64; ++j) x[j] = in[j];
    if (inverse) ntt64_dif<192 - LOG_ZETA>(x);
    else ntt64_dif<LOG_ZETA>(x);
    for (int p = 0; p < 64; ++p) out[brv6(p)] = x[p];
}
/* the N2 = 2048 negacyclic transform on canonical field elements, natural order on both sides; psi_out: the root it is built on */
void iyk_emul_cb_ntt(const uint64_t* in, int inverse, uint64_t* out, uint64_t* psi_out)
{
    if (inverse) cb_inverse(in, out);
    else cb_forward(in, out);
    if (psi_out) *psi_out = cb_find_psi();
}
/* signed gadget digits of `count` words: digits[count][l2] */
int iyk_emul_cb_digits(const uint64_t* x, int count, uint32_t l2, uint32_t Bgbit2, int32_t* digits)
{
    if (l2 != 4 || Bgbit2 != 9) return -1;
    for (int g = 0; g < count; ++g)
        for (int lvl = 0; lvl < 4; ++lvl) digits[g * 4 + lvl] = (int32_t)cb_digit_u<4, 9>(x[g], lvl) - (int32_t)CbConsts<4, 9>::half_bg;
    return 0;
}
/* bk2_ntt_kernel on the CPU: torus u64 [steps][8][2][N2] -> u64 [steps][2 halves][8][2][N2] */
void iyk_emul_bk2_ntt(uint64_t steps, const uint64_t* torus, uint64_t* dst)
{
    std::vector<u64> half(CB_N);
    for (uint64_t poly = 0; poly < steps * CB_ROWS * 2; ++poly)
        for (int hf = 0; hf < 2; ++hf) {
            const uint64_t step = poly / (CB_ROWS * 2), rc = poly % (CB_ROWS * 2);
            for (int j = 0; j < CB_N; ++j) half[j] = hf ? torus[poly * CB_N + j] >> 32 : (u64)(u32)torus[poly * CB_N + j];
            cb_forward(half.data(), dst + step * CB_STEP_WORDS + ((size_t)hf * CB_ROWS * 2 + rc) * CB_N);
        }
}
/* one job of cb_rotate_kernel: w = the n + 1 words of the lvl0 TLWE, out = u64 [N2 + 1] */
int iyk_emul_cb_rotate(uint32_t n, uint32_t l2, uint32_t Bgbit2, const uint32_t* w, int32_t sign, uint32_t off, uint64_t mu,
                       const uint64_t* bk_ntt, uint64_t* out)
{
    if (l2 != 4 || Bgbit2 != 9 || n == 0 || n > CB_MAX_N0 || (sign != 1 && sign != -1)) return -1;
    cb_rotate<4, 9>(n, w, CbJob{0, sign, off, 0, mu}, bk_ntt, out);
    return 0;
}
}

/* ---- cb_rotate_lat.hpp: the latency form's passes and one job, lane by lane; dispatch::cb_plan ------------------------------------ */
namespace {
// the N2 transform through the latency form's passes and one unpadded, swizzled slot
void cbl_forward(const u64* in, u64* out)
{
    const u64* twf = cb_tables().tw.data();
    std::vector<u64> bp(CBL_SLOT);
    for (int j1 = 0; j1 < 64; ++j1) {
        u64 x[32];
        for (int j2 = 0; j2 < 32; ++j2) x[j2] = gl_mul_pow2(in[j1 + 64 * j2], LOG_ZETA * j2);
        cbl_pass1_fwd(j1, x, twf, bp.data());
    }
    std::vector<std::array<u64, 32>> X(64);
    for (int u = 0; u < 64; ++u) cbl_pass2_fwd_read(u, bp.data(), reinterpret_cast<u64(&)[32]>(*X[u].data()));
    for (int u = 0; u < 64; ++u) cbl_pass2_fwd_write(u, reinterpret_cast<const u64(&)[32]>(*X[u].data()), out);
}
void cbl_inverse(const u64* in, u64* out)
{
    const u64* twi = cb_tables().tw.data() + CB_N;
    std::vector<u64> bp(in, in + CB_N);
    std::vector<std::array<u64, 32>> X(64);
    for (int u = 0; u < 64; ++u) cbl_pass1_inv_read(u, bp.data(), twi, reinterpret_cast<u64(&)[32]>(*X[u].data()));
    for (int u = 0; u < 64; ++u) cbl_pass1_inv_write(u, reinterpret_cast<const u64(&)[32]>(*X[u].data()), bp.data());
    for (int j1 = 0; j1 < 64; ++j1) {
        u64 y[32];
        cbl_pass2_inv(j1, bp.data(), y);
        for (int p = 0; p < 32; ++p) out[j1 + 64 * brv5(p)] = y[p];
    }
}

// lane-by-lane run of cb_rotate_lat_kernel for one job: the same phase functions in the same order, one loop over the lanes wherever
// the kernel has a workgroup barrier or a wave-level ordering point
template <int L2, int BGBIT2, class Job, class... Shared>
void cb_rotate_lat(u32 n, const u32* w, const Job& jb, const u64* bk, u64* out, const Shared&... k)
{
    const u64* twf = cb_tables().tw.data();
    const u64* twi = twf + CB_N;
    std::vector<u64> acc(2 * CB_N), buf((size_t)CB_ROWS * CBL_SLOT);
    struct Lane {
        u64 x[32], accum[16];
        CbPair pf[CBL_PF];
    };
    std::vector<Lane> R(CBL_LANES);
#define CBL_LANES_ALL for (int lane = 0; lane < CBL_LANES; ++lane)
#define CBL_LANES_INV for (int lane = 0; lane < 4 * 64; ++lane)
    CBL_LANES_ALL cbl_prologue(lane, jb, w, n, acc.data(), k...);
    CBL_LANES_ALL cbl_prefetch(lane, bk, R[lane].pf);
    u32 ab = cb_abar(jb, w, n, 0, k...);
    for (u32 i = 0; i < n; ++i) {
        const u64* bk_step = bk + (size_t)i * CB_STEP_WORDS;
        const u32 ab_next = cb_abar(jb, w, n, i + 1, k...);
        CBL_LANES_ALL cbl_fwd1<L2, BGBIT2>(lane, ab, acc.data(), twf, buf.data());
        CBL_LANES_ALL cbl_fwd2_read(lane, buf.data(), R[lane].x);
        CBL_LANES_ALL cbl_fwd2_write(lane, R[lane].x, buf.data());
        CBL_LANES_ALL cbl_mac(lane, buf.data(), bk_step, R[lane].pf, R[lane].accum);
        CBL_LANES_ALL cbl_inv_write(lane, R[lane].accum, buf.data());
        if (i + 1 < n) CBL_LANES_ALL cbl_prefetch(lane, bk_step + CB_STEP_WORDS, R[lane].pf);
        CBL_LANES_INV cbl_inv1_read(lane, buf.data(), twi, R[lane].x);
        CBL_LANES_INV cbl_inv1_write(lane, R[lane].x, buf.data());
        CBL_LANES_INV cbl_inv2(lane, buf.data(), acc.data());
        ab = ab_next;
    }
    CBL_LANES_ALL cb_epilogue<CBL_LANES>(lane, jb, acc.data(), out, k...);
#undef CBL_LANES_ALL
#undef CBL_LANES_INV
}
}  // namespace

extern "C" {
/* the latency form's 64-point pass alone (two lanes of 32 points, the first butterfly stage folded into the read), result in natural
 * order; inverse != 0: the root 2^-3, unscaled (a table of ones) */
void iyk_emul_cb_lat_ntt64(const uint64_t* in, int inverse, uint64_t* out)
{
    const int k2 = 5;
    std::vector<u64> bp(CBL_SLOT, 0), ones(CB_N, 1);
    for (int j = 0; j < 64; ++j) bp[inverse ? k2 + 32 * j : k2 * 64 + (j ^ k2)] = in[j];
    for (int half = 0; half < 2; ++half) {
        u64 x[32];
        if (inverse) cbl_pass1_inv_read(k2 + 32 * half, bp.data(), ones.data(), x);
        else cbl_pass2_fwd_read(k2 + 32 * half, bp.data(), x);
        for (int p = 0; p < 32; ++p) out[2 * brv5(p) + half] = x[p];
    }
}
/* the N2 = 2048 negacyclic transform through the latency form's passes, natural order on both sides */
void iyk_emul_cb_lat_ntt(const uint64_t* in, int inverse, uint64_t* out)
{
    if (inverse) cbl_inverse(in, out);
    else cbl_forward(in, out);
}
/* one job of cb_rotate_lat_kernel: the arguments of iyk_emul_cb_rotate */
int iyk_emul_cb_rotate_lat(uint32_t n, uint32_t l2, uint32_t Bgbit2, const uint32_t* w, int32_t sign, uint32_t off, uint64_t mu,
                           const uint64_t* bk_ntt, uint64_t* out)
{
    if (l2 != 4 || Bgbit2 != 9 || n == 0 || n > CB_MAX_N0 || (sign != 1 && sign != -1)) return -1;
    cb_rotate_lat<4, 9>(n, w, CbJob{0, sign, off, 0, mu}, bk_ntt, out);
    return 0;
}
/* dispatch::cb_plan; kind_env: -1 unset, 0 wg, 1 lat, 2 anything else.  Returns 0, or -1 where the kind is refused (form = -1, grid = 0) */
int iyk_emul_cb_plan(uint64_t count, int cus, int kind_env, int* form, int* grid)
{
    const dispatch::CbPlan p = dispatch::cb_plan((long)count, cus, kind_env);
    *form = p.form, *grid = p.grid;
    return p.form < 0 ? -1 : 0;
}
/* the kind cb_plan is given: what the text of IYK_HIP_CB_KERNEL names (null: unset) on a device that was or was not granted the latency form's LDS */
int iyk_emul_cb_kind(const char* text, int lat_granted) { return dispatch::cb_kind_for_device(dispatch::cb_kind_of(text), lat_granted != 0); }
/* dispatch::CB_LAT_MAX_JOBS: the widest batch the latency form takes when nothing is forced (0: none) */
uint64_t iyk_emul_cb_lat_max_jobs(void) { return (uint64_t)dispatch::CB_LAT_MAX_JOBS; }
}

/* ---- fft1024.hpp / cb_rotate_fft.hpp: the FP64 form of the lvl2 rotation — its transform, its key and one job, lane by lane ---------- */
namespace {
struct CbfTables {
    std::vector<cplx> tab;
    CbfTables() : tab(fft1k::TAB_POINTS) { fft1k::make_tables(tab.data()); }
};
const cplx* cbf_tables()
{
    static CbfTables t;
    return t.tab.data();
}
double g_cbf_worst = 0.0;   // largest |z - rint(z)| iyk_emul_cb_rotate_fft has met since the last reset

typedef std::array<cplx, 16> Cbf16;
inline cplx (&cbf_regs(Cbf16& a))[16] { return reinterpret_cast<cplx(&)[16]>(*a.data()); }

// z (time order, already folded) -> spectrum in position order, through one slot
void cbf_forward(std::vector<Cbf16>& X, cplx* sp)
{
    const cplx* tab = cbf_tables();
    for (int L = 0; L < 64; ++L) fft1k::fwd1(L, cbf_regs(X[L]), tab, sp);
    for (int L = 0; L < 64; ++L) fft1k::fwd2_read(L, tab, sp, cbf_regs(X[L]));
    for (int L = 0; L < 64; ++L) fft1k::fwd2_write(L, cbf_regs(X[L]), sp);
    for (int L = 0; L < 64; ++L) fft1k::fwd3_read(L, sp, cbf_regs(X[L]));
}
// spectrum in position order in sp -> the slot ready for fft1k::inv1
void cbf_inverse_to_last_pass(std::vector<Cbf16>& X, cplx* sp)
{
    const cplx* tab = cbf_tables();
    for (int L = 0; L < 64; ++L) fft1k::inv3_read(L, sp, cbf_regs(X[L]));
    for (int L = 0; L < 64; ++L) fft1k::inv3_write(L, cbf_regs(X[L]), sp);
    for (int L = 0; L < 64; ++L) fft1k::inv2_read(L, tab, sp, cbf_regs(X[L]));
    for (int L = 0; L < 64; ++L) fft1k::inv2_write(L, cbf_regs(X[L]), sp);
}

// lane-by-lane run of cb_rotate_fft_kernel for one job: the same phase functions in the same order, one loop over the lanes wherever
// the kernel has a workgroup barrier or a wave-level ordering point
template <int L2, int BGBIT2, class Job, class... Shared>
void cb_rotate_fft(u32 n, const u32* w, const Job& jb, const cplx* bk, u64* out, const Shared&... k)
{
    const cplx* tab = cbf_tables();
    std::vector<u64> acc(2 * CB_N);
    std::vector<cplx> buf((size_t)CB_ROWS * CBF_SLOT);
    struct Lane {
        cplx x[16], accum[16];
    };
    std::vector<Lane> R(CBF_LANES);
#define CBF_LANES_ALL for (int lane = 0; lane < CBF_LANES; ++lane)
    CBF_LANES_ALL cbl_prologue(lane, jb, w, n, acc.data(), k...);
    for (u32 i = 0; i < n; ++i) {
        const u32 ab = cb_abar(jb, w, n, i, k...);
        const cplx* bk_step = bk + (size_t)i * CBF_STEP_POINTS;
        CBF_LANES_ALL cbf_digits<L2, BGBIT2>(lane, ab, acc.data(), R[lane].x);
        CBF_LANES_ALL fft1k::fwd1(lane & 63, R[lane].x, tab, cbf_slot(buf.data(), lane));
        CBF_LANES_ALL fft1k::fwd2_read(lane & 63, tab, cbf_slot(buf.data(), lane), R[lane].x);
        CBF_LANES_ALL fft1k::fwd2_write(lane & 63, R[lane].x, cbf_slot(buf.data(), lane));
        CBF_LANES_ALL fft1k::fwd3_read(lane & 63, cbf_slot(buf.data(), lane), R[lane].x);
        CBF_LANES_ALL fft1k::spec_write(lane & 63, R[lane].x, cbf_slot(buf.data(), lane));
        CBF_LANES_ALL cbf_mac(lane, buf.data(), bk_step, R[lane].accum);
        CBF_LANES_ALL cbf_inv_write(lane, R[lane].accum, buf.data());
        CBF_LANES_ALL fft1k::inv3_read(lane & 63, cbf_slot(buf.data(), lane), R[lane].x);
        CBF_LANES_ALL fft1k::inv3_write(lane & 63, R[lane].x, cbf_slot(buf.data(), lane));
        CBF_LANES_ALL fft1k::inv2_read(lane & 63, tab, cbf_slot(buf.data(), lane), R[lane].x);
        CBF_LANES_ALL fft1k::inv2_write(lane & 63, R[lane].x, cbf_slot(buf.data(), lane));
        CBF_LANES_ALL g_cbf_worst = std::max(g_cbf_worst, cbf_inv_add<true>(lane, tab, buf.data(), acc.data()));
    }
    CBF_LANES_ALL cb_epilogue<CBF_LANES>(lane, jb, acc.data(), out, k...);
#undef CBF_LANES_ALL
}
}  // namespace

extern "C" {
/* the 1024-point transform of fft1024.hpp alone, in: double [1024][2], out: double [1024][2].  inverse == 0: z in time order ->
 * A[k] = sum_j z[j] psi^j W^(jk) in NATURAL frequency order (the position order undone through fft1k::freq_of_pos); inverse != 0:
 * C in natural frequency order -> psi^-j sum_k C[k] W^(-jk) in time order, unscaled (1024 times the inverse) */
void iyk_emul_fft1024(const double* in, int inverse, double* out)
{
    std::vector<cplx> sp(fft1k::M);
    std::vector<Cbf16> X(64);
    if (!inverse) {
        for (int L = 0; L < 64; ++L)
            for (int j2 = 0; j2 < 16; ++j2) X[L][j2] = {in[2 * (L + 64 * j2)], in[2 * (L + 64 * j2) + 1]};
        cbf_forward(X, sp.data());
        for (int L = 0; L < 64; ++L)
            for (int r = 0; r < 16; ++r) {
                const int k = fft1k::freq_of_pos(L + 64 * r);
                out[2 * k] = X[L][r].re, out[2 * k + 1] = X[L][r].im;
            }
        return;
    }
    for (int pos = 0; pos < fft1k::M; ++pos) sp[pos] = {in[2 * fft1k::freq_of_pos(pos)], in[2 * fft1k::freq_of_pos(pos) + 1]};
    cbf_inverse_to_last_pass(X, sp.data());
    for (int L = 0; L < 64; ++L) {
        fft1k::inv1(L, cbf_tables(), sp.data(), cbf_regs(X[L]));
        for (int j2 = 0; j2 < 16; ++j2) out[2 * (L + 64 * j2)] = X[L][j2].re, out[2 * (L + 64 * j2) + 1] = X[L][j2].im;
    }
}
/* the signed 16-bit quarters of `count` key words: q[count][4] */
void iyk_emul_cb_key_quarters(const uint64_t* w, int count, int32_t* q)
{
    for (int g = 0; g < count; ++g)
        for (int j = 0; j < 4; ++j) q[4 * g + j] = fft1k::key_quarter(w[g], j);
}
/* R_0 + (R_1 << 16) + (R_2 << 32) + (R_3 << 48) of `count` quadruples of doubles, each rounded as the kernel rounds */
void iyk_emul_cb_recombine(const double* z, int count, uint64_t* out)
{
    for (int g = 0; g < count; ++g) {
        const int64_t R[4] = {fft1k::round_i64(z[4 * g]), fft1k::round_i64(z[4 * g + 1]), fft1k::round_i64(z[4 * g + 2]), fft1k::round_i64(z[4 * g + 3])};
        out[g] = fft1k::recombine(R);
    }
}
/* bk2_fft_kernel on the CPU: torus u64 [steps][8][2][N2] -> double [steps][4 quarters][8][2][1024][2] */
void iyk_emul_bk2_fft(uint64_t steps, const uint64_t* torus, double* dst_)
{
    cplx* dst = reinterpret_cast<cplx*>(dst_);
    std::vector<cplx> sp(fft1k::M);
    std::vector<Cbf16> X(64);
    for (uint64_t poly = 0; poly < steps * CB_ROWS * 2; ++poly)
        for (int q = 0; q < CBF_QUARTERS; ++q) {
            for (int L = 0; L < 64; ++L) cbf_key_fold(L, q, torus + poly * CB_N, cbf_regs(X[L]));
            cbf_forward(X, sp.data());
            for (int L = 0; L < 64; ++L) cbf_key_write(L, cbf_regs(X[L]), dst + cbf_key_offset(poly / (CB_ROWS * 2), q, (int)(poly % (CB_ROWS * 2))));
        }
}
/* one job of cb_rotate_fft_kernel: the arguments of iyk_emul_cb_rotate with the key of iyk_emul_bk2_fft */
int iyk_emul_cb_rotate_fft(uint32_t n, uint32_t l2, uint32_t Bgbit2, const uint32_t* w, int32_t sign, uint32_t off, uint64_t mu,
                           const double* bk_fft, uint64_t* out)
{
    if (l2 != 4 || Bgbit2 != 9 || n == 0 || n > CB_MAX_N0 || (sign != 1 && sign != -1)) return -1;
    cb_rotate_fft<4, 9>(n, w, CbJob{0, sign, off, 0, mu}, reinterpret_cast<const cplx*>(bk_fft), out);
    return 0;
}
/* largest |z - rint(z)| over every rounded sum of iyk_emul_cb_rotate_fft since the last reset */
double iyk_emul_cb_fft_round_error(int reset)
{
    const double w = g_cbf_worst;
    if (reset) g_cbf_worst = 0.0;
    return w;
}
/* dispatch::cb_fft_grid, dispatch::bk2_form_known */
int iyk_emul_cb_fft_grid(int64_t count, int cus) { return dispatch::cb_fft_grid((long)count, cus); }

static CbManyMu cb_many_shared(uint32_t l, const uint64_t* mu)
{
    return CbManyMu{mu[0], l > 1 ? mu[1] : 0, l > 2 ? mu[2] : 0, l > 3 ? mu[3] : 0, l, args::cb_many_bw(l)};
}
/* ---- the many-digit form: one job of the CbManyJob instance of cb_rotate_kernel (form 0), cb_rotate_lat_kernel (1) or
 * cb_rotate_fft_kernel (2, bk: iyk_emul_bk2_fft's key), lane by lane.  mu: l words; out: u64 [l][N2 + 1] */
int iyk_emul_cb_rotate_many(int form, uint32_t n, uint32_t l2, uint32_t Bgbit2, const uint32_t* w, int32_t sign, uint32_t off, uint32_t l,
                            const uint64_t* mu, const void* bk, uint64_t* out)
{
    if (l2 != 4 || Bgbit2 != 9 || n == 0 || n > CB_MAX_N0 || (sign != 1 && sign != -1) || l < 1 || l > CB_MANY_MAX_L || form < 0 || form > 2) return -1;
    const CbManyMu k = cb_many_shared(l, mu);
    const CbManyJob jb{0, sign, off, 0};
    if (form == 0) cb_rotate<4, 9>(n, w, jb, static_cast<const u64*>(bk), out, k);
    else if (form == 1) cb_rotate_lat<4, 9>(n, w, jb, static_cast<const u64*>(bk), out, k);
    else cb_rotate_fft<4, 9>(n, w, jb, static_cast<const cplx*>(bk), out, k);
    return 0;
}
/* cb_epilogue alone on an accumulator u64 [2][N2] (a, then b), as the `lanes` (256 or 512) lanes of a kernel run it: out u64 [l][N2 + 1] */
int iyk_emul_cb_many_extract(const uint64_t* acc, int lanes, uint32_t l, const uint64_t* mu, uint64_t* out)
{
    if (l < 1 || l > CB_MANY_MAX_L || (lanes != CB_LANES && lanes != CBL_LANES)) return -1;
    const CbManyMu k = cb_many_shared(l, mu);
    const CbManyJob jb{0, 1, 0, 0};
    for (int lane = 0; lane < lanes; ++lane) {
        if (lanes == CB_LANES) cb_epilogue<CB_LANES>(lane, jb, acc, out, k);
        else cb_epilogue<CBL_LANES>(lane, jb, acc, out, k);
    }
    return 0;
}
/* the many-digit mod switch of `count` words: a[g] rounded, b[g] truncated (the value before 2 N2 - .), both multiples of 2^bw */
void iyk_emul_cb_many_modswitch(const uint32_t* x, int count, uint32_t bw, uint32_t* a, uint32_t* b)
{
    for (int g = 0; g < count; ++g) a[g] = cb_many_modswitch_a(x[g], bw), b[g] = (2u * CB_N - cb_many_modswitch_b(x[g], bw)) & (2u * CB_N - 1);
}
int iyk_emul_bk2_form_known(int form) { return dispatch::bk2_form_known(form) ? 1 : 0; }
}

/* ---- batch_args.hpp: the argument checks and job lists of the batch entry points ------------------------------------------------
 * Every iyk_emul_check_* returns the refusal's code and writes its text ("" when accepted) into msg[msg_cap].  An accepted call also
 * writes the job lists it built, one after the other, as 32-bit words into words[words_cap] (a list that does not fit is left out) and
 * the number of jobs of each list into counts[]. */
namespace {
struct CheckOut {
    char* msg;
    size_t msg_cap;
    uint32_t* words;
    uint64_t room;
    uint64_t* counts;
    int finish(const args::Refusal& r)
    {
        std::snprintf(msg, msg_cap, "%s", r.text ? r.text : "");
        return r.code;
    }
    template <class J>
    void list(const std::vector<J>& v)
    {
        static_assert(sizeof(J) % 4 == 0, "a job is whole words");
        const uint64_t n = v.size() * (sizeof(J) / 4);
        *counts++ = v.size();
        if (n > room) return;
        if (n) std::memcpy(words, v.data(), n * 4);
        words += n, room -= n;
    }
};
}  // namespace
#define IYK_CHECK_OUT char *msg, uint64_t msg_cap, uint32_t *words, uint64_t words_cap, uint64_t *counts
#define IYK_CHECK_OUT_INIT CheckOut o{msg, (size_t)msg_cap, words, words_cap, counts}
extern "C" {
int iyk_emul_check_slot_list(uint64_t count, const int32_t* slots, uint64_t arena_slots, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    return o.finish(args::check_slot_list(count, slots, arena_slots));
}
int iyk_emul_check_gate_batch(const iyk_params* p, int debug, uint64_t arena_slots, uint64_t count, const int32_t* ops, const int32_t* in0,
                              const int32_t* in1, const int32_t* in2, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<RotJob> rot;
    std::vector<KsJob> ks;
    std::vector<EwJob> ew;
    const args::Refusal r = args::check_gate_batch(*p, debug != 0, arena_slots, count, ops, in0, in1, in2, out, rot, ks, ew);
    if (!r) o.list(rot), o.list(ks), o.list(ew);
    return o.finish(r);
}
int iyk_emul_check_rotate_only(uint64_t arena_slots, uint64_t count, const int32_t* ia, const int32_t* ib, const int32_t* sa, const int32_t* sb,
                               const uint32_t* off, uint64_t out_rows, const int32_t* out_index, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<RotJob> rot;
    const args::Refusal r = args::check_rotate_only(arena_slots, count, ia, ib, sa, sb, off, out_rows, out_index, rot);
    if (!r) o.list(rot);
    return o.finish(r);
}
int iyk_emul_check_sample_extract_keyswitch(uint64_t trlwe_slots, uint64_t arena_slots, uint64_t count, const int32_t* trlwe_index,
                                            const int32_t* coeff_index, const int32_t* out_slot, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<KsJob> ks;
    const args::Refusal r = args::check_sample_extract_keyswitch(trlwe_slots, arena_slots, count, trlwe_index, coeff_index, out_slot, ks);
    if (!r) o.list(ks);
    return o.finish(r);
}
int iyk_emul_check_cmux_batch(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel, const int32_t* in0, const int32_t* in1,
                              const int32_t* rot, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<CmuxJob> jobs;
    const args::Refusal r = args::check_cmux_batch(trgsw_slots, trlwe_slots, count, sel, in0, in1, rot, out, jobs);
    if (!r) o.list(jobs);
    return o.finish(r);
}
int iyk_emul_check_cmux_chain_batch(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* steps,
                                    const uint32_t* pattern, const int32_t* src, const int32_t* mem, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<CmuxChainJob> jobs;
    const args::Refusal r = args::check_cmux_chain_batch(trgsw_slots, trlwe_slots, count, sel0, steps, pattern, src, mem, out, jobs);
    if (!r) o.list(jobs);
    return o.finish(r);
}
/* lists: the jobs {first, steps, src, out}, the steps {sel, rot} */
int iyk_emul_check_cmux_rotate_chain_batch(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* steps, const int32_t* sel,
                                           const int32_t* rot, const int32_t* src, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<CmuxRotChainJob> jobs;
    std::vector<CmuxRotStep> list;
    const args::Refusal r = args::cmux_rotate_chain_args(trgsw_slots, trlwe_slots, count, steps, sel, rot, src, out, jobs, list);
    if (!r) o.list(jobs), o.list(list);
    return o.finish(r);
}
/* dispatch::cmux_rotate_chain_grid */
int64_t iyk_emul_cmux_rotate_chain_grid(int64_t count) { return (int64_t)dispatch::cmux_rotate_chain_grid((long)count); }
/* list: the jobs {sel0, levels, first, out} */
int iyk_emul_check_cmux_tree_batch(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* levels,
                                   const int32_t* first, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<CmuxTreeJob> jobs;
    const args::Refusal r = args::cmux_tree_args(trgsw_slots, trlwe_slots, count, sel0, levels, first, out, jobs);
    if (!r) o.list(jobs);
    return o.finish(r);
}
/* dispatch::cmux_tree_grid */
int64_t iyk_emul_cmux_tree_grid(int64_t count) { return (int64_t)dispatch::cmux_tree_grid((long)count); }
int iyk_emul_check_trlwe_add_batch(uint64_t trlwe_slots, uint64_t count, const int32_t* a, const int32_t* b, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<TrlweAddJob> jobs;
    const args::Refusal r = args::check_trlwe_add_batch(trlwe_slots, count, a, b, out, jobs);
    if (!r) o.list(jobs);
    return o.finish(r);
}
int iyk_emul_check_privks_batch(uint32_t k, uint64_t tlwe2_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* in, const int32_t* c,
                                const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<PrivksJob> jobs;
    const args::Refusal r = args::check_privks_batch(k, tlwe2_slots, trlwe_slots, count, in, c, out, jobs);
    if (!r) o.list(jobs);
    return o.finish(r);
}
int iyk_emul_check_trgsw_from_rows(const iyk_params* p, uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* out_slot,
                                   const int32_t* rows, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    return o.finish(args::check_trgsw_from_rows(*p, trgsw_slots, trlwe_slots, count, out_slot, rows));
}
int iyk_emul_check_cb_rotate_batch(uint64_t tlwe0_slots, uint64_t tlwe2_slots, uint64_t count, const int32_t* in, const int32_t* sign,
                                   const uint32_t* off, const uint64_t* mu, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<CbJob> jobs;
    const args::Refusal r = args::check_cb_rotate_batch(tlwe0_slots, tlwe2_slots, count, in, sign, off, mu, out, jobs);
    if (!r) o.list(jobs);
    return o.finish(r);
}
/* lists: the jobs, then the shared CbManyMu as one element */
int iyk_emul_cb_rotate_many_args(uint64_t tlwe0_slots, uint64_t tlwe2_slots, uint64_t count, const int32_t* in, const int32_t* sign,
                                        const uint32_t* off, uint32_t l, const uint64_t* mu, const int32_t* out, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    std::vector<CbManyJob> jobs;
    std::vector<CbManyMu> shared(1);
    const args::Refusal r = args::cb_rotate_many_args(tlwe0_slots, tlwe2_slots, count, in, sign, off, l, mu, out, jobs, shared[0]);
    if (!r) o.list(jobs), o.list(shared);
    return o.finish(r);
}
/* lists: the rotations, the shared CbManyMu, the private key switches, the scratch rows of every selector, the selector slots */
int iyk_emul_circuit_bootstrap_many_args(const iyk_params* p, uint32_t bk2_n, uint32_t privks_n_in, uint64_t tlwe0_slots, const int32_t* in,
                                                const int32_t* sign, uint32_t tlwe2_n_in, uint64_t tlwe2_slots, uint64_t tlwe2_first,
                                                uint64_t trlwe_slots, uint64_t trgsw_slots, uint64_t trgsw_first, uint64_t bits, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    args::CbManyLists l;
    const args::Refusal r = args::circuit_bootstrap_many_args(*p, bk2_n, privks_n_in, tlwe0_slots, in, sign, tlwe2_n_in, tlwe2_slots,
                                                                     tlwe2_first, trlwe_slots, trgsw_slots, trgsw_first, bits, l);
    if (!r) o.list(l.rot), o.list(std::vector<CbManyMu>(1, l.shared)), o.list(l.privks), o.list(l.rows), o.list(l.sel);
    return o.finish(r);
}
/* lists: the rotations, the private key switches, the scratch rows of every selector, the selector slots */
int iyk_emul_check_circuit_bootstrap_batch(const iyk_params* p, uint32_t bk2_n, uint32_t privks_n_in, uint64_t tlwe0_slots, const int32_t* in,
                                           const int32_t* sign, uint32_t tlwe2_n_in, uint64_t tlwe2_slots, uint64_t tlwe2_first, uint64_t trlwe_slots,
                                           uint64_t trgsw_slots, uint64_t trgsw_first, uint64_t bits, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    args::CbLists l;
    const args::Refusal r = args::check_circuit_bootstrap_batch(*p, bk2_n, privks_n_in, tlwe0_slots, in, sign, tlwe2_n_in, tlwe2_slots, tlwe2_first,
                                                                trlwe_slots, trgsw_slots, trgsw_first, bits, l);
    if (!r) o.list(l.rot), o.list(l.privks), o.list(l.rows), o.list(l.sel);
    return o.finish(r);
}
/* args::stream_wait_args; st, other: the handles as integers (0 = null).  No job list. */
int iyk_emul_stream_wait_args(uint64_t st, uint64_t other, int st_replica, int other_replica, int st_ordinal, int other_ordinal, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    return o.finish(args::stream_wait_args((const void*)(uintptr_t)st, (const void*)(uintptr_t)other, st_replica, other_replica, st_ordinal,
                                           other_ordinal));
}
/* args::key_upload_seeded_args; the four pointers as integers (0 = null).  No job list. */
int iyk_emul_key_upload_seeded_args(uint64_t st, uint64_t key, uint64_t mask_seed, uint64_t host_b, int st_replica, int key_replica,
                                    int st_ordinal, int key_ordinal, uint64_t key_units, uint64_t first, uint64_t count, IYK_CHECK_OUT)
{
    IYK_CHECK_OUT_INIT;
    return o.finish(args::key_upload_seeded_args((const void*)(uintptr_t)st, (const void*)(uintptr_t)key, (const void*)(uintptr_t)mask_seed,
                                                 (const void*)(uintptr_t)host_b, st_replica, key_replica, st_ordinal, key_ordinal, key_units,
                                                 first, count));
}
}

/* ---- key_expand.hpp: key_mask_expand_kernel lane by lane, under the launch shape the library would give it on `cus` compute units ----
 * kind 1: dst = the first of row_count rows of the private key's device layout u32 [2 ring]; kind 2: the first of row_count rows of the
 * lvl2 key's staged torus-domain window, u64 [2 ring] as u32 words.  src_b: the window's b halves as the client sent them. */
extern "C" int iyk_emul_key_mask_expand(uint32_t kind, const uint8_t* mask_seed, uint64_t first_row, uint64_t row_count, uint32_t ring, int cus,
                                        uint32_t* dst, const uint32_t* src_b)
{
    if (!mask_seed || !dst || !src_b || ring == 0 || ring % kx::BLOCK_WORDS) return -1;
    const kx::MaskKey key = kx::mask_key_of(mask_seed);
    if (kind != kx::KIND_PRIVKS && kind != kx::KIND_BK2) return -1;
    const kx::ExpandArgs A = kind == kx::KIND_PRIVKS ? kx::privks_expand_args(key, first_row, row_count, ring)
                                                     : kx::bk2_expand_args(key, first_row, row_count, ring);
    if (!kx::expand_args_ok(A)) return -1;
    const uint64_t total = A.row_count * A.blocks_per_row, step = (uint64_t)kx::expand_grid(total, cus) * kx::EXPAND_THREADS;
    for (uint64_t lane = 0; lane < step; ++lane)   // every lane of the grid, each with the kernel's stride loop
        for (uint64_t g = lane; g < total; g += step) kx::expand_lane(A, g, dst, src_b);
    return 0;
}

/* ---- lane_jobs.hpp: K request packets of one circuit as one batch — iyk_emul_gate_batch_lanes_args, iyk_emul_lane_jobs, iyk_emul_lane_dispatch */
#include "lane_emul.hpp"

/* ---- cmux_lane_jobs.hpp: CMUX memories per lane — iyk_emul_cmux_lanes_args, iyk_emul_cmux_lane_jobs */
#include "cmux_lane_emul.hpp"
