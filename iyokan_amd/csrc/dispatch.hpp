// dispatch.hpp — which kernel runs a batch and with what launch shape, as pure functions of their arguments.
//
// Host only: no HIP include, no global state, plain C++17.  iyokan_hip.hip reads the environment and the device, calls these
// and launches what they say; emul.cpp (test support) exports them as iyk_emul_*, so the tests see every decision without a
// GPU.  A threshold is changed HERE, and these tests object until their mirrors follow:
//   tests/test_ks_words.py   ks_words.ks_geometry (what tests/test_gpu_keyswitch.py builds its case list from) == ks_plan
//   tests/test_netlist.py    frontier.make_level_cost / with_sub_pass_shape == level_cost_ms / level_price_ms;
//                            what rot_split launches costs what level_cost_ms says
#pragma once

#include <algorithm>

#include "../../include/iyokan_level_cost.h"

namespace iyk {
namespace dispatch {

// ---- blind rotation -------------------------------------------------------------------------------------------------------------

constexpr int ROT_WAVES = 8;   // rotations per workgroup of the wave-per-rotation kernels, one workgroup per CU (kernels.hpp: BR_WAVES)

// The compiled-in cost table (the only copy of these figures: iyokan_amd/frontier.py and host/iyokan_hip.hpp ask the library for
// it through iyk_hip_level_cost_*; build_id is left empty here, the library stamps its own).  Milliseconds: MI355X, this source
// revision (profiles/r04_sweep_*.txt); iyk_hip_calibrate() overwrites them with what the GPU at hand measures.
// path: 2 = complex FFT (the default: the wave-per-rotation kernel's round is the shortest), 1 = FP64 field, 0 = Goldilocks
// integers (ONE kernel, no narrow-frontier dispatch: max_passes = 0, a level costs whole rounds); set80: the 80-bit parameter set
// (n = 500, two digit levels: shorter rounds and passes).  ADVICE r04: the defaults used to be the 128-bit FFT figures whatever ran.
inline iyk_level_cost default_level_cost(int cus, int path, bool set80)
{
    iyk_level_cost c{};
    c.round = ROT_WAVES * cus;
    c.pass = cus;
    c.calibrated = 0;
    // one full round as iyk_hip_calibrate measures it (profiles/r05_model_inputs.json; inside a long launch a round is ~4 % shorter),
    // field paths: r03_bench*.json
    c.round_ms = path == 2 ? (set80 ? 9.4f : 14.5f) : path == 1 ? (set80 ? 20.0f : 19.7f) : (set80 ? 52.0f : 86.0f);
    // workgroup-per-rotation kernels, one pass = one rotation per CU: the FFT one (profiles/r05_model_inputs.json), the field one
    const float pass_fft[8] = {2.62f, 5.11f, 7.57f, 10.09f, 12.52f, 15.00f, 17.62f, 20.05f};
    const float pass_fft80[8] = {1.86f, 3.66f, 5.31f, 6.88f, 8.42f, 10.08f, 11.76f, 13.44f};
    const float pass_fp[8] = {3.33f, 6.96f, 10.23f, 13.52f, 16.79f, 20.1f, 23.4f, 26.7f};
    for (int j = 0; j < 8; ++j) c.pass_ms[j] = path == 2 ? (set80 ? pass_fft80[j] : pass_fft[j]) : pass_fp[j];
    c.max_passes = 0;
    if (path != 0)
        while (c.max_passes < 8 && c.pass_ms[c.max_passes] < c.round_ms) ++c.max_passes;
    return c;
}
inline double level_cost_ms(const iyk_level_cost& c, long rot) { return iyk_level_cost_ms(&c, rot); }
inline double level_price_ms(const iyk_level_cost& c, long rot) { return iyk_level_price_ms(&c, rot); }

// Which rotation kernel a batch is forced onto (IYK_HIP_ROT_KERNEL = fft / w32 / lat3 / latfft); ROT_AUTO: no override.
enum { ROT_AUTO = 0, ROT_W32 = 32, ROT_LAT3 = 3, ROT_FFT = 8, ROT_LATFFT = 9 };
// Which pair of kernels a split names: the active path's (FFT where the key spectra are resident, else the field), or one a
// forced kind names whatever is active.
enum { ROT_FAMILY_ACTIVE = 0, ROT_FAMILY_FFT = 1, ROT_FAMILY_FIELD = 2 };
struct RotSplit {
    int family;
    int tp_first, tp_count;           // [first, first + count) on the wave-per-rotation (throughput) kernel
    int narrow_first, narrow_count;   // ... on the workgroup-per-rotation (narrow-frontier) kernel; either part may be empty
};
// Full rounds (one job per resident wave: `round` = 8 x CUs) on the wave-per-rotation kernel; a remainder of up to max_passes x
// pass_cus rotations on the workgroup-per-rotation kernel (one CU per rotation, pass after pass); above that one more (partial)
// round of the wave-per-rotation kernel is faster, and the whole batch is one launch of it.  max_passes comes from the GPU's
// iyk_level_cost table, so that level_cost_ms prices exactly what this launches.  A forced kind takes the whole batch.
inline RotSplit rot_split(int njobs, int round, int pass_cus, int max_passes, int forced)
{
    if (forced == ROT_FFT) return {ROT_FAMILY_FFT, 0, njobs, njobs, 0};
    if (forced == ROT_LATFFT) return {ROT_FAMILY_FFT, 0, 0, 0, njobs};
    if (forced == ROT_W32) return {ROT_FAMILY_FIELD, 0, njobs, njobs, 0};
    if (forced == ROT_LAT3) return {ROT_FAMILY_FIELD, 0, 0, 0, njobs};
    const int rem = njobs % round, full = njobs - rem;
    if (rem > max_passes * pass_cus) return {ROT_FAMILY_ACTIVE, 0, njobs, njobs, 0};
    return {ROT_FAMILY_ACTIVE, 0, full, full, rem};
}

// ---- key switch -----------------------------------------------------------------------------------------------------------------

constexpr int KS_N = 1024;              // coefficients of a TLWE lvl1 mask: the i range the slices of a launch divide (NTT_N)
constexpr int KS_KIND0_GATES = 16;      // gates per workgroup of keyswitch_kernel (kernels.hpp: KS_G)
constexpr int KS_WAVE_GATES = 16;       // gates per wave of keyswitch_wave_kernel (its GW); a workgroup of the shared form holds GW, of the wide form 4 GW
constexpr int KS_TABLE_GATES = 128;     // gates per workgroup of keyswitch_lut_kernel (kernels.hpp: KSL_WAVES * KSL_G)
constexpr int KS_KIND_DEFAULT = 2;      // IYK_HIP_KS_KERNEL unset: the table for wide batches (round 6), the wave kernel's shared-gates form for narrow ones
constexpr int KS_LUT_MIN_JOBS = 4096;   // kind 2 up to here: the shared-gates form of keyswitch_wave_kernel (narrow frontiers)
constexpr int KS_SHARED_MAX_DEFAULT = 4096;   // IYK_HIP_KS_SHARED_MAX unset: largest batch on the shared-gates form (0 = never)
constexpr int KS_SHARED_WG_DEFAULT = 512;     // IYK_HIP_KS_SHARED_WG unset: workgroups a shared-form launch is sliced up to (A/B: profiles/r05_ks_small_ab.txt)

enum { KS_FORM_KIND0 = 0, KS_FORM_SHARED = 1, KS_FORM_WIDE = 2, KS_FORM_TABLE = 3 };
struct KsPlan {
    int form;          // KS_FORM_*: keyswitch_kernel, keyswitch_wave_kernel<SHARED = true / false>, keyswitch_lut_kernel
    int groups;        // grid x: workgroups along the gates
    int slices;        // grid y: parts of the i range, a power of two
    int i_per_slice;   // KS_N / slices
};
// Key switch: the outputs are initialised to (0,..,0,b'), then the partial sums are subtracted with integer atomics.  The i range
// is sliced so that at least ~2 workgroups per CU exist even for small frontiers.
// kind (IYK_HIP_KS_KERNEL): 2 = keyswitch_lut_kernel (pre-added rows selected by address) for batches above KS_LUT_MIN_JOBS and the
// wave kernel below, 1 = keyswitch_wave_kernel (a wave per 16 gates and whole rows), 0 = keyswitch_kernel (16 gates per
// workgroup, 3 words per thread).  The table and the wave kernel are instantiated for the (t, nc = row words / 128) of the two
// parameter sets only: every other shape runs keyswitch_kernel.
inline KsPlan ks_plan(int kind, int shared_max, int shared_wg, int njobs, int T, int nc, int cus)
{
    auto plan = [njobs](int form, int gates, int max_slices, int min_wg) {
        const int groups = (njobs + gates - 1) / gates;
        int slices = 1;
        while (slices < max_slices && groups * slices < min_wg) slices *= 2;
        return KsPlan{form, groups, slices, KS_N / slices};
    };
    const bool instantiated = (T == 7 && nc == 5) || (T == 8 && nc == 4);
    if (instantiated && kind == 2 && njobs > KS_LUT_MIN_JOBS) return plan(KS_FORM_TABLE, KS_TABLE_GATES, 8, cus);   // one workgroup per CU at a time
    if (instantiated && kind >= 1) {
        if (njobs > shared_max) return plan(KS_FORM_WIDE, 4 * KS_WAVE_GATES, 256, 512);
        // narrow frontier: a workgroup's four waves share GW gates and split the i range; a quarter of the atomics (kernels.hpp).
        // From four groups on a workgroup keeps at least 16 coefficients (64 slices), from two on at least 8 (128): cut finer, a launch
        // of 17 .. 127 gates spends its time on the atomics of its slices — 96 gates: 89 -> 68 us, 48 gates: 70 -> 48.5 us, 32 gates:
        // 49 -> 43 us, 64 gates: 59.5 -> 56 us (profiles/r06_plan_ab.txt; round 6's level plans make ~100-gate levels the common
        // case of a depth-bound netlist).  Per workgroup i_per_slice >= 4: one i per wave at least.
        const int groups = (njobs + KS_WAVE_GATES - 1) / KS_WAVE_GATES;
        return plan(KS_FORM_SHARED, KS_WAVE_GATES, groups >= 4 ? 64 : groups >= 2 ? 128 : 256, std::max(1, shared_wg));
    }
    return plan(KS_FORM_KIND0, KS_KIND0_GATES, 64, 512);
}

// ---- key switch as an integer matrix product (keyswitch_mfma.hpp) ---------------------------------------------------------------
//
// out = (0,..,0,b') - A x B mod 2^32: A[gate][k] is the one-hot form of the gate's digits, B[k][word] the key rows, each 32-bit word
// split into four signed base-256 planes so that the product runs on the int8 matrix instruction (32 x 32 x 32 per step).
//   k = 4 (i t + j) + v,  v = the digit's value: v = u + 1 selects row KSK[i][j][u]; v = 0 is padding (a zero row: digit 0 subtracts
//   nothing), so that a digit expands to one dword, 1 << 8 v, and a k-step of 32 is 8 whole digits.
// The operand is stored as the matrix instruction reads it: a CHUNK of 4 KB per (group of 32 words, k-step), in it one tile of 1 KB
// per plane, in it 16 bytes per lane (lane = 32 (half of the k-step) + word of the group): 16 consecutive k of one column.
constexpr int KS_MATRIX_MIN_JOBS = 4608;   // IYK_HIP_KS_KERNEL unset: batches from here on run the matrix form (sweep: profiles/ks_matrix_ab.txt)
constexpr int KS_MATRIX_GATES = 256;       // gates per workgroup of keyswitch_mfma_kernel: four waves of KS_MATRIX_WAVE_GATES
constexpr int KS_MATRIX_WAVE_GATES = 64;
constexpr int KS_MATRIX_WORDS = 32;        // words per workgroup (x 4 planes): grid y
constexpr long KS_MATRIX_TILE_BYTES = 1024, KS_MATRIX_CHUNK_BYTES = 4 * KS_MATRIX_TILE_BYTES;

constexpr int ks_matrix_ksteps(int T) { return KS_N * T * 4 / 32; }
constexpr int ks_matrix_word_groups(int nc) { return nc * 128 / KS_MATRIX_WORDS; }
constexpr long ks_matrix_bytes(int T, int nc) { return (long)ks_matrix_word_groups(nc) * ks_matrix_ksteps(T) * KS_MATRIX_CHUNK_BYTES; }
// where the chunk of (word group, k-step) starts
constexpr long ks_matrix_chunk_offset(int T, int word_group, int kstep) { return ((long)word_group * ks_matrix_ksteps(T) + kstep) * KS_MATRIX_CHUNK_BYTES; }
// byte of (column k, word, plane); THE layout: the build kernel writes through it, the product kernel and the tests read through it
constexpr long ks_matrix_offset_k(int T, int k, int word, int plane)
{
    return ks_matrix_chunk_offset(T, word / KS_MATRIX_WORDS, k / 32) + plane * KS_MATRIX_TILE_BYTES +
           (long)((k % 32 / 16) * 32 + word % KS_MATRIX_WORDS) * 16 + k % 16;
}
constexpr int ks_matrix_k(int T, int i, int j, int u) { return 4 * (i * T + j) + u + 1; }
constexpr long ks_matrix_offset(int T, int i, int j, int u, int word, int plane) { return ks_matrix_offset_k(T, ks_matrix_k(T, i, j, u), word, plane); }
// plane p of a word: signed base-256 digits s_p in [-128, 127] with sum s_p 256^p = w mod 2^32 (carries propagated, the top one dropped)
constexpr int ks_signed_plane(unsigned w, int plane)
{
    unsigned carry = 0, d = 0;
    for (int p = 0; p <= plane; ++p) {
        d = ((w >> (8 * p)) & 0xFFu) + carry;   // 0 .. 256
        carry = d >= 128u ? 1u : 0u;
    }
    return (int)d - (d >= 128u ? 256 : 0);
}
// Does the batch run the matrix form?  kind_env: what IYK_HIP_KS_KERNEL names, negative where it is unset or names nothing.
// Explicit 0 .. 2 keep ks_plan's meaning; the form exists for the (t, nc) of the two parameter sets only.
constexpr bool ks_matrix_form(int kind_env, int njobs, int T, int nc)
{
    const bool instantiated = (T == 7 && nc == 5) || (T == 8 && nc == 4);
    return instantiated && (kind_env == 3 || (kind_env < 0 && njobs >= KS_MATRIX_MIN_JOBS));
}

// ---- private key switch (privks.hpp) --------------------------------------------------------------------------------------------

constexpr int PRIVKS_WG_PER_CU = 4;   // workgroups of 256 lanes a launch aims to have per CU: 16 waves, each with up to PRIVKS_UNROLL rows in flight

struct PrivksPlan {
    int splits;        // workgroups per job: split s takes i in [s * i_per_split, min((s + 1) * i_per_split, n_words))
    int i_per_split;   // >= 1; (splits - 1) * i_per_split < n_words <= splits * i_per_split: no split is empty, every i has one owner
};
// A job streams the rows of n_words = n_in + 1 input words.  A batch is a handful of jobs (address bits x l x (k+1)), so the i range of
// every job is cut until the launch has ~PRIVKS_WG_PER_CU workgroups per CU, never finer than one word per workgroup.  The launch is
// 1-D: workgroup b is split b % splits of job b / splits.
inline PrivksPlan privks_plan(int njobs, int n_words, int cus)
{
    const long want = (long)PRIVKS_WG_PER_CU * std::max(1, cus);
    long s = (want + njobs - 1) / std::max(1, njobs);
    s = std::min<long>(std::max<long>(s, 1), n_words);
    const int per = (int)((n_words + s - 1) / s);
    return PrivksPlan{(n_words + per - 1) / per, per};
}

// ---- circuit bootstrapping's lvl0 -> lvl2 rotation (cb_rotate.hpp, cb_rotate_lat.hpp) ------------------------------------------

enum { CB_FORM_WG = 0, CB_FORM_LAT = 1 };   // cb_rotate_kernel (256 lanes), cb_rotate_lat_kernel (512 lanes, wave-owned polynomials)
// What IYK_HIP_CB_KERNEL names: unset, "wg", "lat", anything else
enum { CB_KIND_AUTO = -1, CB_KIND_WG = 0, CB_KIND_LAT = 1, CB_KIND_UNKNOWN = 2 };
// IYK_HIP_CB_KERNEL unset: batches of up to this many rotations run the latency form, wider ones cb_rotate_kernel; 0: none does.
// The widths at which the latency form was faster in every interleaved pair by more than the larger spread: all five measured, 1 to
// 258 rotations (two rounds on 256 CUs), at both parameter sets, by a factor of two (profiles/cb_rotate_lat_ab.txt).  Wider batches
// are more rounds of the same workgroups in either form, so no width is left to cb_rotate_kernel: no limit.
constexpr long CB_LAT_MAX_JOBS = 1L << 62;

struct CbPlan {
    int form;   // CB_FORM_*; negative: the kind is refused, nothing is launched
    int grid;   // workgroups: one per rotation up to one per CU, wider batches run in rounds inside the launch
};
constexpr int cb_kind_of(const char* text)
{
    if (!text) return CB_KIND_AUTO;
    if (text[0] == 'w' && text[1] == 'g' && text[2] == 0) return CB_KIND_WG;
    if (text[0] == 'l' && text[1] == 'a' && text[2] == 't' && text[3] == 0) return CB_KIND_LAT;
    return CB_KIND_UNKNOWN;
}
// A device that was not granted the latency form's LDS runs cb_rotate_kernel whatever is asked for; an unknown kind stays refused.
constexpr int cb_kind_for_device(int kind_env, bool lat_granted) { return lat_granted || kind_env == CB_KIND_UNKNOWN ? kind_env : CB_KIND_WG; }
constexpr CbPlan cb_plan(long count, int cus, int kind_env)
{
    const int grid = (int)(count < (long)cus ? count : (long)cus);
    if (kind_env == CB_KIND_WG) return {CB_FORM_WG, grid};
    if (kind_env == CB_KIND_LAT) return {CB_FORM_LAT, grid};
    if (kind_env != CB_KIND_AUTO) return {-1, 0};
    return {count <= CB_LAT_MAX_JOBS ? CB_FORM_LAT : CB_FORM_WG, grid};
}

// ---- the FP64 FFT form of the lvl2 key (cb_rotate_fft.hpp) ----------------------------------------------------------------------
// The form is a property of the key object (iyk_hip_bk2_key_create_form), not of the batch: a form-1 key has ONE kernel, and cb_plan
// above decides nothing for it (IYK_HIP_CB_KERNEL is still parsed, and an unknown value refused, before anything is staged).
enum { BK2_FORM_NTT = 0, BK2_FORM_FFT = 1 };
constexpr bool bk2_form_known(int form) { return form == BK2_FORM_NTT || form == BK2_FORM_FFT; }
// Workgroups of a cb_rotate_fft_kernel launch: one per rotation up to one per CU (the kernel takes a CU's whole LDS); a wider batch
// runs in rounds inside the launch, workgroup b taking jobs b, b + grid, ...  0 where there is nothing to launch.
constexpr int cb_fft_grid(long count, int cus)
{
    if (count <= 0 || cus <= 0) return 0;
    return (int)(count < (long)cus ? count : (long)cus);
}

// ---- the fused rotate chain of a ROM read (cmux_fft.hpp: cmux_rotate_chain_kernel) ----------------------------------------------
// One wave per job, ROT_WAVES jobs per workgroup, like every kernel of cmux_fft.hpp; the last workgroup may be partial.  0 where there
// is nothing to launch.
constexpr long cmux_rotate_chain_grid(long count) { return count <= 0 ? 0 : (count + ROT_WAVES - 1) / ROT_WAVES; }

// ---- the fused read tree of a ROM / RAM (cmux_fft.hpp: cmux_tree_kernel) ---------------------------------------------------------
// One WORKGROUP per job, unlike the kernels above: its ROT_WAVES waves are the up to 2^(4-1) CMUXes of the tree's first level.  0 where
// there is nothing to launch.
constexpr long cmux_tree_grid(long count) { return count <= 0 ? 0 : count; }

}  // namespace dispatch
}  // namespace iyk
