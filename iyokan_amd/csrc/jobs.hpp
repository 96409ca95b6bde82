// jobs.hpp — the job descriptors a batch entry point uploads and a kernel reads, and the limits the argument checks use.
//
// Plain structs and constants only, no HIP include: the kernel headers include this file for the device side, batch_args.hpp (host
// only, visible to the CPU tests through libiyk_emul.so) builds and checks the lists.  The words of a job list ARE the upload: field
// order, types and sizes are the ABI between the two, pinned by the static_asserts below.
#pragma once
#include <stdint.h>

namespace iyk {

// one blind rotation: lin = sa*arena[ia] + sb*arena[ib] + (0,..,0,off)
struct RotJob {
    int32_t ia, ib;
    int32_t sa, sb;
    uint32_t off;
};

// one key switch: tlwe1 = rot[ra] (+ rot[rb] if rb >= 0) + (0,..,0,off); result -> arena[out]
struct KsJob {
    int32_t ra, rb;
    uint32_t off;
    int32_t out;
};

// NOT / COPY / CONST on arena slots
struct EwJob {
    int32_t op, in, out;
};

// T[out] = T[a] + T[b] on TRLWE rows (kernels.hpp: trlwe_add_kernel)
struct TrlweAddJob {
    int32_t a, b, out;
};

// one CMUX (cmux_fft.hpp): in1 >= 0 selects between two rows, in1 < 0 is the rotate form (X^rot - 1) T[in0]
struct CmuxJob {
    int32_t sel, in0, in1, rot, out;
};

// acc = T[src]; steps CMUXes against T[mem] with selector slots sel0 .. sel0 + steps - 1, oriented by the bits of pattern; T[out] = acc
struct CmuxChainJob {
    int32_t sel0, steps;
    uint32_t pattern;
    int32_t src, mem, out;
};

// acc = T[src]; steps rotate-form CMUXes acc += S[sel] [.] ((X^rot - 1) acc) with the (sel, rot) pairs first .. first + steps - 1 of the
// batch's step list (CmuxRotStep, uploaded behind the jobs); T[out] = acc (cmux_fft.hpp: cmux_rotate_chain_kernel)
struct CmuxRotChainJob {
    int32_t first, steps, src, out;
};
struct CmuxRotStep {
    int32_t sel, rot;
};

// A CMUX read tree of 2^levels leaves T[first ..]: level b < levels halves the candidates with selector slot sel0 + b — job i of a level is
// the CMUX (in0 = candidate 2 i, in1 = candidate 2 i + 1) — and T[out] is the one row left (cmux_fft.hpp: cmux_tree_kernel)
struct CmuxTreeJob {
    int32_t sel0, levels, first, out;
};

// private key switch of lvl2 TLWE `in` into TRLWE row `out` with the key's function c (privks.hpp)
struct PrivksJob {
    int32_t in, c, out;
};

// lvl0 -> lvl2 rotation of circuit bootstrapping (cb_rotate.hpp)
struct CbJob {
    int32_t in, sign;
    uint32_t off;
    int32_t out;
    uint64_t mu;
};

// the many-digit form of the same rotation: one job per address bit writes the l lvl2 TLWEs out .. out + l - 1
struct CbManyJob {
    int32_t in, sign;
    uint32_t off;
    int32_t out;
};
// what a many-digit batch shares, a kernel argument: mu[r] for r < l, 0 behind; bw = the smallest integer with 2^bw >= l
static constexpr uint32_t CB_MANY_MAX_L = 4;
struct CbManyMu {
    uint64_t mu0, mu1, mu2, mu3;   // named words, no array: a kernel argument read by index would be copied to scratch memory
    uint32_t l, bw;
};

static_assert(sizeof(RotJob) == 20 && sizeof(KsJob) == 16 && sizeof(EwJob) == 12 && sizeof(TrlweAddJob) == 12, "job layout is the upload format");
static_assert(sizeof(CmuxJob) == 20 && sizeof(CmuxChainJob) == 24 && sizeof(PrivksJob) == 12 && sizeof(CbJob) == 24, "job layout is the upload format");
static_assert(sizeof(CmuxRotChainJob) == 16 && sizeof(CmuxRotStep) == 8, "job layout is the upload format");
static_assert(sizeof(CmuxTreeJob) == 16, "job layout is the upload format");
static_assert(sizeof(CbManyJob) == 16 && sizeof(CbManyMu) == 40, "job layout is the upload format");

static constexpr int CMUX_CHAIN_MAX_STEPS = 32;       // the bits of CmuxChainJob::pattern
static constexpr int CMUX_ROT_CHAIN_MAX_STEPS = 32;   // steps of one CmuxRotChainJob: count * 32 steps bound the step list's 32-bit index
static constexpr int CMUX_TREE_MAX_LEVELS = 4;        // log2(2 BR_WAVES): level 0 of one CmuxTreeJob is one two-row CMUX per wave of a workgroup
static constexpr uint32_t CB_MAX_N0 = 2047;           // n + 1 mod-switched words fit the LDS abar array of cb_rotate_kernel
static constexpr uint32_t PRIVKS_MAX_N_IN = 1u << 16;
static constexpr uint32_t ABAR_STRIDE = 1024;         // words per job in a stream's mod-switched rotation inputs (n + 1 <= 768 used)

// Largest stores and batches an entry point accepts: every index of a job is an int32_t, and a store beyond these is no allocation
static constexpr uint64_t MAX_GATE_BATCH = 1u << 30;  // gates, rotations or extractions of one call
static constexpr uint64_t MAX_ROW_BATCH = 1u << 24;   // CMUX / chain / add jobs of one call
static constexpr uint64_t MAX_CB_BATCH = 1u << 20;    // private key switches or lvl2 rotations of one call
static constexpr uint64_t MAX_TRGSW_SLOTS = 1ull << 24;
static constexpr uint64_t MAX_STORE_ROWS = 1ull << 28;   // TRLWE rows, lvl0 / lvl2 TLWE slots

}  // namespace iyk
