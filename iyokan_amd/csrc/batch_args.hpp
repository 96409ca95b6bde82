// batch_args.hpp — "are these arguments legal, and what job list do they make", as pure functions: one per batch entry point.
//
// Host only, like dispatch.hpp: no HIP include, no global state, no environment reads, plain C++17.  A function takes the caller's
// arrays and the sizes the caller states, plus the scalars of library state its checks read (iyk_params, the debug flag, a key's
// n_in / n), and returns the refusal — an error code and a string literal, nothing allocates — or fills the job vector(s) the entry
// point uploads.  iyokan_hip.hip keeps what needs the library's state or the device (not initialised, the FFT path, null handles,
// stream and key on one GPU, count == 0, hipSetDevice), calls these, stages the lists and launches; emul.cpp exports them as
// iyk_emul_check_*, so every refusal and every job word has a CPU test (tests/test_batch_args.py, tests/batch_refusal_cases.py).
//
// These checks are all that stands between a wrong index from a caller and an out-of-bounds device access.  The ORDER of the checks
// is part of the ABI's behaviour (which refusal a doubly wrong call gets): per-job checks stay in one loop, in the order written.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <unordered_map>
#include <vector>

#include "../../include/iyokan_hip.h"
#include "jobs.hpp"

namespace iyk {
namespace args {

constexpr int32_t RING_N = 1024;     // lvl1 ring degree of every kernel (ntt32.hpp: NTT_N)
constexpr uint32_t CB_RING_N = 2048; // lvl2 ring degree the circuit-bootstrapping rotation writes (cb_rotate.hpp: CB_N)

struct Refusal {
    int code;            // IYK_OK: accepted
    const char* text;    // a string literal, nullptr when accepted
    explicit operator bool() const { return code != IYK_OK; }
};
constexpr Refusal ACCEPT{IYK_OK, nullptr};
constexpr Refusal invalid(const char* text) { return Refusal{IYK_ERR_INVALID, text}; }

inline bool slot_ok(int32_t s, uint64_t slots) { return s >= 0 && (uint64_t)s < slots; }

// The independence contract of a batch, O(count): job g writes row out[g] and reads row ins[..][g] of every list given (a null list
// and a negative entry mean "nothing read").  No two jobs write one row; no job reads a row ANOTHER job writes (a job may write over
// what it reads itself, and jobs may share what they only read).  Duplicate writers are looked for first, over the whole batch.
enum Clash { CLASH_NONE, CLASH_TWO_WRITERS, CLASH_READ_OF_WRITTEN };
inline Clash find_clash(uint64_t count, const int32_t* out, std::initializer_list<const int32_t*> ins = {})
{
    std::unordered_map<int32_t, uint64_t> writer;   // out row -> its job
    writer.reserve(count * 2);
    for (uint64_t g = 0; g < count; ++g)
        if (!writer.emplace(out[g], g).second) return CLASH_TWO_WRITERS;
    for (uint64_t g = 0; g < count; ++g)
        for (const int32_t* in : ins) {
            if (!in || in[g] < 0) continue;
            const auto w = writer.find(in[g]);
            if (w != writer.end() && w->second != g) return CLASH_READ_OF_WRITTEN;
        }
    return CLASH_NONE;
}
// For the entry points that look for a second writer inside their per-job loop, after job g's index checks: a bad index at job g is
// reported unless two of the jobs before it write one row, which the loop would have reported first.
inline Refusal bad_index_or_earlier_writers(uint64_t g, const int32_t* out, const char* bad_index, const char* two_writers)
{
    return invalid(find_clash(g, out) == CLASH_TWO_WRITERS ? two_writers : bad_index);
}

// linear-step coefficients of TFHEpp HomGate (SURVEY.md §8 a-ext)
inline bool gate_coeffs(int op, uint32_t mu, int32_t& sa, int32_t& sb, uint32_t& off)
{
    switch (op) {
    case IYK_OP_AND: sa = 1; sb = 1; off = 0u - mu; return true;
    case IYK_OP_NAND: sa = -1; sb = -1; off = mu; return true;
    case IYK_OP_ANDNOT: sa = 1; sb = -1; off = 0u - mu; return true;
    case IYK_OP_OR: sa = 1; sb = 1; off = mu; return true;
    case IYK_OP_NOR: sa = -1; sb = -1; off = 0u - mu; return true;
    case IYK_OP_ORNOT: sa = 1; sb = -1; off = mu; return true;
    case IYK_OP_XOR: sa = 2; sb = 2; off = 2u * mu; return true;
    case IYK_OP_XNOR: sa = -2; sb = -2; off = 0u - 2u * mu; return true;
    default: return false;
    }
}

// ---- slot-list transfers (iyk_hip_arena_upload_slots / download_slots / sync_slots_multi) ------------------------------------------

// the range check; the cap on count stays with the three entry points
inline Refusal check_slot_list(uint64_t count, const int32_t* slots, uint64_t arena_slots)
{
    for (uint64_t g = 0; g < count; ++g)
        if (!slot_ok(slots[g], arena_slots)) return invalid("slot index outside the arena");
    return ACCEPT;
}

// ---- gates ----------------------------------------------------------------------------------------------------------------------

// iyk_hip_gate_batch: a binary gate is one rotation and one key switch, a MUX two rotations and one key switch of their sum + mu,
// NOT / COPY / CONST are elementwise.  debug (IYK_HIP_DEBUG=1 at init) also verifies the independence contract of the header.
inline Refusal check_gate_batch(const iyk_params& p, bool debug, uint64_t arena_slots, uint64_t count, const int32_t* ops, const int32_t* in0,
                                const int32_t* in1, const int32_t* in2, const int32_t* out, std::vector<RotJob>& rot, std::vector<KsJob>& ks,
                                std::vector<EwJob>& ew)
{
    if (count > MAX_GATE_BATCH) return invalid("batch too large");
    size_t nmux = 0;
    for (uint64_t g = 0; g < count; ++g) nmux += (ops[g] == IYK_OP_MUX);
    if (count + nmux > (size_t)INT32_MAX) return invalid("batch too large: more than 2^31 - 1 rotations");
    rot.reserve(count + nmux);
    ks.reserve(count);
    for (uint64_t g = 0; g < count; ++g) {
        const int op = ops[g];
        if (!slot_ok(out[g], arena_slots)) return invalid("output slot outside the arena");
        int32_t sa, sb;
        uint32_t off;
        if (gate_coeffs(op, p.mu, sa, sb, off)) {
            if (!slot_ok(in0[g], arena_slots) || !slot_ok(in1[g], arena_slots)) return invalid("binary gate needs two input slots inside the arena");
            ks.push_back(KsJob{(int32_t)rot.size(), -1, 0u, out[g]});
            rot.push_back(RotJob{in0[g], in1[g], sa, sb, off});
        }
        else if (op == IYK_OP_MUX) {
            // HomMUX(cs = in2, c1 = in1, c0 = in0): BR(cs + c1 - mu) + BR(c0 - cs - mu) + (0, mu) -> KS
            if (!slot_ok(in0[g], arena_slots) || !slot_ok(in1[g], arena_slots) || !slot_ok(in2[g], arena_slots))
                return invalid("MUX needs three input slots inside the arena");
            ks.push_back(KsJob{(int32_t)rot.size(), (int32_t)rot.size() + 1, p.mu, out[g]});
            rot.push_back(RotJob{in2[g], in1[g], 1, 1, 0u - p.mu});
            rot.push_back(RotJob{in0[g], in2[g], 1, -1, 0u - p.mu});
        }
        else if (op == IYK_OP_NOT || op == IYK_OP_COPY) {
            if (!slot_ok(in0[g], arena_slots)) return invalid("NOT/COPY needs one input slot inside the arena");
            ew.push_back(EwJob{op, in0[g], out[g]});
        }
        else if (op == IYK_OP_CONSTONE || op == IYK_OP_CONSTZERO) {
            ew.push_back(EwJob{op, -1, out[g]});
        }
        else {
            return invalid("unknown gate op");
        }
    }
    if (debug) {
        // only the inputs a gate's op reads count: the others may hold anything
        std::vector<int32_t> r0(count), r1(count), r2(count);
        for (uint64_t g = 0; g < count; ++g) {
            const int op = ops[g];
            const int nin = op == IYK_OP_MUX ? 3 : op < IYK_OP_MUX ? 2 : (op == IYK_OP_NOT || op == IYK_OP_COPY) ? 1 : 0;
            r0[g] = nin > 0 ? in0[g] : -1, r1[g] = nin > 1 ? in1[g] : -1, r2[g] = nin > 2 ? in2[g] : -1;
        }
        const Clash c = find_clash(count, out, {r0.data(), r1.data(), r2.data()});
        if (c == CLASH_TWO_WRITERS) return invalid("debug: two gates of one batch write the same slot");
        if (c == CLASH_READ_OF_WRITTEN) return invalid("debug: a gate reads a slot another gate of the same batch writes");
    }
    return ACCEPT;
}

// iyk_hip_gate_batch_lanes: `lanes` copies of one circuit's arena image in one arena, lane r in slots [r * lane_stride, (r + 1) *
// lane_stride); the descriptors are ONE lane's and stand for every lane, each at its own offset (lane_jobs.hpp).  The lists built are
// those of ONE lane: check_gate_batch with lane_stride in the place of arena_slots, so every index of a job lies inside one lane — and
// that is the whole proof that lanes do not touch each other, and why the debug independence check stays O(count): what holds inside
// lane 0 holds inside lane r, shifted.  What the expansion multiplies is bounded here, before anything is staged: slots (an index
// is an int32_t), jobs, rotation rows.  A refusal leaves the three lists empty.
// Not named check_*, for cmux_rotate_chain_args' reason below; tests/test_lane_jobs.py holds every refusal.
inline Refusal gate_batch_lanes_args(const iyk_params& p, bool debug, uint64_t arena_slots, uint64_t count, const int32_t* ops, const int32_t* in0,
                                     const int32_t* in1, const int32_t* in2, const int32_t* out, uint64_t lanes, uint64_t lane_stride,
                                     std::vector<RotJob>& rot, std::vector<KsJob>& ks, std::vector<EwJob>& ew)
{
    auto checked = [&]() -> Refusal {
        if (lanes == 0) return invalid("lanes is zero");
        if (lane_stride == 0) return invalid("lane stride is zero");
        if (lanes > arena_slots / lane_stride) return invalid("lanes x lane stride slots do not fit the arena");   // no product: lanes may be 2^40
        if (lanes * lane_stride > (1ull << 31)) return invalid("lanes x lane stride beyond the 2^31 slots an index can name");
        if (count > MAX_GATE_BATCH || lanes > MAX_GATE_BATCH || count * lanes > MAX_GATE_BATCH) return invalid("batch too large: count x lanes");
        if (Refusal r = check_gate_batch(p, debug, lane_stride, count, ops, in0, in1, in2, out, rot, ks, ew)) return r;
        if ((uint64_t)rot.size() * lanes > (uint64_t)INT32_MAX) return invalid("batch too large: more than 2^31 - 1 rotations");
        return ACCEPT;
    };
    const Refusal r = checked();
    if (r) rot.clear(), ks.clear(), ew.clear();
    return r;
}

// rotate_only, the body of iyk_hip_blind_rotate_batch (out_index null, out_rows 0) and iyk_hip_bootstrap_trlwe_batch
inline Refusal check_rotate_only(uint64_t arena_slots, uint64_t count, const int32_t* ia, const int32_t* ib, const int32_t* sa, const int32_t* sb,
                                 const uint32_t* off, uint64_t out_rows, const int32_t* out_index, std::vector<RotJob>& rot)
{
    if (count > MAX_GATE_BATCH) return invalid("batch too large");
    rot.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(ia[g], arena_slots) || (ib[g] >= 0 && !slot_ok(ib[g], arena_slots))) return invalid("input slot outside the arena");
        if (out_index && !slot_ok(out_index[g], out_rows)) return invalid("output index outside the buffer");
        rot[g] = RotJob{ia[g], ib[g], sa[g], sb[g], off[g]};
    }
    if (!out_index && out_rows && count > out_rows) return invalid("more jobs than output rows");
    return ACCEPT;
}

// iyk_hip_sample_extract_keyswitch_batch, and with coeff_index iyk_hip_sample_extract_index_keyswitch_batch: extraction g lands in
// rotation row g, which key switch g reads
inline Refusal check_sample_extract_keyswitch(uint64_t trlwe_slots, uint64_t arena_slots, uint64_t count, const int32_t* trlwe_index,
                                              const int32_t* coeff_index, const int32_t* out_slot, std::vector<KsJob>& ks)
{
    if (count > MAX_GATE_BATCH) return invalid("batch too large");
    ks.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(trlwe_index[g], trlwe_slots)) return invalid("TRLWE index outside the buffer");
        if (coeff_index && (coeff_index[g] < 0 || coeff_index[g] >= RING_N)) return invalid("coefficient index outside [0, N)");
        if (!slot_ok(out_slot[g], arena_slots)) return invalid("output slot outside the arena");
        ks[g] = KsJob{(int32_t)g, -1, 0u, out_slot[g]};
    }
    return ACCEPT;
}

// ---- CMUX memories --------------------------------------------------------------------------------------------------------------

// iyk_hip_cmux_batch.  A second writer at job g is reported before a bad index at job g + 1.
inline Refusal check_cmux_batch(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel, const int32_t* in0,
                                const int32_t* in1, const int32_t* rot, const int32_t* out, std::vector<CmuxJob>& jobs)
{
    if (count > MAX_ROW_BATCH) return invalid("batch too large");
    if (trgsw_slots > MAX_TRGSW_SLOTS || trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    const char* const two_writers = "two jobs of one batch write the same TRLWE row";
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(sel[g], trgsw_slots)) return bad_index_or_earlier_writers(g, out, "selector index outside the selector store", two_writers);
        if (!slot_ok(in0[g], trlwe_slots) || !slot_ok(out[g], trlwe_slots) || (in1[g] >= 0 && !slot_ok(in1[g], trlwe_slots)))
            return bad_index_or_earlier_writers(g, out, "TRLWE index outside the buffer", two_writers);
        if (in1[g] < 0 && (rot[g] < 0 || rot[g] >= 2 * RING_N)) return bad_index_or_earlier_writers(g, out, "rot outside [0, 2N)", two_writers);
        jobs[g] = CmuxJob{sel[g], in0[g], in1[g] >= 0 ? in1[g] : -1, in1[g] >= 0 ? 0 : rot[g], out[g]};
    }
    const Clash c = find_clash(count, out, {in0, in1});   // a job may write over its own inputs, never over another job's
    if (c == CLASH_TWO_WRITERS) return invalid(two_writers);
    if (c == CLASH_READ_OF_WRITTEN) return invalid("a job reads a TRLWE row that another job of the batch writes");
    return ACCEPT;
}

// iyk_hip_cmux_chain_batch
inline Refusal check_cmux_chain_batch(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* steps,
                                      const uint32_t* pattern, const int32_t* src, const int32_t* mem, const int32_t* out,
                                      std::vector<CmuxChainJob>& jobs)
{
    if (count > MAX_ROW_BATCH) return invalid("batch too large");
    if (trgsw_slots > MAX_TRGSW_SLOTS || trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (steps[g] < 1 || steps[g] > CMUX_CHAIN_MAX_STEPS) return invalid("steps outside [1, 32]");
        if (sel0[g] < 0 || (uint64_t)sel0[g] + (uint64_t)steps[g] > trgsw_slots)
            return invalid("selector slots sel0 .. sel0 + steps - 1 outside the selector store");
        if (!slot_ok(src[g], trlwe_slots) || !slot_ok(mem[g], trlwe_slots) || !slot_ok(out[g], trlwe_slots))
            return invalid("TRLWE index outside the buffer");
        jobs[g] = CmuxChainJob{sel0[g], steps[g], pattern[g], src[g], mem[g], out[g]};
    }
    const Clash c = find_clash(count, out, {src, mem});
    if (c == CLASH_TWO_WRITERS) return invalid("two jobs of one batch write the same TRLWE row");
    if (c == CLASH_READ_OF_WRITTEN) return invalid("a job reads a TRLWE row that another job of the batch writes");
    return ACCEPT;
}

// iyk_hip_cmux_rotate_chain_batch, O(count + sum of steps).  sel and rot hold the jobs' steps one after the other: job g's are entries
// first[g] .. first[g] + steps[g] - 1, first[g] the sum of the steps before it — so steps[g] is checked before any of its entries is
// read, and nothing is read behind the entries the accepted jobs before it account for.
// Not named check_*: the check_* functions are the ones whose answers tests/golden/batch_refusals_parent.json records from a library
// that had them (tests/test_batch_args.py lists them by that name); this entry point is newer than the record, and its refusals and
// job words have tests/test_rom_chain_args.py, which also holds every text below against a set that reaches it.
inline Refusal cmux_rotate_chain_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* steps, const int32_t* sel,
                                      const int32_t* rot, const int32_t* src, const int32_t* out, std::vector<CmuxRotChainJob>& jobs,
                                      std::vector<CmuxRotStep>& list)
{
    if (count > MAX_ROW_BATCH) return invalid("batch too large");
    if (trgsw_slots > MAX_TRGSW_SLOTS || trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    jobs.resize(count);
    list.clear();
    list.reserve(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (steps[g] < 1 || steps[g] > CMUX_ROT_CHAIN_MAX_STEPS) return invalid("steps outside [1, 32]");
        const size_t first = list.size();   // <= 2^24 * 32: an int32_t
        for (int32_t j = 0; j < steps[g]; ++j) {
            if (!slot_ok(sel[first + j], trgsw_slots)) return invalid("selector index outside the selector store");
            if (rot[first + j] < 0 || rot[first + j] >= 2 * RING_N) return invalid("rot outside [0, 2N)");
            list.push_back(CmuxRotStep{sel[first + j], rot[first + j]});
        }
        if (!slot_ok(src[g], trlwe_slots) || !slot_ok(out[g], trlwe_slots)) return invalid("TRLWE index outside the buffer");
        jobs[g] = CmuxRotChainJob{(int32_t)first, steps[g], src[g], out[g]};
    }
    const Clash c = find_clash(count, out, {src});   // a job may write over its own src, jobs may share src
    if (c == CLASH_TWO_WRITERS) return invalid("two jobs of one batch write the same TRLWE row");
    if (c == CLASH_READ_OF_WRITTEN) return invalid("a job reads a TRLWE row that another job of the batch writes");
    return ACCEPT;
}

// iyk_hip_cmux_tree_batch, O(count * 2^levels).  Job g reads its 2^levels[g] leaves first[g] .. and writes out[g] alone (every row in
// between stays in the workgroup's LDS).  A job may write over one of its OWN leaves — the workgroup has read them all before wave 0
// stores — and jobs may share leaves, as the reads of one ROM all start from its data rows; no out is a leaf or the out of ANOTHER job.
// Named like cmux_rotate_chain_args and for its reason: newer than the record tests/test_batch_args.py holds the check_* functions
// against; tests/test_cmux_tree_emulation.py has every refusal text below against a set that reaches it.
inline Refusal cmux_tree_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* levels,
                              const int32_t* first, const int32_t* out, std::vector<CmuxTreeJob>& jobs)
{
    if (count > MAX_ROW_BATCH) return invalid("batch too large");
    if (trgsw_slots > MAX_TRGSW_SLOTS || trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (levels[g] < 1 || levels[g] > CMUX_TREE_MAX_LEVELS) return invalid("levels outside [1, 4]");
        if (!slot_ok(sel0[g], trgsw_slots) || (uint64_t)sel0[g] + (uint64_t)levels[g] > trgsw_slots)
            return invalid("selector index outside the selector store");
        if (!slot_ok(first[g], trlwe_slots) || (uint64_t)first[g] + (1ull << levels[g]) > trlwe_slots || !slot_ok(out[g], trlwe_slots))
            return invalid("TRLWE index outside the buffer");
        jobs[g] = CmuxTreeJob{sel0[g], levels[g], first[g], out[g]};
    }
    if (find_clash(count, out) == CLASH_TWO_WRITERS) return invalid("two jobs of one batch write the same TRLWE row");
    std::unordered_map<int32_t, uint64_t> writer;   // out row -> its job
    writer.reserve(count * 2);
    for (uint64_t g = 0; g < count; ++g) writer.emplace(out[g], g);
    for (uint64_t g = 0; g < count; ++g)
        for (int32_t k = 0; k < (1 << levels[g]); ++k) {
            const auto w = writer.find(first[g] + k);
            if (w != writer.end() && w->second != g) return invalid("a job reads a TRLWE row that another job of the batch writes");
        }
    return ACCEPT;
}

// ---- CMUX memories per lane (iyk_hip_cmux_*_batch_lanes, cmux_lane_jobs.hpp) ----------------------------------------------------
// `lanes` copies of one memory: lane r's rows are lane 0's + r * row_stride, its selector slots lane 0's + r * sel_stride.  The arrays
// are ONE lane's.  Each *_lanes_args below, before anything is staged:
//   (d) refuses lanes == 0, a zero stride with lanes > 1 and count x lanes > MAX_ROW_BATCH (no product before both factors are bounded:
//       lanes may be 2^31);
//   (a) runs the parent's check of lane 0's list against the WHOLE stores — indices, independence inside the lane;
//   (b) the span rule: the rows lane 0's list touches span less than row_stride (max - min < row_stride), so lane r's rows — the same
//       rows + r * row_stride — are disjoint from those of every other lane: what (a) proved inside lane 0 holds for the whole batch,
//       and the proof stays O(count) (a tree: O(count) too, its leaves are the range first .. first + 2^levels - 1);
//   (c) the highest row + (lanes - 1) * row_stride lies inside the TRLWE store and the highest selector slot + (lanes - 1) * sel_stride
//       inside the selector store, by division; both stores are at most 2^28, so no offset index reaches 2^31 (checked all the same).
// Selector slots are only read: lanes may interleave them (sel_stride smaller than a list's selector span: the stage-major layout).
// lanes == 1: the strides are not looked at, the check is the parent's.  A refusal leaves the list(s) empty.
// Not named check_*, for cmux_rotate_chain_args' reason above; tests/test_cmux_lane_jobs.py holds every refusal.
struct LaneReach {
    int64_t row_lo = INT64_MAX, row_hi = -1, sel_hi = -1;   // of one lane's list
    void row(int64_t i) { row_lo = i < row_lo ? i : row_lo, row_hi = i > row_hi ? i : row_hi; }
    void sel(int64_t i) { sel_hi = i > sel_hi ? i : sel_hi; }
};
inline Refusal cmux_lanes_counts(uint64_t count, uint64_t lanes, uint64_t sel_stride, uint64_t row_stride)
{
    if (lanes == 0) return invalid("lanes is zero");
    if (lanes > 1 && (sel_stride == 0 || row_stride == 0)) return invalid("a stride is zero with more than one lane");
    if (count > MAX_ROW_BATCH || lanes > MAX_ROW_BATCH || count * lanes > MAX_ROW_BATCH) return invalid("batch too large: count x lanes");
    return ACCEPT;
}
inline Refusal cmux_lanes_reach(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t lanes, uint64_t sel_stride, uint64_t row_stride, const LaneReach& m)
{
    if (lanes == 1 || m.row_hi < 0) return ACCEPT;
    if ((uint64_t)(m.row_hi - m.row_lo) >= row_stride) return invalid("the rows of one lane's jobs span row_stride or more: two lanes would share a row");
    const uint64_t more = lanes - 1;
    if (more > (trlwe_slots - 1 - (uint64_t)m.row_hi) / row_stride) return invalid("the last lane's rows lie outside the TRLWE store");
    if (more > (trgsw_slots - 1 - (uint64_t)m.sel_hi) / sel_stride) return invalid("the last lane's selector slots lie outside the selector store");
    if (more > ((uint64_t)INT32_MAX - (uint64_t)m.row_hi) / row_stride || more > ((uint64_t)INT32_MAX - (uint64_t)m.sel_hi) / sel_stride)
        return invalid("an index of the last lane beyond 2^31 - 1");
    return ACCEPT;
}

// The frame the four checkers below share: (d), then the parent's check (a), which fills the list(s), then `reach` — the kernel's own
// lines: the rows and selector slots ONE lane's list(s) touch — into (b) and (c).  list: the step list, rotate_chain alone (else null);
// its sum(steps) x lanes entries stay inside the 32-bit CmuxRotChainJob::first.  A refusal leaves the list(s) empty.
template <class Job, class Parent, class Reach>
Refusal cmux_lanes_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, uint64_t lanes, uint64_t sel_stride, uint64_t row_stride,
                        std::vector<Job>& jobs, std::vector<CmuxRotStep>* list, Parent parent, Reach reach)
{
    auto checked = [&]() -> Refusal {
        if (Refusal r = cmux_lanes_counts(count, lanes, sel_stride, row_stride)) return r;
        if (Refusal r = parent()) return r;
        if (list && (uint64_t)list->size() * lanes > (uint64_t)INT32_MAX) return invalid("batch too large: more than 2^31 - 1 steps");
        LaneReach m;
        reach(m);
        return cmux_lanes_reach(trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride, m);
    };
    const Refusal r = checked();
    if (r) jobs.clear();
    if (r && list) list->clear();
    return r;
}

inline Refusal cmux_batch_lanes_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel, const int32_t* in0,
                                     const int32_t* in1, const int32_t* rot, const int32_t* out, uint64_t lanes, uint64_t sel_stride,
                                     uint64_t row_stride, std::vector<CmuxJob>& jobs)
{
    return cmux_lanes_args(trgsw_slots, trlwe_slots, count, lanes, sel_stride, row_stride, jobs, nullptr,
        [&] { return check_cmux_batch(trgsw_slots, trlwe_slots, count, sel, in0, in1, rot, out, jobs); },
        [&](LaneReach& m) {
            for (const CmuxJob& j : jobs) {
                m.sel(j.sel), m.row(j.in0), m.row(j.out);
                if (j.in1 >= 0) m.row(j.in1);
            }
        });
}

inline Refusal cmux_chain_batch_lanes_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* steps,
                                           const uint32_t* pattern, const int32_t* src, const int32_t* mem, const int32_t* out, uint64_t lanes,
                                           uint64_t sel_stride, uint64_t row_stride, std::vector<CmuxChainJob>& jobs)
{
    return cmux_lanes_args(trgsw_slots, trlwe_slots, count, lanes, sel_stride, row_stride, jobs, nullptr,
        [&] { return check_cmux_chain_batch(trgsw_slots, trlwe_slots, count, sel0, steps, pattern, src, mem, out, jobs); },
        [&](LaneReach& m) {
            for (const CmuxChainJob& j : jobs) m.sel((int64_t)j.sel0 + j.steps - 1), m.row(j.src), m.row(j.mem), m.row(j.out);
        });
}

inline Refusal cmux_rotate_chain_batch_lanes_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* steps, const int32_t* sel,
                                                  const int32_t* rot, const int32_t* src, const int32_t* out, uint64_t lanes, uint64_t sel_stride,
                                                  uint64_t row_stride, std::vector<CmuxRotChainJob>& jobs, std::vector<CmuxRotStep>& list)
{
    return cmux_lanes_args(trgsw_slots, trlwe_slots, count, lanes, sel_stride, row_stride, jobs, &list,
        [&] { return cmux_rotate_chain_args(trgsw_slots, trlwe_slots, count, steps, sel, rot, src, out, jobs, list); },
        [&](LaneReach& m) {
            for (const CmuxRotChainJob& j : jobs) m.row(j.src), m.row(j.out);
            for (const CmuxRotStep& s : list) m.sel(s.sel);
        });
}

inline Refusal cmux_tree_batch_lanes_args(uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* levels,
                                          const int32_t* first, const int32_t* out, uint64_t lanes, uint64_t sel_stride, uint64_t row_stride,
                                          std::vector<CmuxTreeJob>& jobs)
{
    return cmux_lanes_args(trgsw_slots, trlwe_slots, count, lanes, sel_stride, row_stride, jobs, nullptr,
        [&] { return cmux_tree_args(trgsw_slots, trlwe_slots, count, sel0, levels, first, out, jobs); },
        [&](LaneReach& m) {
            for (const CmuxTreeJob& j : jobs) m.sel((int64_t)j.sel0 + j.levels - 1), m.row(j.first), m.row((int64_t)j.first + (1 << j.levels) - 1), m.row(j.out);
        });
}

// iyk_hip_trlwe_add_batch
inline Refusal check_trlwe_add_batch(uint64_t trlwe_slots, uint64_t count, const int32_t* a, const int32_t* b, const int32_t* out,
                                     std::vector<TrlweAddJob>& jobs)
{
    if (count > MAX_ROW_BATCH) return invalid("batch too large");
    if (trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(a[g], trlwe_slots) || !slot_ok(b[g], trlwe_slots) || !slot_ok(out[g], trlwe_slots))
            return invalid("TRLWE index outside the buffer");
        jobs[g] = TrlweAddJob{a[g], b[g], out[g]};
    }
    const Clash c = find_clash(count, out, {a, b});
    if (c == CLASH_TWO_WRITERS) return invalid("two jobs of one batch write the same TRLWE row");
    if (c == CLASH_READ_OF_WRITTEN) return invalid("a job reads a TRLWE row that another job of the batch writes");
    return ACCEPT;
}

// ---- circuit bootstrapping and its parts ------------------------------------------------------------------------------------------

// iyk_hip_privks_batch.  k: iyk_params::k.  Rows are only written, so a second writer is the one clash there is.
inline Refusal check_privks_batch(uint32_t k, uint64_t tlwe2_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* in, const int32_t* c,
                                  const int32_t* out, std::vector<PrivksJob>& jobs)
{
    if (count > MAX_CB_BATCH) return invalid("batch too large");
    if (tlwe2_slots > MAX_STORE_ROWS || trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    const char* const two_writers = "two jobs of one batch write the same TRLWE row";
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(in[g], tlwe2_slots)) return bad_index_or_earlier_writers(g, out, "TLWE index outside the lvl2 store", two_writers);
        if (c[g] < 0 || c[g] > (int32_t)k) return bad_index_or_earlier_writers(g, out, "c outside [0, k]", two_writers);
        if (!slot_ok(out[g], trlwe_slots)) return bad_index_or_earlier_writers(g, out, "TRLWE index outside the buffer", two_writers);
        jobs[g] = PrivksJob{in[g], c[g], out[g]};
    }
    if (find_clash(count, out) == CLASH_TWO_WRITERS) return invalid(two_writers);
    return ACCEPT;
}

// iyk_hip_trgsw_from_rows: `rows` is what is uploaded, (k+1) l TRLWE rows per selector; nothing else is built
inline Refusal check_trgsw_from_rows(const iyk_params& p, uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* out_slot,
                                     const int32_t* rows)
{
    if (trgsw_slots > MAX_TRGSW_SLOTS || trlwe_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    if (count > trgsw_slots) return invalid("more selectors than the store has slots");
    const char* const two_writers = "two selectors of one call go to the same slot";
    const size_t per = (size_t)(p.k + 1) * p.l;
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(out_slot[g], trgsw_slots)) return bad_index_or_earlier_writers(g, out_slot, "selector index outside the selector store", two_writers);
        for (size_t r = 0; r < per; ++r)   // selector g's slot is looked at before its rows: g + 1
            if (!slot_ok(rows[g * per + r], trlwe_slots)) return bad_index_or_earlier_writers(g + 1, out_slot, "TRLWE index outside the buffer", two_writers);
    }
    if (find_clash(count, out_slot) == CLASH_TWO_WRITERS) return invalid(two_writers);
    return ACCEPT;
}

// iyk_hip_cb_rotate_batch
inline Refusal check_cb_rotate_batch(uint64_t tlwe0_slots, uint64_t tlwe2_slots, uint64_t count, const int32_t* in, const int32_t* sign,
                                     const uint32_t* off, const uint64_t* mu, const int32_t* out, std::vector<CbJob>& jobs)
{
    if (count > MAX_CB_BATCH) return invalid("batch too large");
    if (tlwe0_slots > MAX_STORE_ROWS || tlwe2_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    const char* const two_writers = "two jobs of one batch write the same lvl2 TLWE";
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(in[g], tlwe0_slots)) return bad_index_or_earlier_writers(g, out, "TLWE index outside the lvl0 store", two_writers);
        if (sign[g] != 1 && sign[g] != -1) return bad_index_or_earlier_writers(g, out, "sign outside {+1, -1}", two_writers);
        if (!slot_ok(out[g], tlwe2_slots)) return bad_index_or_earlier_writers(g, out, "TLWE index outside the lvl2 store", two_writers);
        jobs[g] = CbJob{in[g], sign[g], off[g], out[g], mu[g]};
    }
    if (find_clash(count, out) == CLASH_TWO_WRITERS) return invalid(two_writers);
    return ACCEPT;
}

// What iyk_hip_circuit_bootstrap_batch hands its three parts: lvl2 slot tlwe2_first + bit l + r, scratch row (bit (k+1) + c) l + r, selector
// slot trgsw_first + bit (the order of cmux.selectors_from_tlwe0)
struct CbLists {
    std::vector<CbJob> rot;         // bits * l rotations
    std::vector<PrivksJob> privks;  // bits * (k+1) l private key switches
    std::vector<int32_t> rows, sel; // iyk_hip_trgsw_from_rows: the scratch rows of every selector, its slot
};
// iyk_hip_circuit_bootstrap_batch: what only the combination can check, then the three parts' own builders on the expanded lists —
// whatever they check is checked before the first launch.  bk2_n, privks_n_in: of the two keys.  The batch cap and the store caps are
// restated ahead of the combination checks: the parts would report them too, but only after a wrong n or n_in.
inline Refusal check_circuit_bootstrap_batch(const iyk_params& p, uint32_t bk2_n, uint32_t privks_n_in, uint64_t tlwe0_slots, const int32_t* in,
                                             const int32_t* sign, uint32_t tlwe2_n_in, uint64_t tlwe2_slots, uint64_t tlwe2_first,
                                             uint64_t trlwe_slots, uint64_t trgsw_slots, uint64_t trgsw_first, uint64_t bits, CbLists& o)
{
    const uint64_t l = p.l, per = (uint64_t)(p.k + 1) * l;
    if (bits > MAX_CB_BATCH / per) return invalid("batch too large");
    if (tlwe0_slots > MAX_STORE_ROWS || tlwe2_slots > MAX_STORE_ROWS || trlwe_slots > MAX_STORE_ROWS || trgsw_slots > MAX_TRGSW_SLOTS)
        return invalid("store larger than an allocation can be");
    if (bk2_n != p.n) return invalid("the lvl2 bootstrapping key's n is not the initialised n of the lvl0 store's rows");
    if (tlwe2_n_in != CB_RING_N) return invalid("the lvl2 store's n_in is not the 2048 the rotation writes");
    if (tlwe2_n_in != privks_n_in) return invalid("the lvl2 store's n_in is not the private key-switching key's");
    if (tlwe2_first > tlwe2_slots || bits * l > tlwe2_slots - tlwe2_first) return invalid("bits * l lvl2 slots from the first do not fit the lvl2 store");
    if (trlwe_slots < bits * per) return invalid("the TRLWE scratch store has fewer than bits (k+1) l rows");
    if (trgsw_first > trgsw_slots || bits > trgsw_slots - trgsw_first) return invalid("selector slots outside the selector store");
    std::vector<int32_t> r_in(bits * l), r_sign(bits * l), r_out(bits * l), p_in(bits * per), p_c(bits * per);
    std::vector<uint32_t> r_off(bits * l, 0u);
    std::vector<uint64_t> r_mu(bits * l);
    o.rows.resize(bits * per);
    o.sel.resize(bits);
    for (uint64_t b = 0; b < bits; ++b) {
        o.sel[b] = (int32_t)(trgsw_first + b);
        for (uint64_t r = 0; r < l; ++r) {
            r_in[b * l + r] = in[b], r_sign[b * l + r] = sign[b];
            r_mu[b * l + r] = 1ull << (63 - (r + 1) * p.Bgbit);
            r_out[b * l + r] = (int32_t)(tlwe2_first + b * l + r);
        }
        for (uint64_t c = 0; c <= p.k; ++c)
            for (uint64_t r = 0; r < l; ++r) {
                const uint64_t row = b * per + c * l + r;
                p_in[row] = (int32_t)(tlwe2_first + b * l + r), p_c[row] = (int32_t)c, o.rows[row] = (int32_t)row;
            }
    }
    if (Refusal r = check_cb_rotate_batch(tlwe0_slots, tlwe2_slots, bits * l, r_in.data(), r_sign.data(), r_off.data(), r_mu.data(), r_out.data(), o.rot))
        return r;
    if (Refusal r = check_privks_batch(p.k, tlwe2_slots, trlwe_slots, bits * per, p_in.data(), p_c.data(), o.rows.data(), o.privks)) return r;
    return check_trgsw_from_rows(p, trgsw_slots, trlwe_slots, bits, o.sel.data(), o.rows.data());
}

// ---- the many-digit form of the lvl2 rotation: one job per bit, l outputs per job ----------------------------------

// the smallest bw with 2^bw >= l, for 1 <= l <= CB_MANY_MAX_L
constexpr uint32_t cb_many_bw(uint32_t l) { return l <= 1 ? 0u : l <= 2 ? 1u : 2u; }

// iyk_hip_cb_rotate_many_batch: job g writes lvl2 slots out[g] .. out[g] + l - 1.  shared: the kernel argument, mu[r] = 0 for r >= l.
// Named like cmux_rotate_chain_args and for its reason; tests/test_cb_many_cases.py holds every refusal of the two functions below.
inline Refusal cb_rotate_many_args(uint64_t tlwe0_slots, uint64_t tlwe2_slots, uint64_t count, const int32_t* in, const int32_t* sign,
                                          const uint32_t* off, uint32_t l, const uint64_t* mu, const int32_t* out, std::vector<CbManyJob>& jobs,
                                          CbManyMu& shared)
{
    if (count > MAX_CB_BATCH) return invalid("batch too large");
    if (tlwe0_slots > MAX_STORE_ROWS || tlwe2_slots > MAX_STORE_ROWS) return invalid("store larger than an allocation can be");
    if (l < 1 || l > CB_MANY_MAX_L) return invalid("l outside [1, 4]");
    jobs.resize(count);
    for (uint64_t g = 0; g < count; ++g) {
        if (!slot_ok(in[g], tlwe0_slots)) return invalid("TLWE index outside the lvl0 store");
        if (sign[g] != 1 && sign[g] != -1) return invalid("sign outside {+1, -1}");
        if (out[g] < 0 || (uint64_t)out[g] + l > tlwe2_slots) return invalid("l TLWEs from out do not fit the lvl2 store");
        jobs[g] = CbManyJob{in[g], sign[g], off[g], out[g]};
    }
    std::vector<int32_t> sorted(out, out + count);
    std::sort(sorted.begin(), sorted.end());
    for (uint64_t g = 1; g < count; ++g)
        if ((uint64_t)sorted[g] - (uint64_t)sorted[g - 1] < l) return invalid("two jobs of one batch write the same lvl2 TLWE");
    shared = CbManyMu{mu[0], l > 1 ? mu[1] : 0, l > 2 ? mu[2] : 0, l > 3 ? mu[3] : 0, l, cb_many_bw(l)};
    return ACCEPT;
}

// What iyk_hip_circuit_bootstrap_many_batch hands its three parts: CbLists' slots and rows, with one rotation per bit
struct CbManyLists {
    std::vector<CbManyJob> rot;     // bits rotations
    CbManyMu shared;
    std::vector<PrivksJob> privks;  // bits * (k+1) l private key switches
    std::vector<int32_t> rows, sel;
};
// iyk_hip_circuit_bootstrap_many_batch: check_circuit_bootstrap_batch's checks in its order, then the three parts' own builders
inline Refusal circuit_bootstrap_many_args(const iyk_params& p, uint32_t bk2_n, uint32_t privks_n_in, uint64_t tlwe0_slots, const int32_t* in,
                                                  const int32_t* sign, uint32_t tlwe2_n_in, uint64_t tlwe2_slots, uint64_t tlwe2_first,
                                                  uint64_t trlwe_slots, uint64_t trgsw_slots, uint64_t trgsw_first, uint64_t bits, CbManyLists& o)
{
    const uint64_t l = p.l, per = (uint64_t)(p.k + 1) * l;
    if (l < 1 || l > CB_MANY_MAX_L) return invalid("l outside [1, 4]");   // first: the cap below divides by per
    if (bits > MAX_CB_BATCH / per) return invalid("batch too large");
    if (tlwe0_slots > MAX_STORE_ROWS || tlwe2_slots > MAX_STORE_ROWS || trlwe_slots > MAX_STORE_ROWS || trgsw_slots > MAX_TRGSW_SLOTS)
        return invalid("store larger than an allocation can be");
    if (bk2_n != p.n) return invalid("the lvl2 bootstrapping key's n is not the initialised n of the lvl0 store's rows");
    if (tlwe2_n_in != CB_RING_N) return invalid("the lvl2 store's n_in is not the 2048 the rotation writes");
    if (tlwe2_n_in != privks_n_in) return invalid("the lvl2 store's n_in is not the private key-switching key's");
    if (tlwe2_first > tlwe2_slots || bits * l > tlwe2_slots - tlwe2_first) return invalid("bits * l lvl2 slots from the first do not fit the lvl2 store");
    if (trlwe_slots < bits * per) return invalid("the TRLWE scratch store has fewer than bits (k+1) l rows");
    if (trgsw_first > trgsw_slots || bits > trgsw_slots - trgsw_first) return invalid("selector slots outside the selector store");
    std::vector<int32_t> r_out(bits), p_in(bits * per), p_c(bits * per);
    std::vector<uint32_t> r_off(bits, 0u);
    uint64_t mu[CB_MANY_MAX_L] = {0, 0, 0, 0};
    for (uint64_t r = 0; r < l; ++r) mu[r] = 1ull << (63 - (r + 1) * p.Bgbit);
    o.rows.resize(bits * per);
    o.sel.resize(bits);
    for (uint64_t b = 0; b < bits; ++b) {
        o.sel[b] = (int32_t)(trgsw_first + b);
        r_out[b] = (int32_t)(tlwe2_first + b * l);
        for (uint64_t c = 0; c <= p.k; ++c)
            for (uint64_t r = 0; r < l; ++r) {
                const uint64_t row = b * per + c * l + r;
                p_in[row] = (int32_t)(tlwe2_first + b * l + r), p_c[row] = (int32_t)c, o.rows[row] = (int32_t)row;
            }
    }
    if (Refusal r = cb_rotate_many_args(tlwe0_slots, tlwe2_slots, bits, in, sign, r_off.data(), (uint32_t)l, mu, r_out.data(), o.rot, o.shared))
        return r;
    if (Refusal r = check_privks_batch(p.k, tlwe2_slots, trlwe_slots, bits * per, p_in.data(), p_c.data(), o.rows.data(), o.privks)) return r;
    return check_trgsw_from_rows(p, trgsw_slots, trlwe_slots, bits, o.sel.data(), o.rows.data());
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------

// iyk_hip_stream_wait_stream(st, other): st waits for what `other` holds now.  *_replica: iyk_hip_stream::gpu, the index into
// iyk_hip_init's device list; *_ordinal: the HIP device behind it (two replicas may share one) — the caller reads both from non-null
// handles only and passes anything for a null one.  Replicas are told apart even on one device: a replica's stores, keys and transform
// constants are its own, and nothing one replica enqueues reads another's.  Not named check_*, for cmux_rotate_chain_args' reason;
// tests/test_cmux_stage_cb.py holds every refusal below.
inline Refusal stream_wait_args(const void* st, const void* other, int st_replica, int other_replica, int st_ordinal, int other_ordinal)
{
    if (!st || !other) return invalid("null stream");
    if (st == other) return invalid("a stream cannot wait for itself");
    if (st_ordinal != other_ordinal) return invalid("the two streams are on different GPUs");
    if (st_replica != other_replica) return invalid("the two streams belong to different replicas");
    return ACCEPT;
}

// ---- seeded key windows -------------------------------------------------------------------------------------------------------------

// iyk_hip_privks_key_upload_seeded / iyk_hip_bk2_key_upload_seeded: a window [first, first + count) of a key of key_units rows (private
// key) or steps (lvl2 key), its mask seed and its b halves.  *_replica / *_ordinal: as stream_wait_args, read from non-null handles
// only.  An empty window is refused: a seeded call always launches the expansion, and a launch of no lanes is no launch.  The largest
// legal window is the whole key.  Not named check_*, for cmux_rotate_chain_args' reason; tests/test_key_expand.py holds every refusal.
inline Refusal key_upload_seeded_args(const void* st, const void* key, const void* mask_seed, const void* host_b, int st_replica,
                                      int key_replica, int st_ordinal, int key_ordinal, uint64_t key_units, uint64_t first, uint64_t count)
{
    if (!st || !key || !mask_seed || !host_b) return invalid("null argument");
    if (st_ordinal != key_ordinal) return invalid("the stream and the key are on different GPUs");
    if (st_replica != key_replica) return invalid("the stream and the key belong to different replicas");
    if (count == 0) return invalid("empty window");
    if (first > key_units || count > key_units - first) return invalid("window outside the key");
    return ACCEPT;
}

}  // namespace args
}  // namespace iyk
