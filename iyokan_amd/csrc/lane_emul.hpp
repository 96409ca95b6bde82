// lane_emul.hpp — TEST SUPPORT: the lane batch of iyk_hip_gate_batch_lanes on the CPU, exported by libiyk_emul.so (emul.cpp includes this
// file; nothing of the product does).  On its own so that tests/test_lane_jobs.py can also build it alone, in seconds, from copies of
// lane_jobs.hpp with one edit each: the mutants its cases must tell from the real thing.
//
//   iyk_emul_gate_batch_lanes_args   batch_args.hpp's gate_batch_lanes_args: the refusal's code and text; accepted, the lists of ONE lane
//                                    as 32-bit words (rotations, key switches, elementwise jobs) and the three counts
//   iyk_emul_lane_jobs               lane_jobs_kernel's loop over lane_write_job, thread by thread: the lists of all lanes from those words
//   iyk_emul_lane_dispatch           what the expanded batch launches: dispatch.hpp on the TOTAL rotation / key-switch counts
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "batch_args.hpp"
#include "dispatch.hpp"
#include "lane_jobs.hpp"

extern "C" {

int iyk_emul_gate_batch_lanes_args(const iyk_params* p, int debug, uint64_t arena_slots, uint64_t count, const int32_t* ops, const int32_t* in0,
                                   const int32_t* in1, const int32_t* in2, const int32_t* out, uint64_t lanes, uint64_t lane_stride, char* msg,
                                   uint64_t msg_cap, uint32_t* words, uint64_t words_cap, uint64_t* counts /* [4]: the last one 1 if a refusal left a list non-empty */)
{
    using namespace iyk;
    std::vector<RotJob> rot;
    std::vector<KsJob> ks;
    std::vector<EwJob> ew;
    const args::Refusal r = args::gate_batch_lanes_args(*p, debug != 0, arena_slots, count, ops, in0, in1, in2, out, lanes, lane_stride, rot, ks, ew);
    std::snprintf(msg, (size_t)msg_cap, "%s", r.text ? r.text : "");
    counts[0] = rot.size(), counts[1] = ks.size(), counts[2] = ew.size();
    counts[3] = r && (rot.size() || ks.size() || ew.size());
    const uint64_t need = rot.size() * 5 + ks.size() * 4 + ew.size() * 3;
    if (!r && need <= words_cap) {
        if (!rot.empty()) std::memcpy(words, rot.data(), rot.size() * sizeof(RotJob));
        if (!ks.empty()) std::memcpy(words + rot.size() * 5, ks.data(), ks.size() * sizeof(KsJob));
        if (!ew.empty()) std::memcpy(words + rot.size() * 5 + ks.size() * 4, ew.data(), ew.size() * sizeof(EwJob));
    }
    return r.code;
}

// words1: one lane's lists as above, counts1 = {nrot, nks, new}; words_out: (5 nrot + 4 nks + 3 new) * lanes words, the expanded lists
// one after the other.  `threads` > 0: the kernel's traversal with that many threads in all, each going round its grid-stride loop.
int iyk_emul_lane_jobs(const uint32_t* words1, const uint64_t* counts1, uint64_t lanes, uint64_t lane_stride, uint64_t threads, uint32_t* words_out)
{
    using namespace iyk;
    const uint64_t nrot = counts1[0], nks = counts1[1], new_ = counts1[2];
    std::vector<RotJob> rot1(nrot), rot(nrot * lanes);
    std::vector<KsJob> ks1(nks), ks(nks * lanes);
    std::vector<EwJob> ew1(new_), ew(new_ * lanes);
    if (nrot) std::memcpy(rot1.data(), words1, nrot * sizeof(RotJob));
    if (nks) std::memcpy(ks1.data(), words1 + nrot * 5, nks * sizeof(KsJob));
    if (new_) std::memcpy(ew1.data(), words1 + nrot * 5 + nks * 4, new_ * sizeof(EwJob));
    const LaneLists L{rot1.data(), ks1.data(), ew1.data(), rot.data(), ks.data(), ew.data(), (uint32_t)nrot, (uint32_t)nks, (uint32_t)new_,
                      (uint32_t)lanes, (uint32_t)lane_stride};
    const uint64_t total = lane_jobs_total(L);
    if (threads == 0) threads = 1;
    for (uint64_t t = 0; t < threads; ++t)
        for (uint64_t i = t; i < total; i += threads) lane_write_job(L, i);
    uint32_t* w = words_out;
    if (!rot.empty()) std::memcpy(w, rot.data(), rot.size() * sizeof(RotJob));
    w += rot.size() * 5;
    if (!ks.empty()) std::memcpy(w, ks.data(), ks.size() * sizeof(KsJob));
    w += ks.size() * 4;
    if (!ew.empty()) std::memcpy(w, ew.data(), ew.size() * sizeof(EwJob));
    return 0;
}

// out[0 .. 4]: rot_split of nrot x lanes rotations; out[5 .. 8]: ks_plan of nks x lanes key switches; out[9]: ks_matrix_form of them
void iyk_emul_lane_dispatch(uint64_t nrot, uint64_t nks, uint64_t lanes, int round, int pass_cus, int max_passes, int forced, int kind, int shared_max,
                            int shared_wg, int kind_env, int T, int nc, int cus, int out[10])
{
    using namespace iyk::dispatch;
    const RotSplit s = rot_split((int)(nrot * lanes), round, pass_cus, max_passes, forced);
    out[0] = s.family, out[1] = s.tp_first, out[2] = s.tp_count, out[3] = s.narrow_first, out[4] = s.narrow_count;
    const KsPlan k = ks_plan(kind, shared_max, shared_wg, (int)(nks * lanes), T, nc, cus);
    out[5] = k.form, out[6] = k.groups, out[7] = k.slices, out[8] = k.i_per_slice;
    out[9] = ks_matrix_form(kind_env, (int)(nks * lanes), T, nc) ? 1 : 0;
}

}  // extern "C"
