// cmux_lane_emul.hpp — TEST SUPPORT: the lane batches of iyk_hip_cmux_*_batch_lanes on the CPU, exported by libiyk_emul.so (emul.cpp
// includes this file; nothing of the product does).  On its own, like lane_emul.hpp, so that tests/test_cmux_lane_jobs.py can also build it
// alone from copies of cmux_lane_jobs.hpp with one edit each: the mutants its cases must tell from the real thing.
//
// family: 0 CmuxJob (a = sel, in0, in1, rot, out), 1 CmuxChainJob (sel0, steps, pattern, src, mem, out), 2 CmuxRotChainJob + CmuxRotStep
// (steps, sel, rot, src, out), 3 CmuxTreeJob (sel0, levels, first, out).
//   iyk_emul_cmux_lanes_args   batch_args.hpp's *_lanes_args: the refusal's code and text; accepted, the list(s) of ONE lane as 32-bit
//                              words (jobs, then steps) and the two counts
//   iyk_emul_cmux_lane_jobs    cmux_lane_jobs_kernel's loop over lane_write_cmux, thread by thread: the lists of all lanes from those words
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "batch_args.hpp"
#include "cmux_lane_jobs.hpp"

namespace iyk {
namespace cmux_lane_emul {

template <class Job>
int expand(const uint32_t* words1, uint64_t n, uint64_t nsteps, uint64_t lanes, uint64_t sel_stride, uint64_t row_stride, uint64_t threads,
           uint32_t* words_out)
{
    constexpr size_t W = sizeof(Job) / 4;
    std::vector<Job> job1(n), job(n * lanes);
    std::vector<CmuxRotStep> step1(nsteps), step(nsteps * lanes);
    if (n) std::memcpy(job1.data(), words1, n * sizeof(Job));
    if (nsteps) std::memcpy(step1.data(), words1 + n * W, nsteps * sizeof(CmuxRotStep));
    const CmuxLaneLists<Job> L{job1.data(), step1.data(), job.data(), step.data(), (uint32_t)n, (uint32_t)nsteps, (uint32_t)lanes,
                               (uint32_t)sel_stride, (uint32_t)row_stride};
    const uint64_t total = lane_cmux_total(L);
    if (threads == 0) threads = 1;
    for (uint64_t t = 0; t < threads; ++t)
        for (uint64_t i = t; i < total; i += threads) lane_write_cmux(L, i);
    if (!job.empty()) std::memcpy(words_out, job.data(), job.size() * sizeof(Job));
    if (!step.empty()) std::memcpy(words_out + job.size() * W, step.data(), step.size() * sizeof(CmuxRotStep));
    return 0;
}

}  // namespace cmux_lane_emul
}  // namespace iyk

extern "C" {

int iyk_emul_cmux_lanes_args(int family, uint64_t trgsw_slots, uint64_t trlwe_slots, uint64_t count, const int32_t* a0, const int32_t* a1,
                             const int32_t* a2, const int32_t* a3, const int32_t* a4, const int32_t* a5, uint64_t lanes, uint64_t sel_stride,
                             uint64_t row_stride, char* msg, uint64_t msg_cap, uint32_t* words, uint64_t words_cap,
                             uint64_t* counts /* [3]: jobs, steps, 1 if a refusal left a list non-empty */)
{
    using namespace iyk;
    std::vector<CmuxJob> cm;
    std::vector<CmuxChainJob> ch;
    std::vector<CmuxRotChainJob> rc;
    std::vector<CmuxRotStep> st;
    std::vector<CmuxTreeJob> tr;
    args::Refusal r = args::invalid("unknown family");
    const void* data = nullptr;
    size_t n = 0, w = 0;
    switch (family) {
    case 0:
        r = args::cmux_batch_lanes_args(trgsw_slots, trlwe_slots, count, a0, a1, a2, a3, a4, lanes, sel_stride, row_stride, cm);
        data = cm.data(), n = cm.size(), w = sizeof(CmuxJob) / 4;
        break;
    case 1:
        r = args::cmux_chain_batch_lanes_args(trgsw_slots, trlwe_slots, count, a0, a1, (const uint32_t*)a2, a3, a4, a5, lanes, sel_stride, row_stride, ch);
        data = ch.data(), n = ch.size(), w = sizeof(CmuxChainJob) / 4;
        break;
    case 2:
        r = args::cmux_rotate_chain_batch_lanes_args(trgsw_slots, trlwe_slots, count, a0, a1, a2, a3, a4, lanes, sel_stride, row_stride, rc, st);
        data = rc.data(), n = rc.size(), w = sizeof(CmuxRotChainJob) / 4;
        break;
    case 3:
        r = args::cmux_tree_batch_lanes_args(trgsw_slots, trlwe_slots, count, a0, a1, a2, a3, lanes, sel_stride, row_stride, tr);
        data = tr.data(), n = tr.size(), w = sizeof(CmuxTreeJob) / 4;
        break;
    default: break;
    }
    std::snprintf(msg, (size_t)msg_cap, "%s", r.text ? r.text : "");
    counts[0] = n, counts[1] = st.size();
    counts[2] = r && (n || st.size());
    if (!r && n * w + st.size() * 2 <= words_cap) {
        if (n) std::memcpy(words, data, n * w * 4);
        if (!st.empty()) std::memcpy(words + n * w, st.data(), st.size() * sizeof(CmuxRotStep));
    }
    return r.code;
}

// words1: one lane's list(s) as above, counts1 = {jobs, steps}; words_out: (W jobs + 2 steps) * lanes words, the expanded jobs and then the
// expanded steps.  `threads` > 0: the kernel's traversal with that many threads in all, each going round its grid-stride loop.
int iyk_emul_cmux_lane_jobs(int family, const uint32_t* words1, const uint64_t* counts1, uint64_t lanes, uint64_t sel_stride, uint64_t row_stride,
                            uint64_t threads, uint32_t* words_out)
{
    using namespace iyk;
    using namespace iyk::cmux_lane_emul;
    const uint64_t n = counts1[0], ns = counts1[1];
    switch (family) {
    case 0: return expand<CmuxJob>(words1, n, 0, lanes, sel_stride, row_stride, threads, words_out);
    case 1: return expand<CmuxChainJob>(words1, n, 0, lanes, sel_stride, row_stride, threads, words_out);
    case 2: return expand<CmuxRotChainJob>(words1, n, ns, lanes, sel_stride, row_stride, threads, words_out);
    case 3: return expand<CmuxTreeJob>(words1, n, 0, lanes, sel_stride, row_stride, threads, words_out);
    default: return -1;
    }
}

}  // extern "C"
