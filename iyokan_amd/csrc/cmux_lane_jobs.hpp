// cmux_lane_jobs.hpp — CMUX memories per lane: the CMUX job lists of ONE lane's memory, expanded on the device to those of all lanes.
//
// A laned memory is K copies of the one-lane memory at fixed strides: lane r owns TRLWE rows [r * row_stride, (r + 1) * row_stride) and
// its selector slots are lane 0's + r * sel_stride (sel_stride is a parameter of the memory: under stage_cb it is the stage's bit count,
// which may be smaller than a port's selector base — lanes interleave inside a stage).  The iyk_hip_cmux_*_batch_lanes entry points
// stage the CmuxJob / CmuxChainJob / CmuxRotChainJob (+ CmuxRotStep) / CmuxTreeJob list of ONE lane — what batch_args.hpp builds from the
// caller's arrays — and cmux_lane_jobs_kernel writes the lists of all lanes into the stream's lane scratch:
//   lane-major: output job r * n + j is lane r's copy of job j of a list of n;
//   selector slots get + r * sel_stride, TRLWE rows + r * row_stride, a rotate chain's `first` + r * nsteps (lane r's steps are entries
//   r * nsteps .. of the expanded step list, nsteps the steps of one lane); rot, steps, pattern and levels stay what they are;
//   a negative index (the in1 of a rotate-form CmuxJob) stays what it is.
// cmux_fft_kernel / cmux_chain_kernel / cmux_rotate_chain_kernel / cmux_tree_kernel then run the expanded list as ONE batch of count x
// lanes jobs: they are not changed.
//
// The arithmetic of an output job is lane_cmux_* below and which job an output index is lane_write_cmux: __host__ __device__, so that the
// kernel and the emulation library (cmux_lane_emul.hpp, tests/test_cmux_lane_jobs.py) run the same functions.
// Nothing overflows: the *_lanes_args checks (batch_args.hpp) have refused an offset index >= 2^31 and nsteps * lanes > 2^31 - 1.
#pragma once
#include <stdint.h>

#include "jobs.hpp"
#include "lane_jobs.hpp"

namespace iyk {

IYK_LANE_HD CmuxJob lane_cmux_job(const CmuxJob& j, uint32_t r, uint32_t sel_stride, uint32_t row_stride)
{
    return CmuxJob{lane_index(j.sel, r, sel_stride), lane_index(j.in0, r, row_stride), lane_index(j.in1, r, row_stride), j.rot,
                   lane_index(j.out, r, row_stride)};
}
IYK_LANE_HD CmuxChainJob lane_cmux_chain_job(const CmuxChainJob& j, uint32_t r, uint32_t sel_stride, uint32_t row_stride)
{
    return CmuxChainJob{lane_index(j.sel0, r, sel_stride), j.steps, j.pattern, lane_index(j.src, r, row_stride), lane_index(j.mem, r, row_stride),
                        lane_index(j.out, r, row_stride)};
}
IYK_LANE_HD CmuxTreeJob lane_cmux_tree_job(const CmuxTreeJob& j, uint32_t r, uint32_t sel_stride, uint32_t row_stride)
{
    return CmuxTreeJob{lane_index(j.sel0, r, sel_stride), j.levels, lane_index(j.first, r, row_stride), lane_index(j.out, r, row_stride)};
}
IYK_LANE_HD CmuxRotChainJob lane_cmux_rot_chain_job(const CmuxRotChainJob& j, uint32_t r, uint32_t nsteps, uint32_t row_stride)
{
    return CmuxRotChainJob{lane_index(j.first, r, nsteps), j.steps, lane_index(j.src, r, row_stride), lane_index(j.out, r, row_stride)};
}
IYK_LANE_HD CmuxRotStep lane_cmux_rot_step(const CmuxRotStep& s, uint32_t r, uint32_t sel_stride)
{
    return CmuxRotStep{lane_index(s.sel, r, sel_stride), s.rot};
}

// One expansion: the list of one lane (job1, n jobs; for a rotate chain also step1, nsteps steps) and where the lists of all lanes go.
template <class Job>
struct CmuxLaneLists {
    const Job* job1;
    const CmuxRotStep* step1;   // rotate chain only
    Job* job;                   // n * lanes
    CmuxRotStep* step;          // nsteps * lanes
    uint32_t n, nsteps, lanes, sel_stride, row_stride;
};
template <class Job>
IYK_LANE_HD uint64_t lane_cmux_total(const CmuxLaneLists<Job>& L)
{
    return ((uint64_t)L.n + L.nsteps) * L.lanes;
}

IYK_LANE_HD CmuxJob lane_cmux_any(const CmuxLaneLists<CmuxJob>& L, uint32_t j, uint32_t r) { return lane_cmux_job(L.job1[j], r, L.sel_stride, L.row_stride); }
IYK_LANE_HD CmuxChainJob lane_cmux_any(const CmuxLaneLists<CmuxChainJob>& L, uint32_t j, uint32_t r)
{
    return lane_cmux_chain_job(L.job1[j], r, L.sel_stride, L.row_stride);
}
IYK_LANE_HD CmuxTreeJob lane_cmux_any(const CmuxLaneLists<CmuxTreeJob>& L, uint32_t j, uint32_t r)
{
    return lane_cmux_tree_job(L.job1[j], r, L.sel_stride, L.row_stride);
}
IYK_LANE_HD CmuxRotChainJob lane_cmux_any(const CmuxLaneLists<CmuxRotChainJob>& L, uint32_t j, uint32_t r)
{
    return lane_cmux_rot_chain_job(L.job1[j], r, L.nsteps, L.row_stride);
}

// Output entry i of the expanded lists, counted one list after the other: the jobs, then (rotate chain) the steps.
template <class Job>
IYK_LANE_HD void lane_write_cmux(const CmuxLaneLists<Job>& L, uint64_t i)
{
    const uint64_t jobs = (uint64_t)L.n * L.lanes;
    if (i < jobs) {
        const uint32_t r = (uint32_t)(i / L.n), j = (uint32_t)(i % L.n);
        L.job[i] = lane_cmux_any(L, j, r);
    }
    else {
        const uint64_t k = i - jobs;
        const uint32_t r = (uint32_t)(k / L.nsteps), j = (uint32_t)(k % L.nsteps);
        L.step[k] = lane_cmux_rot_step(L.step1[j], r, L.sel_stride);
    }
}

// Where the expanded step list starts behind the expanded jobs in one allocation (16-byte aligned), and the allocation's size
struct CmuxLaneScratch {
    size_t step_off, bytes;
};
inline CmuxLaneScratch cmux_lane_scratch(uint64_t n, size_t job_bytes, uint64_t nsteps, uint64_t lanes)
{
    CmuxLaneScratch s{};
    s.step_off = (size_t)((n * lanes * job_bytes + 15) & ~(uint64_t)15);
    s.bytes = s.step_off + (size_t)(nsteps * lanes * sizeof(CmuxRotStep));
    return s;
}

#if defined(__HIPCC__)
// one thread per output entry; jobs and steps of a rotate chain in ONE launch
template <class Job>
__global__ __launch_bounds__(LANE_JOBS_THREADS) void cmux_lane_jobs_kernel(const CmuxLaneLists<Job> L)
{
    const uint64_t total = lane_cmux_total(L), step = (uint64_t)gridDim.x * LANE_JOBS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * LANE_JOBS_THREADS + threadIdx.x; i < total; i += step) lane_write_cmux(L, i);
}
#endif

}  // namespace iyk
