// lane_jobs.hpp — K request packets of one circuit in one batch: the job lists of ONE lane, expanded on the device to those of all.
//
// A lane is one copy of a circuit's arena image; K lanes live in one arena, lane r in slots [r * lane_stride, (r + 1) * lane_stride).
// iyk_hip_gate_batch_lanes stages the RotJob / KsJob / EwJob lists of ONE lane — what batch_args.hpp builds from the caller's
// descriptors, every index inside [0, lane_stride) — and lane_jobs_kernel writes the lists of all lanes into a scratch of the stream:
//   lane-major: output job r * n + j is lane r's copy of job j of a list of n;
//   arena slots (RotJob::ia / ib, KsJob::out, EwJob::in / out) get + r * lane_stride, rotation rows (KsJob::ra / rb) + r * nrot — lane
//   r's rotations are rows r * nrot .. of the stream's rotation buffer, as the lane-major rotation list puts them;
//   a negative index ("none": ib, rb, the in of a constant) stays what it is.
// The rotation and key-switch kernels then run the expanded lists as ONE batch of count x lanes jobs: they are not changed.
//
// The arithmetic of an output job is lane_rot_job / lane_ks_job / lane_ew_job below and which job an output index is lane_write_job:
// __host__ __device__, so that the kernel and the emulation library (lane_emul.hpp, tests/test_lane_jobs.py) run the same functions.
// Nothing overflows: gate_batch_lanes_args (batch_args.hpp) has refused lanes * lane_stride > 2^31 and nrot * lanes > 2^31 - 1.
#pragma once
#include <stdint.h>

#include "jobs.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IYK_LANE_HD __host__ __device__ inline
#else
#define IYK_LANE_HD inline
#endif

namespace iyk {

// index `i` of one lane -> the same index of lane r, `per_lane` apart; negative: none
IYK_LANE_HD int32_t lane_index(int32_t i, uint32_t r, uint32_t per_lane) { return i < 0 ? i : (int32_t)((uint32_t)i + r * per_lane); }

IYK_LANE_HD RotJob lane_rot_job(const RotJob& j, uint32_t r, uint32_t lane_stride)
{
    return RotJob{lane_index(j.ia, r, lane_stride), lane_index(j.ib, r, lane_stride), j.sa, j.sb, j.off};
}
IYK_LANE_HD KsJob lane_ks_job(const KsJob& j, uint32_t r, uint32_t lane_stride, uint32_t nrot)
{
    return KsJob{lane_index(j.ra, r, nrot), lane_index(j.rb, r, nrot), j.off, lane_index(j.out, r, lane_stride)};
}
IYK_LANE_HD EwJob lane_ew_job(const EwJob& j, uint32_t r, uint32_t lane_stride)
{
    return EwJob{j.op, lane_index(j.in, r, lane_stride), lane_index(j.out, r, lane_stride)};
}

// One expansion: the lists of one lane (rot1 / ks1 / ew1, nrot / nks / new_ jobs) and where the lists of all lanes go.
struct LaneLists {
    const RotJob* rot1;
    const KsJob* ks1;
    const EwJob* ew1;
    RotJob* rot;   // nrot * lanes
    KsJob* ks;     // nks * lanes
    EwJob* ew;     // new_ * lanes
    uint32_t nrot, nks, new_, lanes, lane_stride;
};
IYK_LANE_HD uint64_t lane_jobs_total(const LaneLists& L) { return ((uint64_t)L.nrot + L.nks + L.new_) * L.lanes; }
// Output job i of the three expanded lists, counted one list after the other: rotations, key switches, elementwise jobs.
IYK_LANE_HD void lane_write_job(const LaneLists& L, uint64_t i)
{
    const uint64_t rots = (uint64_t)L.nrot * L.lanes, kss = (uint64_t)L.nks * L.lanes;
    if (i < rots) {
        const uint32_t r = (uint32_t)(i / L.nrot), j = (uint32_t)(i % L.nrot);
        L.rot[i] = lane_rot_job(L.rot1[j], r, L.lane_stride);
    }
    else if (i < rots + kss) {
        const uint64_t k = i - rots;
        const uint32_t r = (uint32_t)(k / L.nks), j = (uint32_t)(k % L.nks);
        L.ks[k] = lane_ks_job(L.ks1[j], r, L.lane_stride, L.nrot);
    }
    else {
        const uint64_t k = i - rots - kss;
        const uint32_t r = (uint32_t)(k / L.new_), j = (uint32_t)(k % L.new_);
        L.ew[k] = lane_ew_job(L.ew1[j], r, L.lane_stride);
    }
}

// Where the three expanded lists start in one allocation (each 16-byte aligned), and its size
struct LaneScratch {
    size_t ks_off, ew_off, bytes;
};
inline LaneScratch lane_scratch(uint64_t nrot, uint64_t nks, uint64_t new_, uint64_t lanes)
{
    LaneScratch s{};
    s.ks_off = (size_t)((nrot * lanes * sizeof(RotJob) + 15) & ~(uint64_t)15);
    s.ew_off = (size_t)((s.ks_off + nks * lanes * sizeof(KsJob) + 15) & ~(uint64_t)15);
    s.bytes = s.ew_off + (size_t)(new_ * lanes * sizeof(EwJob));
    return s;
}

#if defined(__HIPCC__)
constexpr int LANE_JOBS_THREADS = 256;
constexpr unsigned LANE_JOBS_MAX_GRID = 1024;   // wider expansions go round the grid-stride loop
// one thread per output job
__global__ __launch_bounds__(LANE_JOBS_THREADS) void lane_jobs_kernel(const LaneLists L)
{
    const uint64_t total = lane_jobs_total(L), step = (uint64_t)gridDim.x * LANE_JOBS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * LANE_JOBS_THREADS + threadIdx.x; i < total; i += step) lane_write_job(L, i);
}
inline unsigned lane_jobs_grid(uint64_t total)
{
    const uint64_t blocks = (total + LANE_JOBS_THREADS - 1) / LANE_JOBS_THREADS;
    return (unsigned)(blocks < LANE_JOBS_MAX_GRID ? (blocks ? blocks : 1) : LANE_JOBS_MAX_GRID);
}
#endif

}  // namespace iyk
