/* iyokan_level_cost.h — what a level of blind rotations costs, as pure functions of an iyk_level_cost table.
 *
 * iyk_hip_gate_batch's rotation dispatch (iyokan_amd/csrc/dispatch.hpp: rot_split) prices a level this way, and every planner
 * that chooses batch sizes (iyokan_amd/host/iyokan_hip.hpp: planFrontiers; iyokan_amd/frontier.py restates the two functions
 * in Python, pinned to these by tests/test_netlist.py) calls THESE — the one C / C++ copy.  No state, no library call: usable
 * without linking libiyokan_hip.so. */
#ifndef IYOKAN_LEVEL_COST_H
#define IYOKAN_LEVEL_COST_H

#include "iyokan_hip.h"

/* Milliseconds of `rot` rotations on one GPU: full rounds on the wave-per-rotation kernel, a remainder of up to
 * max_passes * pass rotations in passes of the narrow-frontier kernel, a larger remainder as one more round. */
static inline double iyk_level_cost_ms(const iyk_level_cost* c, long rot)
{
    if (rot <= 0) return 0.0;
    const long full = rot / c->round, rem = rot % c->round;
    const double t = (double)c->round_ms * (double)full;
    if (rem == 0) return t;
    if (rem <= (long)c->max_passes * c->pass) return t + c->pass_ms[(rem + c->pass - 1) / c->pass - 1];
    return t + c->round_ms;
}

/* What ONE pass of the narrow-frontier kernel costs by how much of it is filled, per quarter, relative to a full pass: up to a
 * quarter of the CUs busy it runs at the part's full clock, with all of them busy into the power limit (2.466 / 2.497 / 2.554 /
 * 2.635 ms at 64 / 128 / 192 / 256 rotations, profiles/r06_plan_ab.txt). */
static const double IYK_SUB_PASS_SHAPE[4] = {0.936, 0.947, 0.969, 1.0};

/* What plans are COMPARED by: iyk_level_cost_ms with the first pass priced by how full it is. */
static inline double iyk_level_price_ms(const iyk_level_cost* c, long rot)
{
    if (rot > 0 && rot <= c->pass) {
        const long q = (4 * rot - 1) / c->pass;
        return iyk_level_cost_ms(c, c->pass) * IYK_SUB_PASS_SHAPE[q < 3 ? q : 3];
    }
    return iyk_level_cost_ms(c, rot);
}

#endif /* IYOKAN_LEVEL_COST_H */
