// rt_fast_timing.hip -- timing variants of the production kernel (rt_render.h RT_FAMILY_TIMING; TIMING_BIT: phase
// clocks, per-pixel work for rt_lane_plan, per-wave clock records): 25 (= 17 + timing), 29 (= 21 + timing), 9 (no
// split), and the lean 25 | 128 (rt_variant.h LEAN_BIT), so that the lane-cost probe and the timing frame of a knob-free
// frame describe the kernel that renders it (rt_fast_lean.hip).
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_TIMING)

}  // namespace rtk
