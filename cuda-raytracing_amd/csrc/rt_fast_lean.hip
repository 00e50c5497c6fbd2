// rt_fast_lean.hip -- the fixed-policy ("lean") production variant: MODE 17 | 128 (rt_fast.h LEAN_BIT), the
// MODE 17 kernel of rt_fast_prod.hip with RT_TUNE compiled in as 0, without the fallbacks for a missing mirror
// array, and with the arguments used only around the traversal read where they are used (rt_fast_body.h arg),
// built for 5, 6 and 7 waves per SIMD.  rt_kernel.hip launch_fast sends a frame here when it sets no knob the
// kernel reads and the scene's mirror holds every array the variant assumes -- the frames bench.py times
// (config 2 runs render_fast_kernel_w7<30, false, 145>); every other frame renders through rt_fast_prod.hip.
// Scenes with leaf trees stay on the general MODE 21: its lean form was built and measured slower (config 4
// 93.7 vs 80.0 ms: without the scalars the 7-wave build spills 264 vector dwords instead of 210;
// profiles/lean_ab.txt).  A unit of its own, so the families still compile in parallel.
#include "rt_fast_body.h"

namespace rtk {
namespace {
template <int STACK>
hipError_t dispatch(int mode, const RenderArgs& a, int waves, hipStream_t s) {
    switch (mode) {
        case 17 | rtfast::LEAN_BIT: return launch_occ<STACK, false, 17 | rtfast::LEAN_BIT>(a, waves, s);
    }
    return hipErrorInvalidValue;
}
}  // namespace

RT_FAST_FAMILY(launch_fast_lean, dispatch)

}  // namespace rtk
