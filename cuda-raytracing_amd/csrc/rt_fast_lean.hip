// rt_fast_lean.hip -- the fixed-policy ("lean") production variant (rt_render.h RT_FAMILY_LEAN): MODE_PROD | LEAN_BIT =
// 17 | 128 (rt_variant.h), the MODE 17 kernel of rt_fast_prod.hip with RT_TUNE compiled in as 0, without the
// fallbacks for a missing mirror array, and with the arguments used only around the traversal read where they are
// used (rt_fast_body.h arg), built for 5, 6 and 7 waves per SIMD.  choose_variant sends a frame here when it sets no
// knob the kernel reads and the scene's mirror holds every array the variant assumes -- the frames bench.py times
// (config 2 runs render_fast_kernel_w7<30, false, 145>); every other frame renders through rt_fast_prod.hip.
// Scenes with leaf trees stay on the general MODE 21: its lean form was built and measured slower (config 4
// 93.7 vs 80.0 ms: without the scalars the 7-wave build spills 264 vector dwords instead of 210;
// profiles/lean_ab.txt).  A unit of its own, so the families still compile in parallel.
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_LEAN)

}  // namespace rtk
