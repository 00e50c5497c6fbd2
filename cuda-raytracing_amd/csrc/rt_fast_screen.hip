// rt_fast_screen.hip -- big-leaf screen variants (rt_render.h RT_FAMILY_SCREEN; SCREEN_BIT; rt_fast.h screen_leaf,
// mirror.h pf = 3): 49 / 53 (= 17 / 21 + screens), 57 / 61 (their timing variants).  Exact, and measured slower on the
// one BASELINE scene that has screenable leaves (config 4: 85.2-85.4 vs 82.5-82.9 ms), so
// they live in librt_hip_exp.so and the mirror builds screen records only when rt_build_options
// leaf_screens asks for them.
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_SCREEN)

}  // namespace rtk
