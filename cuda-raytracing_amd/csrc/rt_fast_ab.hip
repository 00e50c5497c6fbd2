// rt_fast_ab.hip -- A/B variants behind RT_TUNE bit 12 (tools/; rt_render.h RT_FAMILY_AB): MODE_NOSPLIT = 1 (no split
// small steps) and 5 (the same with leaf trees).  The big-leaf mode A/B variants are in rt_fast_ab2.hip.
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_AB)

}  // namespace rtk
