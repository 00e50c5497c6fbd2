// rt_fast_ab2.hip -- A/B variants behind RT_TUNE bits 4-5 (tools/; rt_render.h RT_FAMILY_AB2): big leaves BIG_SCALAR = 2
// (scalar records only) and BIG_PAIRS = 0 (pair records in every big-leaf mode).
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_AB2)

}  // namespace rtk
