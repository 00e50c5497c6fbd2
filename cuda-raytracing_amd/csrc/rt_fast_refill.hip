// rt_fast_refill.hip -- refill variants (rt_render_params.refill_lanes: lanes take new pixels from a
// queue; measured slower, opt-in; rt_render.h RT_FAMILY_REFILL): MODE_PROD | REFILL_BIT = 81, and 85 with leaf trees.
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_REFILL)

}  // namespace rtk
