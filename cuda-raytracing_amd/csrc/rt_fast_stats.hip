// rt_fast_stats.hip -- statistics variants (exact counts of the reference's traversal work on scalar
// records; rt_render.h RT_FAMILY_STATS): MODE BIG_SCALAR = 2, and 6 (| TREE_BIT) through the leaf trees.
#include "rt_fast_body.h"

namespace rtk {

RT_APPLY(RT_FAST_FAMILY, RT_FAMILY_STATS)

}  // namespace rtk
