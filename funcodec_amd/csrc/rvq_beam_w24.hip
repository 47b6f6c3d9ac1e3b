// rvq_beam_kernel<D, 2> and <D, 4> for every row width (rvq_beam_kernel.h): the twelve together compile in seconds.
#include "rvq_beam_kernel.h"

namespace fc {
#define FC_BEAM_D(DD) FC_BEAM_HERE(DD, 2) FC_BEAM_HERE(DD, 4)
FC_BEAM_D(16)
FC_BEAM_D(32)
FC_BEAM_D(64)
FC_BEAM_D(128)
FC_BEAM_D(256)
FC_BEAM_D(512)
#undef FC_BEAM_D
}  // namespace fc
