// rvq_beam_kernel<256, 8> (rvq_beam_kernel.h): a width-8 instantiation compiles about as long as the longest other unit, so each has its own.
#include "rvq_beam_kernel.h"

namespace fc {
FC_BEAM_HERE(256, 8)
}  // namespace fc
