// The cxx mixed-owner batches' kernels (hb_cmixed.hpp) for 8-, 16- and 32-limb primes.
#include "hb_cmixed.hpp"

HB_INST_CMIXED(8)
HB_INST_CMIXED(16)
HB_INST_CMIXED(32)
