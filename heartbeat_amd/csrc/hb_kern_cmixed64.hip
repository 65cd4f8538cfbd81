// The cxx mixed-owner batches' kernels (hb_cmixed.hpp) for 64-limb (2048-bit) primes.
#include "hb_cmixed.hpp"

HB_INST_CMIXED(64)
