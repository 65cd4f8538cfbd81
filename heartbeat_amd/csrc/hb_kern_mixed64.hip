// The mixed-owner batches' kernels (hb_mixed.hpp) for 64-limb (2048-bit) primes.
#include "hb_mixed.hpp"

HB_INST_MIXED(64)
