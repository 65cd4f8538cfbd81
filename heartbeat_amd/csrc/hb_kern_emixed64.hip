// The mixed-owner encodes' kernels (hb_emixed.hpp) for 64-limb (2048-bit) primes.
#include "hb_emixed.hpp"

HB_INST_EMIXED(64)
