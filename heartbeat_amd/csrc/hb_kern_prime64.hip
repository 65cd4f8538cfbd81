// The prime kernels (hb_prime.hpp) for 64-limb (2048-bit) candidates.
#include "hb_prime.hpp"

HB_INST_PRIME(64)
