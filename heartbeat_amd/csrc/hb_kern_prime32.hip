// The prime kernels (hb_prime.hpp) for 32-limb (1024-bit) candidates.
#include "hb_prime.hpp"

HB_INST_PRIME(32)
