// The batched prove's kernels (hb_pbatch.hpp) for 64-limb (2048-bit) primes.
#include "hb_pbatch.hpp"

HB_INST_PBATCH(64)
