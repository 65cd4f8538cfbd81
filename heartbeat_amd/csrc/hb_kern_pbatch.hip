// The batched prove's kernels (hb_pbatch.hpp) for 8-, 16- and 32-limb primes.
#include "hb_pbatch.hpp"

HB_INST_PBATCH(8)
HB_INST_PBATCH(16)
HB_INST_PBATCH(32)
