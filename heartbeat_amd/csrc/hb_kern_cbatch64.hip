// The batched cxx PRF launch (hb_cbatch.hpp) for 64-limb primes (2048 bits).
#include "hb_cbatch.hpp"

HB_INST_CBATCH(64)
