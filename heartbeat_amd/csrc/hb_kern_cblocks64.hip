// The cxx listed-block PRF launch (hb_cblocks.hpp) for 64-limb primes (2048 bits).
#include "hb_cblocks.hpp"

HB_INST_CBLOCKS(64)
