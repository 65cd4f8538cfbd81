// The cxx listed-block PRF launch (hb_cblocks.hpp) for 8-, 16- and 32-limb primes.
#include "hb_cblocks.hpp"

HB_INST_CBLOCKS(8)
HB_INST_CBLOCKS(16)
HB_INST_CBLOCKS(32)
