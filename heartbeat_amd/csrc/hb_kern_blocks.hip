// The listed-block encode's PRF kernel (hb_blocks.hpp) for 8-, 16- and 32-limb primes.
#include "hb_blocks.hpp"

HB_INST_BLOCKS(8)
HB_INST_BLOCKS(16)
HB_INST_BLOCKS(32)
