// The listed-block encode's PRF kernel (hb_blocks.hpp) for 64-limb (2048-bit) primes.
#include "hb_blocks.hpp"

HB_INST_BLOCKS(64)
