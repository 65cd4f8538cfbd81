// The batched cxx PRF launch (hb_cbatch.hpp) for 8-, 16- and 32-limb primes.
#include "hb_cbatch.hpp"

HB_INST_CBATCH(8)
HB_INST_CBATCH(16)
HB_INST_CBATCH(32)
