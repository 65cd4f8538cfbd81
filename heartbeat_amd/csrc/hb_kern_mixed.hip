// The mixed-owner batches' kernels (hb_mixed.hpp) for 8-, 16- and 32-limb primes.
#include "hb_mixed.hpp"

HB_INST_MIXED(8)
HB_INST_MIXED(16)
HB_INST_MIXED(32)
