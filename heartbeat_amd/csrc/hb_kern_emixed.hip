// The mixed-owner encodes' kernels (hb_emixed.hpp) for 8-, 16- and 32-limb primes.
#include "hb_emixed.hpp"

HB_INST_EMIXED(8)
HB_INST_EMIXED(16)
HB_INST_EMIXED(32)
