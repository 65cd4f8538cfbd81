// The batched cxx prove and verify launches (hb_cpv.hpp) for 64-limb primes (2048 bits).
#include "hb_cpv.hpp"

HB_INST_CPV(64)
