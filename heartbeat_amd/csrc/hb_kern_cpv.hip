// The batched cxx prove and verify launches (hb_cpv.hpp) for 8-, 16- and 32-limb primes.
#include "hb_cpv.hpp"

HB_INST_CPV(8)
HB_INST_CPV(16)
HB_INST_CPV(32)
