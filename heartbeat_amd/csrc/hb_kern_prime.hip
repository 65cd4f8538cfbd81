// The prime kernels (hb_prime.hpp) for 2-, 8- and 16-limb candidates.
#include "hb_prime.hpp"

HB_INST_PRIME(2)
HB_INST_PRIME(8)
HB_INST_PRIME(16)
