// The batched verify's kernels (hb_vbatch.hpp) for 8-, 16- and 32-limb primes.
#include "hb_vbatch.hpp"

HB_INST_VBATCH(8)
HB_INST_VBATCH(16)
HB_INST_VBATCH(32)
