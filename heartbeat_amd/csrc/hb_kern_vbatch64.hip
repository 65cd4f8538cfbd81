// The batched verify's kernels (hb_vbatch.hpp) for 64-limb (2048-bit) primes.
#include "hb_vbatch.hpp"

HB_INST_VBATCH(64)
