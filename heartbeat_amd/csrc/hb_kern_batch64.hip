// The batched encode's kernels (hb_batch.hpp) for 64-limb (2048-bit) primes.
#include "hb_batch.hpp"

HB_INST_BATCH(64)
