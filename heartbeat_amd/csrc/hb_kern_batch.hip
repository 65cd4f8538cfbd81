// The batched encode's kernels (hb_batch.hpp) for 8-, 16- and 32-limb primes.
#include "hb_batch.hpp"

HB_INST_BATCH(8)
HB_INST_BATCH(16)
HB_INST_BATCH(32)
