// chain_count.hip — the counting instances of the chaining kernels (BWAMS_CHAIN_COUNT=1, bwams_debug_chain_counts): chain.hip compiled
// once more for launch_chain_counting alone, so that the code object a production run launches from holds no counting instance
// (chain.hip, at launch_chain, says what their presence cost).
#define BWAMS_CHAIN_COUNT_TU
#include "chain.hip"
