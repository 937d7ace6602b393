// chain_count.hip — the counting instances of the chaining kernels (BWAMS_CHAIN_COUNT=1, bwams_debug_chain_counts): chain_wave.h
// instantiated for COUNT = true in a code object of its own, so that the one a production run launches from (chain.hip's) holds
// no counting instance (chain_wave.h, at launch_chain_t, says what their presence cost).
#include "chain_wave.h"

namespace bwams {

int launch_chain_counting(const ChainArgs &A, const uint32_t *n_seeds, int cu_count, hipStream_t st, hipStream_t *aux, hipEvent_t fork, hipEvent_t *join) {
    return launch_chain_t<true>(A, n_seeds, cu_count, st, aux, fork, join);
}

}  // namespace bwams
