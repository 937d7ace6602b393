// recal_apply.hip — the quality model applied to the QUAL bytes of BAM records (rules A to C in include/bwams.h above
// bwams_recal_model_create).  Neither the reference nor the CIGAR is read: SEQ, QUAL and, with read groups, the aux fields.
//
// The model on the device is laid out as common.h says (RecalModelDev).  An apply:
//   recal_apply_check_kernel    lane per record: rule B.  *bad = min(*bad, record << 3 | reason).
//   recal_apply_record_kernel   lane per record: rule A and recalibration rule 6's read group (aux_rg.h); key = 2 * group + (cycles
//                               negative), the counting add's key, or n_keys for a record that stays as it is.
//   recal_apply_kernel          a wave per rewritten record, a lane per base in rounds of 64: the lanes of a round hold neighbouring
//                               QUAL bytes and SEQ nibbles.  B, the CYCLE and the CONTEXT delta come by three global byte loads per
//                               base from a model of some 30 KB a read group, which stays in cache; one byte store per base.
// A second rewrite kernel was measured against this one and removed (profiles/recal_apply.md): records radix-sorted by
// key, a workgroup staging the key's rows into LDS, a lane rewriting an aligned dword of QUAL.  It was slower, kernel against kernel
// and with its sort.
#include <algorithm>
#include "common.h"
#include "bam_rec.h"
#include "aux_rg.h"

namespace bwams {
namespace {

// rule A without its last test (the first QUAL byte)
__device__ __forceinline__ bool head_taken(const uint8_t *p, uint32_t exclude) { return !(bam_flag(p) & exclude) && bam_l_seq(p) > 0; }

__global__ void __launch_bounds__(256) recal_apply_check_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t exclude,
                                                                int32_t max_cycle, int walk_aux, unsigned long long *bad) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        if (!head_taken(p, exclude)) continue;
        const uint32_t l_name = bam_l_name(p), n_cig = bam_n_cig(p);
        const int64_t l_seq = bam_l_seq(p);
        int why = -1;
        bool found;
        int64_t v0, v1;
        if (bam_aux_at(l_name, n_cig, l_seq) > bam_end(p)) why = kRecalBadBounds;
        else if (!bam_has_qual(p, l_name, n_cig, l_seq)) why = -1;                                 // rule A leaves it alone
        else if (l_seq > max_cycle) why = kRecalBadCycle;
        else if (walk_aux && !aux_first_rg(p, &found, &v0, &v1)) why = kRecalBadAux;
        if (why >= 0) atomicMin(bad, (unsigned long long)r << 3 | (unsigned)why);
    }
}

__global__ void __launch_bounds__(256) recal_apply_record_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t exclude,
                                                                 MdGroupsDev G, uint32_t n_keys, uint32_t *keys, unsigned long long *n_taken) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;                 // whole waves enter every round: the ballot needs them
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += (int64_t)gridDim.x * blockDim.x) {
        bool taken = false;
        if (r < n_rec) {
            const uint8_t *p = bam + rec_off[r];
            taken = head_taken(p, exclude) && bam_has_qual(p, bam_l_name(p), bam_n_cig(p), bam_l_seq(p));
            keys[r] = taken ? rg_key(p, G) : n_keys;                     // rule B walked the aux fields already
        }
        const uint64_t m = __ballot(taken);
        if (lane == 0 && m) atomicAdd(n_taken, (unsigned long long)__popcll((unsigned long long)m));
    }
}

__global__ void __launch_bounds__(256) recal_apply_kernel(uint8_t *bam, const int64_t *rec_off, int64_t n_rec, RecalModelDev M,
                                                          const uint32_t *keys, uint32_t n_keys) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t cols = M.cols();
    for (int64_t r = wave; r < n_rec; r += n_waves) {
        const uint32_t key = keys[r];
        if (key >= n_keys) continue;
        uint8_t *p = bam + rec_off[r];
        const uint32_t l_name = bam_l_name(p), n_cig = bam_n_cig(p);
        const int32_t l_seq = bam_l_seq(p);
        const bool rev = (bam_flag(p) & 0x10) != 0;
        const uint8_t *seq = p + bam_seq_at(l_name, n_cig);
        uint8_t *qual = p + bam_qual_at(l_name, n_cig, l_seq);
        const int64_t row0 = (int64_t)(key >> 1) * kRecalQuals;
        for (int32_t i = lane; i < l_seq; i += 64) {
            const uint32_t byte = qual[i], code = seq_code(seq, i);      // the loads leave before anything branches on them
            const int32_t j = rev ? i + 1 : i - 1;                       // the neighbour in sequencing order
            const uint32_t ncode = j >= 0 && j < l_seq ? seq_code(seq, j) : 0;
            if ((int)byte < M.preserve_below) continue;
            const int64_t row = row0 + (int64_t)min(byte, (uint32_t)(kRecalQuals - 1));
            const int32_t c = rev ? l_seq - i : i + 1;
            const int b = base_of_code(code), nb = base_of_code(ncode);  // recalibration rule 6's context, or none
            int v = (int)M.b[row] + M.dc[row * cols + ((key & 1) ? -c : c) + M.max_cycle];
            if (b >= 0 && nb >= 0) v += M.dx[row * kRecalContexts + recal_context(nb, b, rev)];
            qual[i] = (uint8_t)(v < 1 ? 1 : v > M.max_q ? M.max_q : v);
        }
    }
}

}  // namespace

void launch_recal_apply_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalModelDev &M, int walk_aux,
                              unsigned long long *bad, int cu_count, hipStream_t st) {
    if (n_rec > 0)
        recal_apply_check_kernel<<<grid_of(n_rec, 256, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, M.exclude, M.max_cycle, walk_aux, bad);
}

void launch_recal_apply_records(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalModelDev &M, const MdGroupsDev &G,
                                uint32_t n_keys, uint32_t *keys, unsigned long long *n_taken, int cu_count, hipStream_t st) {
    if (n_rec > 0)
        recal_apply_record_kernel<<<grid_of(n_rec, 256, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, M.exclude, G, n_keys, keys, n_taken);
}

void launch_recal_apply(uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalModelDev &M, const uint32_t *keys, uint32_t n_keys,
                        int cu_count, hipStream_t st) {
    if (n_rec > 0) recal_apply_kernel<<<grid_of(n_rec, 4, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, M, keys, n_keys);
}

}  // namespace bwams
