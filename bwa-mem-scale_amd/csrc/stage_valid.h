// stage_valid.h — which of a batch's products are current (bwams_batch::valid, a bit per product): the products, what is computed
// directly from each, and the closure of that, worked out by the compiler.  Plain C++; produced / outdated / has, the three
// functions every entry point uses on the mask, stand behind bwams_batch in common.h.
#pragma once

#include <cstdint>

namespace bwams {

// reads: the resident chunk (d_enc, d_cum, the counts beside them).  names: what bwams_sam_upload leaves.  probe: the EMF probe's
// words of bwams_emf_run.  built: the flat task lists of bwams_extend_build.  ext: the extended regions.  er: mem_perfect2reg's
// regions.  al: mem_reg2aln's records.  sorted, templates, template_locs: of the current BAM records.
enum class Product { reads, names, seeds, probe, chains, built, ext, dedup, pair, er, al, sam, bam, sorted, templates, template_locs, kCount };

constexpr uint32_t bit(Product p) { return 1u << (int)p; }
template <class... P> constexpr uint32_t bits(P... p) { return (0u | ... | bit(p)); }

// {from, to}: to is computed directly from from (the kernels' argument structs say so).  reads -> chains beside seeds -> chains:
// bwams_chain_run_ert and bwams_chain_upload chain over the resident reads without a seed run.  bam has a second source with no
// parent, bwams_bam_upload.  pair -> al holds whatever al was made from (source 0 reads dedup alone): the coarser rule costs a
// caller one bwams_reg2aln_run and saves a special case here.
struct Edge { Product from, to; };
constexpr Edge kEdges[] = {
    {Product::reads, Product::names}, {Product::reads, Product::seeds}, {Product::reads, Product::probe}, {Product::reads, Product::chains},
    {Product::reads, Product::er},
    {Product::seeds, Product::chains},
    {Product::probe, Product::er},
    {Product::chains, Product::built}, {Product::built, Product::ext}, {Product::ext, Product::dedup}, {Product::dedup, Product::pair},
    {Product::dedup, Product::al}, {Product::pair, Product::al},
    {Product::al, Product::sam}, {Product::names, Product::sam}, {Product::er, Product::sam},
    {Product::sam, Product::bam}, {Product::bam, Product::sorted}, {Product::bam, Product::templates},
    {Product::templates, Product::template_locs},
};

// everything computed from p, directly or through other products; p itself only if the edges held a cycle
constexpr uint32_t derived(Product p) {
    uint32_t m = 0;
    for (bool grew = true; grew;) {
        grew = false;
        for (const Edge &e : kEdges)
            if ((e.from == p || (m & bit(e.from))) && !(m & bit(e.to))) {
                m |= bit(e.to);
                grew = true;
            }
    }
    return m;
}
struct DerivedTable {
    uint32_t of[(int)Product::kCount] = {};
    constexpr DerivedTable() {
        for (int i = 0; i < (int)Product::kCount; ++i) of[i] = derived((Product)i);
    }
};
inline constexpr DerivedTable kDerived;

constexpr bool acyclic() {
    for (int i = 0; i < (int)Product::kCount; ++i)
        if (kDerived.of[i] & (1u << i)) return false;
    return true;
}
constexpr uint32_t kBamSide = bits(Product::bam, Product::sorted, Product::templates, Product::template_locs);
static_assert((int)Product::kCount <= 32, "a bit per product in a uint32_t");
static_assert(acyclic(), "no product is its own descendant");
// new reads clear every other product: uploaded BAM records (bwams_bam_upload) go with the rest, the mask does not keep a product's source
static_assert(derived(Product::reads) == ((1u << (int)Product::kCount) - 1 - bit(Product::reads)), "new reads outdate everything else");
static_assert(derived(Product::names) == (bit(Product::sam) | kBamSide), "new names outdate the text and what follows it, nothing before");
static_assert(derived(Product::bam) == (kBamSide - bit(Product::bam)), "new BAM records leave the SAM text valid");
static_assert(!(derived(Product::seeds) & bits(Product::probe, Product::er, Product::names)), "a seed run leaves the probe, its regions and the names valid");

}  // namespace bwams
