// (row, channel)-per-lane kernel instantiations (cemlp_cl.hpp) for one algebra. Included by k_cl_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_cl.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;
static_assert(kClSliceCap == kClMaxBwdGroups, "the host sizes the partial buffer for the slices the kernels lay it out for");
static_assert(kClNoStore >= kClMaxArrayBytes && kClNoStore <= 0xFFFFFFFFull - 0xFFFF, "the no-store offset lies behind every admitted array and does not wrap");
// the furthest offset a launch forms: a backward wave requests the rows of the tile two grid strides behind its last one
// (8 rows of 256 bytes per tile), plus a partial tile, the lane's place and the immediate offset
static_assert(kClMaxArrayBytes + (2ull * kClMaxBwdGroups * kClWaves + 3) * 8 * 256 + 4096 <= 0x100000000ull, "no offset of a launch wraps");

// floats of one slice of every block launch together (the region holds kClSliceCap of them)
template <int C, int MODE, int NBLK, int NA>
constexpr size_t cl_part_floats() {
    return ClPart<ALG_T, C, ClTab<C, MODE, NA, 0, true>::I>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
}

// grads += the workgroups' slices of one backward (its last kernel)
template <int C, int MODE, int NBLK, int NA>
hipError_t cl_sum(hipStream_t st, const DevCemlp& Cd, const float* part, unsigned nslices) {
    constexpr int I0 = ClTab<C, MODE, NA, 0, true>::I;
    return launch_kernel<cl_reduce_kernel<ALG_T, C, I0, NBLK>>(cl_reduce_groups<ALG_T, C, I0, NBLK>(), 256, 0, st, Cd, part, (int)nslices,
                                                              (int)kClSliceCap);
}

template <int C, int MODE, int NBLK, int NA>
hipError_t cl_launch(bool bwd, bool, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io, float*) {
    if (!bwd) {
        constexpr size_t lds = cl_fwd_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
        return launch_kernel<cemlp_cl_fwd_kernel<ALG_T, C, MODE, NBLK, NA>>(grid, 64 * kClWaves, lds, st, Cd, io);
    }
    // all blocks in one launch (last block first); then grads += the workgroups' partial sums of all blocks, fixed order
    if (grid > (unsigned)kClSliceCap) return hipErrorInvalidValue;
    constexpr size_t lds = cl_bwd_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    // CSMPN_FLAG_SAVE_STATE selects the instantiation that reads the saved block outputs (a compile-time choice: as a
    // run-time branch it spilled the node program)
    const hipError_t e0 = io.save_state ? launch_kernel<cemlp_cl_bwd_kernel<ALG_T, C, MODE, NBLK, NA, true>>(grid, 64 * kClWaves, lds, st, Cd, io)
                                        : launch_kernel<cemlp_cl_bwd_kernel<ALG_T, C, MODE, NBLK, NA, false>>(grid, 64 * kClWaves, lds, st, Cd, io);
    if (e0 != hipSuccess || io.defer_sum) return e0;   // deferred: the caller sums the slices (cl_sum_slices)
    // block 1's slices start kClSliceCap slices of block 0 behind block 0's; the host reserves slice_floats x kClMaxBwdGroups
    // (= kClSliceCap, asserted above), the slices of all blocks at the cap: exact by construction
    return cl_sum<C, MODE, NBLK, NA>(st, Cd, io.rl_partials, grid);
}

// served shapes: 8 channels x {edge with 6 attribute channels, node with 3}
template <int C, int MODE, int NBLK, int NA>
constexpr LaneEntry cl_entry() { return {{MODE, NBLK, C, NA}, 0, cl_part_floats<C, MODE, NBLK, NA>(), cl_launch<C, MODE, NBLK, NA>}; }
constexpr LaneEntry kShapes[] = {cl_entry<8, MODE_EDGE, 2, 6>(), cl_entry<8, MODE_NODE, 2, 3>()};

bool same_shape(const LaneShape& s, const LaneShape& t) {
    return s.mode == t.mode && s.nblk == t.nblk && s.channels == t.channels && s.attr == t.attr;
}
// Deferred slice sums (RowIO::defer_sum). A layer's node and edge backward together: one launch, the node program's elements
// in front. Any other pair: one launch each.
hipError_t cl_sum_slices(const SliceSet& a, const SliceSet* b, hipStream_t st) {
    constexpr LaneShape edge = kShapes[0].shape, node = kShapes[1].shape;
    if (b && same_shape(a.shape, edge) && same_shape(b->shape, node)) return cl_sum_slices(*b, &a, st);
    if (b && same_shape(a.shape, node) && same_shape(b->shape, edge)) {
        constexpr int IN = ClTab<8, MODE_NODE, 3, 0, true>::I, IE = ClTab<8, MODE_EDGE, 6, 0, true>::I;
        constexpr unsigned groups = cl_reduce_groups<ALG_T, 8, IN, 2>() + cl_reduce_groups<ALG_T, 8, IE, 2>();
        return launch_kernel<cl_reduce2_kernel<ALG_T, 8, IN, 2, IE, 2>>(groups, 256, 0, st, a.C, a.part, (int)a.nslices, b->C, b->part,
                                                                         (int)b->nslices, (int)kClSliceCap);
    }
    for (const SliceSet* s : {&a, b}) {
        if (!s) continue;
        hipError_t e = hipErrorInvalidValue;
        if (same_shape(s->shape, edge)) e = cl_sum<8, MODE_EDGE, 2, 6>(st, s->C, s->part, s->nslices);
        else if (same_shape(s->shape, node)) e = cl_sum<8, MODE_NODE, 2, 3>(st, s->C, s->part, s->nslices);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

const LaneUnit& CSMPN_CAT(cemlp_cl_, CSMPN_ALG_TAG)() { return LaneUnitOf<kShapes, cl_sum_slices>::unit; }
}  // namespace csmpn
