// (row, channel)-per-lane kernel instantiations (cemlp_cl.hpp) for one algebra. Included by k_cl_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_cl.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;
static_assert(kClSliceCap == kClMaxBwdGroups, "the host sizes the partial buffer for the slices the kernels lay it out for");

// floats of one slice of every block launch together (the region holds kClSliceCap of them)
template <int C, int MODE, int NBLK, int NA>
constexpr size_t cl_part_floats() {
    return ClPart<ALG_T, C, ClTab<C, MODE, NA, 0, true>::I>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
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
    if (e0 != hipSuccess) return e0;
    // block 1's slices start kClSliceCap slices of block 0 behind block 0's; the host reserves slice_floats x kClMaxBwdGroups
    // (= kClSliceCap, asserted above), the slices of all blocks at the cap: exact by construction
    constexpr int I0 = ClTab<C, MODE, NA, 0, true>::I;
    constexpr int total = (int)cl_part_floats<C, MODE, NBLK, NA>();
    return launch_kernel<cl_reduce_kernel<ALG_T, C, I0, NBLK>>((total + 15) / 16, 256, 0, st, Cd, (const float*)io.rl_partials, (int)grid,
                                                              (int)kClSliceCap);
}

// served shapes: 8 channels x {edge with 6 attribute channels, node with 3}
template <int C, int MODE, int NBLK, int NA>
constexpr LaneEntry cl_entry() { return {{MODE, NBLK, C, NA}, 0, cl_part_floats<C, MODE, NBLK, NA>(), cl_launch<C, MODE, NBLK, NA>}; }
constexpr LaneEntry kShapes[] = {cl_entry<8, MODE_EDGE, 2, 6>(), cl_entry<8, MODE_NODE, 2, 3>()};
}  // namespace

const LaneUnit& CSMPN_CAT(cemlp_cl_, CSMPN_ALG_TAG)() { return LaneUnitOf<kShapes>::unit; }
}  // namespace csmpn
