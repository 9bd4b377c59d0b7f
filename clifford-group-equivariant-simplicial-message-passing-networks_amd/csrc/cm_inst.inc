// Channel-MFMA kernel instantiations (cemlp_cm.hpp) for one algebra. Included by k_cm_<tag>.hip with CSMPN_ALG_N,
// CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_cm.hpp"
#include "cemlp_cmb.hpp"
#include "cemlp_cmp.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;
static_assert(kClSliceCap == kClMaxBwdGroups, "one slice layout for cl_reduce_kernel, sized by the host for this many slices per block");
static_assert(kCmMaxBwdGroups <= kClSliceCap, "every workgroup of a backward launch has a slice in that layout");

// floats of one workgroup's slices of a backward's partial buffer, all blocks together (the region holds kClSliceCap of them)
template <int C, int MODE, int NBLK, int NA>
constexpr size_t cm_part_floats() {
    return ClPart<ALG_T, C, CmTab<C, MODE, NA, 0>::I>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
}

template <int C, int MODE, int NBLK, int NA>
hipError_t cm_launch(bool bwd, bool, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io, float*) {
    if (bwd) {
        if (grid > (unsigned)kCmMaxBwdGroups) return hipErrorInvalidValue;
        hipError_t e;
        if constexpr (C == 32) {
            // 32 channels: two waves per row tile (cemlp_cmp.hpp), 4-wave workgroups, one per CU; then the slices' sum
            constexpr size_t lds = cp_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
            static_assert(lds <= 160 * 1024, "one workgroup per CU");
            // CSMPN_FLAG_SAVE_STATE (two blocks) selects the instantiation that reads y, R, s of the blocks from the saved buffer
            const bool saves = NBLK > 1 && io.save_state != 0;
            e = saves ? launch_kernel<cemlp_cmp_kernel<ALG_T, C, MODE, NBLK, NA, true>>(grid, 64 * kCpWaves, lds, st, Cd, io)
                      : launch_kernel<cemlp_cmp_kernel<ALG_T, C, MODE, NBLK, NA>>(grid, 64 * kCpWaves, lds, st, Cd, io);
        } else {
            // all blocks in one launch (last block first), 8-wave workgroups at two waves per SIMD (cemlp_cmb.hpp); then
            // grads += the workgroups' partial sums, fixed order
            constexpr size_t lds = cb_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
            static_assert(lds <= 160 * 1024, "one workgroup per CU");
            e = launch_kernel<cemlp_cmb_kernel<ALG_T, C, MODE, NBLK, NA>>(grid, 64 * kCbWaves, lds, st, Cd, io);
        }
        if (e != hipSuccess) return e;
        constexpr int I0 = CmTab<C, MODE, NA, 0>::I;
        constexpr int total = (int)cm_part_floats<C, MODE, NBLK, NA>();
        // (the host reserves slice_floats x kClMaxBwdGroups = the slices of all blocks at the slice cap: exact by construction)
        return launch_kernel<cl_reduce_kernel<ALG_T, C, I0, NBLK>>((total + 15) / 16, 256, 0, st, Cd, (const float*)io.rl_partials, (int)grid,
                                                                  (int)kClSliceCap);
    }
    constexpr size_t lds = cm_fwd_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
    static_assert((C == 16 ? CM_FWD_OCC : 1) * lds <= 160 * 1024, "workgroups per CU the forward is compiled for");
    return launch_kernel<cemlp_cm_fwd_kernel<ALG_T, C, MODE, NBLK, NA>>(grid, 64 * kCmWaves, lds, st, Cd, io);
}

// served shapes: 16 channels (S2) and 32 channels (md17's width; forward: one workgroup per CU, tables of both blocks: 116 KB
// of LDS) x {edge with 6 attribute channels, node with 3}
template <int C, int MODE, int NBLK, int NA>
constexpr LaneEntry cm_entry() { return {{MODE, NBLK, C, NA}, 0, cm_part_floats<C, MODE, NBLK, NA>(), cm_launch<C, MODE, NBLK, NA>}; }
constexpr LaneEntry kShapes[] = {cm_entry<16, MODE_EDGE, 2, 6>(), cm_entry<16, MODE_NODE, 2, 3>(), cm_entry<32, MODE_EDGE, 2, 6>(),
                                 cm_entry<32, MODE_NODE, 2, 3>()};
}  // namespace

const LaneUnit& CSMPN_CAT(cemlp_cm_, CSMPN_ALG_TAG)() { return LaneUnitOf<kShapes>::unit; }
}  // namespace csmpn
