// Wide parity-lane kernel instantiations (cemlp_plw.hpp) for one algebra. Included by k_plw_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_plw.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

// block BLK's backward (with SAVES: the instantiation that reads the saved block outputs), then the fixed-order sum of its slices
template <class CF, int BLK>
hipError_t plw_launch_bwd(bool saves, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io) {
    using PP = PlwPart<CF, BLK>;
    constexpr size_t lds = sizeof(float) * CF::bwd_total;
    static_assert((size_t)PP::slice * kPlwMaxGroups * CF::WG_PER_CU_BWD * sizeof(float) <= plw_part_bytes(CF::C),
                  "one slice per workgroup at the grid cap: inside the region the host reserves in front of the tables");
    hipError_t e;
    if constexpr (CF::NBLK > 1) {
        e = !saves ? launch_kernel<cemlp_plw_bwd_kernel<ALG_T, CF, BLK>>(grid, 64 * CF::NG, lds, st, Cd, io)
                   : launch_kernel<cemlp_plw_bwd_kernel<ALG_T, CF, BLK, true>>(grid, 64 * CF::NG, lds, st, Cd, io);
    } else {
        e = launch_kernel<cemlp_plw_bwd_kernel<ALG_T, CF, BLK>>(grid, 64 * CF::NG, lds, st, Cd, io);
    }
    if (e != hipSuccess) return e;
    return launch_kernel<plw_reduce_kernel<ALG_T, CF, BLK>>((PP::w_floats + PP::i_tot + 63) / 64, 64 * kPlReduceSubs, 0, st, Cd,
                                                           (const float*)io.slices, (int)grid);
}

template <class CF>
hipError_t plw_launch(bool bwd, bool, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io_in, float* tabs) {
    static_assert(CF::tab_total * sizeof(float) <= plw_tables_bytes(CF::C), "rotation tables: inside the region the host reserves");
    RowIO io = io_in;
    io.tabs = tabs;
    hipError_t e = launch_kernel<plw_pack_kernel<CF, ALG_T>>((CF::tab_total + 255) / 256, 256, 0, st, Cd, tabs);
    if (e != hipSuccess) return e;
    if (!bwd) return launch_kernel<cemlp_plw_fwd_kernel<ALG_T, CF>>(grid, 64 * CF::NG, sizeof(float) * CF::fwd_total, st, Cd, io);
    // one launch per block (last block first); CSMPN_FLAG_SAVE_STATE (two blocks) selects the instantiations that read the saved block outputs
    const bool saves = CF::NBLK > 1 && io.save_state != 0;
    if constexpr (CF::NBLK > 1) {
        e = plw_launch_bwd<CF, 1>(saves, grid, st, Cd, io);
        if (e != hipSuccess) return e;
    }
    return plw_launch_bwd<CF, 0>(saves, grid, st, Cd, io);
}

template <class CF>
constexpr size_t plw_slice_floats() {
    return CF::NBLK > 1 && PlwPart<CF, 1>::slice > PlwPart<CF, 0>::slice ? PlwPart<CF, 1>::slice : PlwPart<CF, 0>::slice;
}
// served shapes: NG = ceil(channels / 8) waves; the slices of the two blocks' launches take turns in one region
template <int NG, int C, int MODE, int NA, int NBLK = 2>
constexpr LaneEntry plw_entry() {
    using CF = PlwCfg<ALG_T, NG, C, MODE, NA, NBLK>;
    return {{MODE, NBLK, C, NA}, CF::tab_total, plw_slice_floats<CF>(), plw_launch<CF>};
}
#define CSMPN_PLW_EGCL(C, NG) plw_entry<NG, C, MODE_EDGE, 6>(), plw_entry<NG, C, MODE_NODE, 3>()
constexpr LaneEntry kShapes[] = {
    // standalone CEMLPs (MODE_PLAIN; `attr` = input channels <= 8): the convex-hulls feature embeddings,
    // CEMLP(2 -> 28, one block) and CEMLP(3 -> 28 -> 28)
    plw_entry<4, 28, MODE_PLAIN, 2, 1>(), plw_entry<4, 28, MODE_PLAIN, 3, 2>(),
    // EGCL stages: edge with 6 attribute channels, node with 3
    CSMPN_PLW_EGCL(8, 1), CSMPN_PLW_EGCL(16, 2), CSMPN_PLW_EGCL(24, 3), CSMPN_PLW_EGCL(28, 4), CSMPN_PLW_EGCL(32, 4)};
#undef CSMPN_PLW_EGCL
}  // namespace

const LaneUnit& CSMPN_CAT(cemlp_plw_, CSMPN_ALG_TAG)() { return LaneUnitOf<kShapes>::unit; }
}  // namespace csmpn
