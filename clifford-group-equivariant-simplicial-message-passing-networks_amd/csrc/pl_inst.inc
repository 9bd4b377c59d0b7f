// Parity-lane kernel instantiations (cemlp_pl.hpp) for one algebra. Included by k_pl_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_pl.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <int MODE, int NBLK, int I0, bool BWD, bool SAVES = false>
hipError_t pl_launch_one(unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    using LY = PlLay<ALG_T, NBLK, I0>;
    constexpr size_t lds = sizeof(float) * (BWD ? LY::bwd_total : LY::fwd_total);
    const hipError_t e = launch_kernel<cemlp_pl_kernel<ALG_T, MODE, NBLK, I0, BWD, SAVES>>(grid, 64 * kPlWaves, lds, st, C, io);
    if constexpr (BWD) {
        if (e != hipSuccess) return e;
        // grads += the waves' slices of parameter-gradient sums, fixed order
        using PP = PlPart<LY>;
        static_assert((size_t)PP::slice * kPlWaves * kPlMaxBwdGroups * sizeof(float) <= pl_part_bytes(),
                      "one slice per wave at the grid cap: inside the region the host reserves");
        return launch_kernel<pl_reduce_kernel<ALG_T, NBLK, I0>>((PP::w_floats + 2 * PP::i_blk + 63) / 64, 64 * kPlReduceSubs, 0, st, C,
                                                               (const float*)io.slices, (int)(grid * kPlWaves));
    }
    return e;
}

// input channels of block 0: the 8-channel segment(s) and the attribute channels
constexpr int pl_i0(int mode, int na) { return (mode == MODE_EDGE ? 8 : 2 * 8) + na; }

template <int MODE, int NBLK, int NA>
hipError_t pl_launch(bool bwd, bool, unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io, float*) {
    constexpr int I0 = pl_i0(MODE, NA);
    if (!bwd) return pl_launch_one<MODE, NBLK, I0, false>(grid, st, C, io);
    // CSMPN_FLAG_SAVE_STATE selects the instantiation that reads the saved block outputs
    return io.save_state ? pl_launch_one<MODE, NBLK, I0, true, true>(grid, st, C, io) : pl_launch_one<MODE, NBLK, I0, true>(grid, st, C, io);
}

// served shapes, the EGCL stages of the S3 configuration: 8 channels x {edge with 6 attribute channels, node with 3}
template <int MODE, int NBLK, int NA>
constexpr LaneEntry pl_entry() {
    return {{MODE, NBLK, 8, NA}, 0, PlPart<PlLay<ALG_T, NBLK, pl_i0(MODE, NA)>>::slice, pl_launch<MODE, NBLK, NA>};
}
constexpr LaneEntry kShapes[] = {pl_entry<MODE_EDGE, 2, 6>(), pl_entry<MODE_NODE, 2, 3>()};
}  // namespace

const LaneUnit& CSMPN_CAT(cemlp_pl_, CSMPN_ALG_TAG)() { return LaneUnitOf<kShapes>::unit; }
}  // namespace csmpn
