// Wide row-tile kernel instantiations (cemlp_wide.hpp), one unit per algebra. Included by k_wide_<tag>.hip with
// CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_wide.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <int MODE, bool BWD>
hipError_t launch_wide_one(unsigned grid, unsigned block, size_t lds, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    return launch_kernel<cemlp_wide_kernel<ALG_T, MODE, BWD>>(grid, block, lds, st, C, io);
}
}  // namespace

hipError_t CSMPN_CAT(launch_cemlp_wide_, CSMPN_ALG_TAG)(int mode, bool bwd, unsigned grid, unsigned block, size_t lds,
                                                        hipStream_t st, const DevCemlp& C, const RowIO& io) {
    switch (mode) {
        case MODE_PLAIN: return bwd ? launch_wide_one<MODE_PLAIN, true>(grid, block, lds, st, C, io)
                                    : launch_wide_one<MODE_PLAIN, false>(grid, block, lds, st, C, io);
        case MODE_EDGE: return bwd ? launch_wide_one<MODE_EDGE, true>(grid, block, lds, st, C, io)
                                   : launch_wide_one<MODE_EDGE, false>(grid, block, lds, st, C, io);
        default: return bwd ? launch_wide_one<MODE_NODE, true>(grid, block, lds, st, C, io)
                            : launch_wide_one<MODE_NODE, false>(grid, block, lds, st, C, io);
    }
}
}  // namespace csmpn
