// Parity-lane kernel instantiations (cemlp_pl.hpp) for one algebra. Included by k_pl_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_pl.hpp"
#include "launch.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <int MODE, int NBLK, int I0, bool BWD, bool SAVES = false>
hipError_t pl_launch_one(unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    auto kern = cemlp_pl_kernel<ALG_T, MODE, NBLK, I0, BWD, SAVES>;
    using LY = PlLay<ALG_T, NBLK, I0>;
    constexpr size_t lds = sizeof(float) * (BWD ? LY::bwd_total : LY::fwd_total);
    if constexpr (lds > 64 * 1024) {
        // dynamic LDS beyond 64 KB must be enabled per kernel and device
        static bool enabled[64] = {};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= 64 || !enabled[dev]) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            if (dev >= 0 && dev < 64) enabled[dev] = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kPlWaves), lds, st, C, io);
    if constexpr (BWD) {
        // grads += the waves' slices of parameter-gradient sums, fixed order
        using PP = PlPart<LY>;
        auto red = pl_reduce_kernel<ALG_T, NBLK, I0>;
        hipLaunchKernelGGL(red, dim3((PP::w_floats + 2 * PP::i_blk + 63) / 64), dim3(64 * kPlReduceSubs), 0, st, C, (const float*)io.plw_part,
                           (int)(grid * kPlWaves));
    }
    return hipGetLastError();
}

template <int MODE, int NBLK, int I0>
hipError_t pl_launch_dir(bool bwd, unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    if (!bwd) return pl_launch_one<MODE, NBLK, I0, false>(grid, st, C, io);
    // CSMPN_FLAG_SAVE_STATE selects the instantiation that reads the saved block outputs
    return io.save_state ? pl_launch_one<MODE, NBLK, I0, true, true>(grid, st, C, io) : pl_launch_one<MODE, NBLK, I0, true>(grid, st, C, io);
}
}  // namespace

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

// the EGCL shapes of the S3 configuration: 8 channels, 6 edge-attribute / 3 node-attribute channels
hipError_t CSMPN_CAT(launch_cemlp_pl_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0, bool bwd, unsigned grid,
                                                      hipStream_t st, const DevCemlp& C, const RowIO& io, bool* handled) {
    *handled = true;
    if (channels == 8 && mode == MODE_EDGE && nblk == 2 && i0 == 14) return pl_launch_dir<MODE_EDGE, 2, 14>(bwd, grid, st, C, io);
    if (channels == 8 && mode == MODE_NODE && nblk == 2 && i0 == 19) return pl_launch_dir<MODE_NODE, 2, 19>(bwd, grid, st, C, io);
    *handled = false;
    return hipSuccess;
}
// floats of one wave's slice of the backward's partial buffer (0: shape not served)
size_t CSMPN_CAT(cemlp_pl_slice_floats_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0) {
    if (channels == 8 && nblk == 2 && mode == MODE_EDGE && i0 == 14) return PlPart<PlLay<ALG_T, 2, 14>>::slice;
    if (channels == 8 && nblk == 2 && mode == MODE_NODE && i0 == 19) return PlPart<PlLay<ALG_T, 2, 19>>::slice;
    return 0;
}
bool CSMPN_CAT(has_cemlp_pl_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0) {
    return channels == 8 && nblk == 2 && ((mode == MODE_EDGE && i0 == 14) || (mode == MODE_NODE && i0 == 19));
}
}  // namespace csmpn
