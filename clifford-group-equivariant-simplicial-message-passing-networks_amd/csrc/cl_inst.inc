// (row, channel)-per-lane kernel instantiations (cemlp_cl.hpp) for one algebra. Included by k_cl_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_cl.hpp"
#include "launch.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <int C, int MODE, int NBLK, int NA, bool SAVES>
hipError_t cl_launch_bwd(unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io) {
    constexpr size_t lds = cl_bwd_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    auto kern = cemlp_cl_bwd_kernel<ALG_T, C, MODE, NBLK, NA, SAVES>;
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
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kClWaves), lds, st, Cd, io);
    return hipGetLastError();
}

template <int C, int MODE, int NBLK, int NA>
hipError_t cl_launch(bool bwd, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io_in) {
    const RowIO& io = io_in;
    if (!bwd) {
        constexpr size_t lds = cl_fwd_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
        static_assert(lds <= 64 * 1024, "dynamic LDS beyond 64 KB would need the per-kernel attribute");
        hipLaunchKernelGGL((cemlp_cl_fwd_kernel<ALG_T, C, MODE, NBLK, NA>), dim3(grid), dim3(64 * kClWaves), lds, st, Cd, io);
        return hipGetLastError();
    }
    // all blocks in one launch (last block first); then grads += the workgroups' partial sums of all blocks, fixed order
    if (grid > (unsigned)kClSliceCap) return hipErrorInvalidValue;
    // CSMPN_FLAG_SAVE_STATE selects the instantiation that reads the saved block outputs (a compile-time choice: as a
    // run-time branch it spilled the node program)
    const hipError_t e0 = io.save_state ? cl_launch_bwd<C, MODE, NBLK, NA, true>(grid, st, Cd, io)
                                        : cl_launch_bwd<C, MODE, NBLK, NA, false>(grid, st, Cd, io);
    if (e0 != hipSuccess) return e0;
    constexpr int I0 = ClTab<C, MODE, NA, 0, true>::I;
    constexpr int total = ClPart<ALG_T, C, I0>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
    hipLaunchKernelGGL((cl_reduce_kernel<ALG_T, C, I0, NBLK>), dim3((total + 15) / 16), dim3(256), 0, st, Cd,
                       (const float*)io.rl_partials, (int)grid, (int)kClSliceCap);
    return hipGetLastError();
}
// floats of one slice of every block launch together (the region holds kClSliceCap of them)
template <int C, int MODE, int NBLK, int NA>
constexpr size_t cl_part_floats() {
    return ClPart<ALG_T, C, ClTab<C, MODE, NA, 0, true>::I>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
}
}  // namespace

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

// channels = width of every block's output; i0 = input channels of block 0. *handled = false: no instantiation for
// this shape (the caller goes on to the other kernel families).
hipError_t CSMPN_CAT(launch_cemlp_cl_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0, bool bwd, unsigned grid,
                                                      hipStream_t st, const DevCemlp& C, const RowIO& io, bool* handled) {
    *handled = true;
    if (channels == 8 && mode == MODE_EDGE && nblk == 2 && i0 == 14) return cl_launch<8, MODE_EDGE, 2, 6>(bwd, grid, st, C, io);
    if (channels == 8 && mode == MODE_NODE && nblk == 2 && i0 == 19) return cl_launch<8, MODE_NODE, 2, 3>(bwd, grid, st, C, io);
    *handled = false;
    return hipSuccess;
}
bool CSMPN_CAT(has_cemlp_cl_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0) {
    return channels == 8 && nblk == 2 && ((mode == MODE_EDGE && i0 == 14) || (mode == MODE_NODE && i0 == 19));
}
// floats of one workgroup's slice of a block backward's partial buffer (0: shape not served)
size_t CSMPN_CAT(cemlp_cl_partial_floats_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0) {
    if (channels == 8 && nblk == 2 && mode == MODE_EDGE && i0 == 14) return cl_part_floats<8, MODE_EDGE, 2, 6>();
    if (channels == 8 && nblk == 2 && mode == MODE_NODE && i0 == 19) return cl_part_floats<8, MODE_NODE, 2, 3>();
    return 0;
}
}  // namespace csmpn
