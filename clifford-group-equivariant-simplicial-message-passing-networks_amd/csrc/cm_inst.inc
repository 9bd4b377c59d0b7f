// Channel-MFMA kernel instantiations (cemlp_cm.hpp) for one algebra. Included by k_cm_<tag>.hip with CSMPN_ALG_N,
// CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_cm.hpp"
#include "cemlp_cmb.hpp"
#include "cemlp_cmp.hpp"
#include "launch.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

// dynamic LDS beyond 64 KB must be enabled per kernel and device
template <class K>
hipError_t cm_enable_lds(K kern, size_t lds, bool (&enabled)[64]) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !enabled[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) enabled[dev] = true;
    }
    return hipSuccess;
}

template <int C, int MODE, int NBLK, int NA>
hipError_t cm_launch(bool bwd, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io) {
    if (bwd) {
        if constexpr (C == 32) {
            // 32 channels: two waves per row tile (cemlp_cmp.hpp), 4-wave workgroups, one per CU; then the slices' sum
            if (grid > (unsigned)kCmMaxBwdGroups) return hipErrorInvalidValue;
            constexpr size_t lds = cp_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
            static_assert(lds <= 160 * 1024, "one workgroup per CU");
            // CSMPN_FLAG_SAVE_STATE (two blocks) selects the instantiation that reads y, R, s of the blocks from the saved buffer
            const bool saves = NBLK > 1 && io.save_state != 0;
            if (saves) {
                auto kern = cemlp_cmp_kernel<ALG_T, C, MODE, NBLK, NA, true>;
                static bool enabled[64] = {};
                const hipError_t e = cm_enable_lds(kern, lds, enabled);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kCpWaves), lds, st, Cd, io);
            } else {
                auto kern = cemlp_cmp_kernel<ALG_T, C, MODE, NBLK, NA>;
                static bool enabled[64] = {};
                const hipError_t e = cm_enable_lds(kern, lds, enabled);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kCpWaves), lds, st, Cd, io);
            }
            constexpr int I0 = CmTab<C, MODE, NA, 0>::I;
            constexpr int total = ClPart<ALG_T, C, I0>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
            hipLaunchKernelGGL((cl_reduce_kernel<ALG_T, C, I0, NBLK>), dim3((total + 15) / 16), dim3(256), 0, st, Cd,
                               (const float*)io.rl_partials, (int)grid, (int)kClSliceCap);
            return hipGetLastError();
        } else {
        // all blocks in one launch (last block first), 8-wave workgroups at two waves per SIMD (cemlp_cmb.hpp); then
        // grads += the workgroups' partial sums, fixed order
        static_assert(kCmSliceCap == kClSliceCap, "one slice layout for cl_reduce_kernel");
        if (grid > (unsigned)kCmMaxBwdGroups) return hipErrorInvalidValue;
        constexpr size_t lds = cb_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
        static_assert(lds <= 160 * 1024, "one workgroup per CU");
        auto kern = cemlp_cmb_kernel<ALG_T, C, MODE, NBLK, NA>;
        if constexpr (lds > 64 * 1024) {
            static bool enabled[64] = {};
            const hipError_t e = cm_enable_lds(kern, lds, enabled);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kCbWaves), lds, st, Cd, io);
        constexpr int I0 = CmTab<C, MODE, NA, 0>::I;
        constexpr int total = ClPart<ALG_T, C, I0>::total + (NBLK > 1 ? ClPart<ALG_T, C, C>::total : 0);
        hipLaunchKernelGGL((cl_reduce_kernel<ALG_T, C, I0, NBLK>), dim3((total + 15) / 16), dim3(256), 0, st, Cd,
                           (const float*)io.rl_partials, (int)grid, (int)kClSliceCap);
        return hipGetLastError();
        }
    }
    constexpr size_t lds = cm_fwd_lds_bytes<ALG_T, C, MODE, NBLK, NA>();
    static_assert((C == 16 ? CM_FWD_OCC : 1) * lds <= 160 * 1024, "workgroups per CU the forward is compiled for");
    auto kern = cemlp_cm_fwd_kernel<ALG_T, C, MODE, NBLK, NA>;
    if constexpr (lds > 64 * 1024) {
        static bool enabled[64] = {};
        const hipError_t e = cm_enable_lds(kern, lds, enabled);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kCmWaves), lds, st, Cd, io);
    return hipGetLastError();
}
}  // namespace

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

// channels = width of every block's output; i0 = input channels of block 0. *handled = false: no instantiation for
// this shape (the caller goes on to the other kernel families).
hipError_t CSMPN_CAT(launch_cemlp_cm_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0, bool bwd, unsigned grid,
                                                      hipStream_t st, const DevCemlp& C, const RowIO& io, bool* handled) {
    *handled = true;
    if (channels == 16 && mode == MODE_EDGE && nblk == 2 && i0 == 22) return cm_launch<16, MODE_EDGE, 2, 6>(bwd, grid, st, C, io);
    if (channels == 16 && mode == MODE_NODE && nblk == 2 && i0 == 35) return cm_launch<16, MODE_NODE, 2, 3>(bwd, grid, st, C, io);
    // 32 channels (md17's width): the forward only, one workgroup per CU (tables of both blocks: 116 KB of LDS)
    if (channels == 32 && mode == MODE_EDGE && nblk == 2 && i0 == 38) return cm_launch<32, MODE_EDGE, 2, 6>(bwd, grid, st, C, io);
    if (channels == 32 && mode == MODE_NODE && nblk == 2 && i0 == 67) return cm_launch<32, MODE_NODE, 2, 3>(bwd, grid, st, C, io);
    *handled = false;
    return hipSuccess;
}
bool CSMPN_CAT(has_cemlp_cm_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0, bool bwd) {
    (void)bwd;
    if (channels == 32) return nblk == 2 && ((mode == MODE_EDGE && i0 == 38) || (mode == MODE_NODE && i0 == 67));
    return channels == 16 && nblk == 2 && ((mode == MODE_EDGE && i0 == 22) || (mode == MODE_NODE && i0 == 35));
}
// floats of one workgroup's slices of a backward's partial buffer, all blocks together (0: shape not served)
size_t CSMPN_CAT(cemlp_cm_partial_floats_, CSMPN_ALG_TAG)(int mode, int nblk, int channels, int i0) {
    if (!CSMPN_CAT(has_cemlp_cm_, CSMPN_ALG_TAG)(mode, nblk, channels, i0, true)) return 0;
    if (channels == 32) return ClPart<ALG_T, 32, 32>::total + (mode == MODE_EDGE ? ClPart<ALG_T, 32, 38>::total : ClPart<ALG_T, 32, 67>::total);
    return ClPart<ALG_T, 16, 16>::total + (mode == MODE_EDGE ? ClPart<ALG_T, 16, 22>::total : ClPart<ALG_T, 16, 35>::total);
}
}  // namespace csmpn
