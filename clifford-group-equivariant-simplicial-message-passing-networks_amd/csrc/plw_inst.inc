// Wide parity-lane kernel instantiations (cemlp_plw.hpp) for one algebra. Included by k_plw_<tag>.hip
// with CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_plw.hpp"
#include "launch.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <class KERN>
hipError_t plw_enable_lds(KERN kern, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <int NG, int C, int MODE, int NA, int NBLK = 2>
hipError_t plw_launch(bool bwd, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io_in, float* tabs) {
    using CF = PlwCfg<ALG_T, NG, C, MODE, NA, NBLK>;
    RowIO io = io_in;
    io.plw_tabs = tabs;
    {
        auto pk = plw_pack_kernel<CF, ALG_T>;
        hipLaunchKernelGGL(pk, dim3((CF::tab_total + 255) / 256), dim3(256), 0, st, Cd, tabs);
    }
    if (!bwd) {
        auto kern = cemlp_plw_fwd_kernel<ALG_T, CF>;
        constexpr size_t lds = sizeof(float) * CF::fwd_total;
        hipError_t e = plw_enable_lds(kern, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NG), lds, st, Cd, io);
        return hipGetLastError();
    }
    {
        constexpr size_t lds = sizeof(float) * CF::bwd_total;
        // CSMPN_FLAG_SAVE_STATE (two blocks) selects the instantiations that read the saved block outputs
        constexpr bool kCanSave = NBLK > 1;
        const bool saves = kCanSave && io.save_state != 0;
        if constexpr (NBLK > 1) {
            auto k1 = cemlp_plw_bwd_kernel<ALG_T, CF, 1>;
            if constexpr (kCanSave) { if (saves) k1 = cemlp_plw_bwd_kernel<ALG_T, CF, 1, true>; }
            hipError_t e = plw_enable_lds(k1, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k1, dim3(grid), dim3(64 * NG), lds, st, Cd, io);
            auto r1 = plw_reduce_kernel<ALG_T, CF, 1>;
            hipLaunchKernelGGL(r1, dim3((PlwPart<CF, 1>::w_floats + PlwPart<CF, 1>::i_tot + 63) / 64), dim3(64 * kPlReduceSubs), 0, st, Cd, (const float*)io.plw_part, (int)grid);
        }
        auto k0 = cemlp_plw_bwd_kernel<ALG_T, CF, 0>;
        if constexpr (kCanSave) { if (saves) k0 = cemlp_plw_bwd_kernel<ALG_T, CF, 0, true>; }
        hipError_t e = plw_enable_lds(k0, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k0, dim3(grid), dim3(64 * NG), lds, st, Cd, io);
        auto r0 = plw_reduce_kernel<ALG_T, CF, 0>;
        hipLaunchKernelGGL(r0, dim3((PlwPart<CF, 0>::w_floats + PlwPart<CF, 0>::i_tot + 63) / 64), dim3(64 * kPlReduceSubs), 0, st, Cd, (const float*)io.plw_part, (int)grid);
        return hipGetLastError();
    }
}
}  // namespace

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

// served shapes: (channels, NG) x {edge with 6 attribute channels, node with 3}
#define CSMPN_PLW_SHAPES(X) X(8, 1) X(16, 2) X(24, 3) X(28, 4) X(32, 4)

// standalone CEMLPs (MODE_PLAIN; `attr` = input channels <= 8): the convex-hulls feature embeddings,
// CEMLP(2 -> 28, one block) and CEMLP(3 -> 28 -> 28)
#define CSMPN_PLW_PLAIN(X) X(28, 4, 2, 1) X(28, 4, 3, 2)

size_t CSMPN_CAT(cemlp_plw_table_floats_, CSMPN_ALG_TAG)(int mode, int channels, int attr, int nblk) {
#define X(CH, NG_, IN, NB) \
    if (mode == MODE_PLAIN && channels == CH && attr == IN && nblk == NB) return PlwCfg<ALG_T, NG_, CH, MODE_PLAIN, IN, NB>::tab_total;
    CSMPN_PLW_PLAIN(X)
#undef X
    if (nblk != 2) return 0;
#define X(CH, NG_)                                                                                              \
    if (channels == CH && mode == MODE_EDGE && attr == 6) return PlwCfg<ALG_T, NG_, CH, MODE_EDGE, 6>::tab_total; \
    if (channels == CH && mode == MODE_NODE && attr == 3) return PlwCfg<ALG_T, NG_, CH, MODE_NODE, 3>::tab_total;
    CSMPN_PLW_SHAPES(X)
#undef X
    return 0;
}
hipError_t CSMPN_CAT(launch_cemlp_plw_, CSMPN_ALG_TAG)(int mode, int channels, int attr, int nblk, bool bwd, unsigned grid,
                                                       hipStream_t st, const DevCemlp& C, const RowIO& io, float* tabs, bool* handled) {
    *handled = true;
#define X(CH, NG_, IN, NB) \
    if (mode == MODE_PLAIN && channels == CH && attr == IN && nblk == NB) return plw_launch<NG_, CH, MODE_PLAIN, IN, NB>(bwd, grid, st, C, io, tabs);
    CSMPN_PLW_PLAIN(X)
#undef X
    if (nblk != 2) { *handled = false; return hipSuccess; }
#define X(CH, NG_)                                                                                                          \
    if (channels == CH && mode == MODE_EDGE && attr == 6) return plw_launch<NG_, CH, MODE_EDGE, 6>(bwd, grid, st, C, io, tabs); \
    if (channels == CH && mode == MODE_NODE && attr == 3) return plw_launch<NG_, CH, MODE_NODE, 3>(bwd, grid, st, C, io, tabs);
    CSMPN_PLW_SHAPES(X)
#undef X
    *handled = false;
    return hipSuccess;
}
}  // namespace csmpn
