// 16-row-tile MFMA-mixing kernel instantiations (cemlp_pg.hpp) for one algebra. Included by k_pg_<tag>.hip with
// CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_pg.hpp"
#include "launch.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <class KERN>
hipError_t pg_enable_lds(KERN kern, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <int C, int MODE, int NA>
hipError_t pg_launch(bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io_in, float* tabs) {
    using CF = PgCfg<ALG_T, C, MODE, NA>;
    RowIO io = io_in;
    io.plw_tabs = tabs;
    if (pack) hipLaunchKernelGGL((pg_pack_kernel<CF, ALG_T>), dim3((CF::tab_floats + 255) / 256), dim3(256), 0, st, Cd, tabs);
    if (!bwd) {
        auto kern = cemlp_pg_fwd_kernel<ALG_T, CF>;
        constexpr size_t lds = sizeof(float) * CF::lds_floats;
        hipError_t e = pg_enable_lds(kern, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kPgThreads), lds, st, Cd, io);
        return hipGetLastError();
    }
    // one launch per block (last block first), each followed by the fixed-order sum of its workgroups' slices
    constexpr size_t lds = sizeof(float) * CF::bwd_lds_floats;
    auto k1 = cemlp_pg_bwd_kernel<ALG_T, CF, 1>;
    hipError_t e = pg_enable_lds(k1, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k1, dim3(grid), dim3(kPgThreads), lds, st, Cd, io);
    hipLaunchKernelGGL((pg_reduce_kernel<ALG_T, CF, 1>), dim3((CF::slice_floats(1) + 63) / 64), dim3(256), 0, st, Cd, (const float*)io.plw_part, (int)grid);
    auto k0 = cemlp_pg_bwd_kernel<ALG_T, CF, 0>;
    e = pg_enable_lds(k0, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k0, dim3(grid), dim3(kPgThreads), lds, st, Cd, io);
    hipLaunchKernelGGL((pg_reduce_kernel<ALG_T, CF, 0>), dim3((CF::slice_floats(0) + 63) / 64), dim3(256), 0, st, Cd, (const float*)io.plw_part, (int)grid);
    return hipGetLastError();
}
}  // namespace

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

// served widths x {edge with 6 attribute channels, node with 3}
#define CSMPN_PG_SHAPES(X) X(24) X(28) X(32)

size_t CSMPN_CAT(cemlp_pg_table_floats_, CSMPN_ALG_TAG)(int mode, int channels, int attr) {
#define X(CH)                                                                                                  \
    if (channels == CH && mode == MODE_EDGE && attr == 6) return PgCfg<ALG_T, CH, MODE_EDGE, 6>::tab_floats;   \
    if (channels == CH && mode == MODE_NODE && attr == 3) return PgCfg<ALG_T, CH, MODE_NODE, 3>::tab_floats;
    CSMPN_PG_SHAPES(X)
#undef X
    return 0;
}
size_t CSMPN_CAT(cemlp_pg_slice_floats_, CSMPN_ALG_TAG)(int mode, int channels, int attr) {
#define X(CH)                                                                                                  \
    if (channels == CH && mode == MODE_EDGE && attr == 6) return PgCfg<ALG_T, CH, MODE_EDGE, 6>::slice_max;    \
    if (channels == CH && mode == MODE_NODE && attr == 3) return PgCfg<ALG_T, CH, MODE_NODE, 3>::slice_max;
    CSMPN_PG_SHAPES(X)
#undef X
    return 0;
}
bool CSMPN_CAT(has_cemlp_pg_, CSMPN_ALG_TAG)(int mode, int channels, int attr, bool bwd) {
    (void)bwd;
    return CSMPN_CAT(cemlp_pg_table_floats_, CSMPN_ALG_TAG)(mode, channels, attr) != 0;
}
hipError_t CSMPN_CAT(launch_cemlp_pg_, CSMPN_ALG_TAG)(int mode, int channels, int attr, bool bwd, bool pack, unsigned grid, hipStream_t st,
                                                      const DevCemlp& C, const RowIO& io, float* tabs, bool* handled) {
    *handled = true;
#define X(CH)                                                                                                               \
    if (channels == CH && mode == MODE_EDGE && attr == 6) return pg_launch<CH, MODE_EDGE, 6>(bwd, pack, grid, st, C, io, tabs);   \
    if (channels == CH && mode == MODE_NODE && attr == 3) return pg_launch<CH, MODE_NODE, 3>(bwd, pack, grid, st, C, io, tabs);
    CSMPN_PG_SHAPES(X)
#undef X
    *handled = false;
    return hipSuccess;
}
}  // namespace csmpn
