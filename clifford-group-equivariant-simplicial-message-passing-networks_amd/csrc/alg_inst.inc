// Per-algebra kernel instantiations. Included by k_<tag>.hip with
// CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_kernel.hpp"
#include "cemlp_ps.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <int MODE, int VAR, int H, bool BWD>
hipError_t launch_one(unsigned grid, unsigned block, size_t lds, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    return launch_kernel<cemlp_kernel<ALG_T, MODE, VAR, H, BWD>>(grid, block, lds, st, C, io);
}

// H = 2 (32-row tiles for <= 8 channels) is instantiated for the small algebras only: with
// D = 32 blades a 32-row tile does not fit the LDS anyway.
constexpr bool kHasH2 = CSMPN_ALG_N <= 3;

template <int MODE>
hipError_t launch_mode(int var, int h, bool bwd, unsigned grid, unsigned block, size_t lds, hipStream_t st,
                       const DevCemlp& C, const RowIO& io) {
    switch (var) {
        case VAR_WAVE:
            if constexpr (kHasH2) {
                if (h == 2) return bwd ? launch_one<MODE, VAR_WAVE, 2, true>(grid, block, lds, st, C, io)
                                       : launch_one<MODE, VAR_WAVE, 2, false>(grid, block, lds, st, C, io);
            }
            return bwd ? launch_one<MODE, VAR_WAVE, 1, true>(grid, block, lds, st, C, io)
                       : launch_one<MODE, VAR_WAVE, 1, false>(grid, block, lds, st, C, io);
        case VAR_GROUP: return bwd ? launch_one<MODE, VAR_GROUP, 1, true>(grid, block, lds, st, C, io)
                                   : launch_one<MODE, VAR_GROUP, 1, false>(grid, block, lds, st, C, io);
        // deliberate: the forward of VAR_GROUP_NM is the VAR_GROUP instantiation - the variants differ only in the backward's mirror
        case VAR_GROUP_NM: return bwd ? launch_one<MODE, VAR_GROUP_NM, 1, true>(grid, block, lds, st, C, io)
                                      : launch_one<MODE, VAR_GROUP, 1, false>(grid, block, lds, st, C, io);
        default: return bwd ? launch_one<MODE, VAR_GLOBAL, 1, true>(grid, block, lds, st, C, io)
                            : launch_one<MODE, VAR_GLOBAL, 1, false>(grid, block, lds, st, C, io);
    }
}

// parity-split kernels (cemlp_ps.hpp): odd numbers of generators only
constexpr bool kHasPS = (CSMPN_ALG_N % 2) == 1;

template <int MODE, bool BWD>
hipError_t launch_ps_one(unsigned grid, unsigned block, size_t lds, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    if constexpr (kHasPS) {
        return launch_kernel<cemlp_ps_kernel<ALG_T, MODE, BWD>>(grid, block, lds, st, C, io);
    } else {
        return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t CSMPN_CAT(launch_cemlp_, CSMPN_ALG_TAG)(int mode, int var, int h, bool bwd, unsigned grid,
                                                   unsigned block, size_t lds, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    switch (mode) {
        case MODE_PLAIN: return launch_mode<MODE_PLAIN>(var, h, bwd, grid, block, lds, st, C, io);
        case MODE_EDGE: return launch_mode<MODE_EDGE>(var, h, bwd, grid, block, lds, st, C, io);
        default: return launch_mode<MODE_NODE>(var, h, bwd, grid, block, lds, st, C, io);
    }
}

hipError_t CSMPN_CAT(launch_cemlp_ps_, CSMPN_ALG_TAG)(int mode, bool bwd, unsigned grid, unsigned block, size_t lds,
                                                      hipStream_t st, const DevCemlp& C, const RowIO& io) {
    switch (mode) {
        case MODE_PLAIN: return bwd ? launch_ps_one<MODE_PLAIN, true>(grid, block, lds, st, C, io)
                                    : launch_ps_one<MODE_PLAIN, false>(grid, block, lds, st, C, io);
        case MODE_EDGE: return bwd ? launch_ps_one<MODE_EDGE, true>(grid, block, lds, st, C, io)
                                   : launch_ps_one<MODE_EDGE, false>(grid, block, lds, st, C, io);
        default: return bwd ? launch_ps_one<MODE_NODE, true>(grid, block, lds, st, C, io)
                            : launch_ps_one<MODE_NODE, false>(grid, block, lds, st, C, io);
    }
}

hipError_t CSMPN_CAT(launch_gp_, CSMPN_ALG_TAG)(bool bwd, const float* a, const float* b, const float* gout,
                                                float* out, float* ga, float* gb, long rows, hipStream_t st) {
    const unsigned block = 256, grid = (unsigned)((rows + block - 1) / block);
    if (rows == 0) return hipSuccess;
    if (bwd) hipLaunchKernelGGL((gp_kernel<ALG_T, true>), dim3(grid), dim3(block), 0, st, a, b, gout, out, ga, gb, rows);
    else hipLaunchKernelGGL((gp_kernel<ALG_T, false>), dim3(grid), dim3(block), 0, st, a, b, gout, out, ga, gb, rows);
    return hipGetLastError();
}
}  // namespace csmpn

namespace csmpn {
bool CSMPN_CAT(has_h2_, CSMPN_ALG_TAG)() { return CSMPN_ALG_N <= 3; }
bool CSMPN_CAT(has_ps_, CSMPN_ALG_TAG)() { return (CSMPN_ALG_N % 2) == 1; }
}
