// Wide row-tile kernel instantiations (cemlp_wide.hpp), one unit per algebra. Included by k_wide_<tag>.hip with
// CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_wide.hpp"
#include "launch.hpp"

#include <atomic>

namespace csmpn {
namespace {
constexpr int kMaxDevices = 64;
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

template <int MODE, bool BWD>
hipError_t launch_wide_one(unsigned grid, unsigned block, size_t lds, hipStream_t st, const DevCemlp& C, const RowIO& io) {
    auto kern = cemlp_wide_kernel<ALG_T, MODE, BWD>;
    // dynamic LDS beyond 64 KB must be enabled per kernel and device (grow-only; see alg_inst.inc)
    static std::atomic<size_t> lds_enabled[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    size_t cur = lds_enabled[dev].load(std::memory_order_relaxed);
    if (cur < 64 * 1024) cur = 64 * 1024;
    if (lds > cur) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        lds_enabled[dev].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, C, io);
    return hipGetLastError();
}
}  // namespace

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

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
