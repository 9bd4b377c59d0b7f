// Per-algebra instantiation of the float64 row-tile kernel (cemlp_f64.hpp). Included by k_f64_<tag>.hip with CSMPN_ALG_N,
// CSMPN_ALG_NEG and CSMPN_ALG_TAG defined; exports csmpn::f64::launch_<tag>.
#include <atomic>

#include "cemlp_f64.hpp"

#define CSMPN_F64_CAT2(a, b) a##b
#define CSMPN_F64_CAT(a, b) CSMPN_F64_CAT2(a, b)

namespace csmpn {
namespace f64 {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;

// dynamic LDS beyond 64 KB must be enabled per kernel and device: grow-only, one slot per device ordinal
template <bool BWD>
hipError_t launch_dir(unsigned grid, size_t lds, hipStream_t st, const Args& a) {
    if (lds > kLdsSmall) {
        static std::atomic<size_t> enabled[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (lds > enabled[dev].load(std::memory_order_relaxed)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cemlp_f64_kernel<ALG_T, BWD>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            enabled[dev].store(lds, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL((cemlp_f64_kernel<ALG_T, BWD>), dim3(grid), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}
}  // namespace

hipError_t CSMPN_F64_CAT(launch_, CSMPN_ALG_TAG)(bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args& a) {
    return bwd ? launch_dir<true>(grid, lds, st, a) : launch_dir<false>(grid, lds, st, a);
}
}  // namespace f64
}  // namespace csmpn
