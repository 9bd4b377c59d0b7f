// Per-n instantiation of the run-time-signature row-tile kernel (cemlp_sig.hpp): float and double, forward and backward.
// Included by k_sig_n<n>.hip with CSMPN_SIG_N defined; exports the two overloads of csmpn::sig::launch_n<n>.
#include <atomic>

#include "cemlp_sig.hpp"

#define CSMPN_SIG_CAT2(a, b) a##b
#define CSMPN_SIG_CAT(a, b) CSMPN_SIG_CAT2(a, b)

namespace csmpn {
namespace sig {
namespace {
// dynamic LDS beyond 64 KB must be enabled per kernel and device: grow-only, one slot per device ordinal
template <class Real, bool BWD>
hipError_t launch_dir(unsigned grid, size_t lds, hipStream_t st, const Args<Real>& a) {
    if (lds > kLdsSmall) {
        static std::atomic<size_t> enabled[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (lds > enabled[dev].load(std::memory_order_relaxed)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cemlp_sig_kernel<CSMPN_SIG_N, Real, BWD>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            enabled[dev].store(lds, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL((cemlp_sig_kernel<CSMPN_SIG_N, Real, BWD>), dim3(grid), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}
}  // namespace

hipError_t CSMPN_SIG_CAT(launch_n, CSMPN_SIG_N)(bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args<float>& a) {
    return bwd ? launch_dir<float, true>(grid, lds, st, a) : launch_dir<float, false>(grid, lds, st, a);
}
hipError_t CSMPN_SIG_CAT(launch_n, CSMPN_SIG_N)(bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args<double>& a) {
    return bwd ? launch_dir<double, true>(grid, lds, st, a) : launch_dir<double, false>(grid, lds, st, a);
}
}  // namespace sig
}  // namespace csmpn
