// Host side shared by the kernel instantiation units (*_inst.inc, k_pq_n3.hip): the one way a kernel is launched, and the
// shape table a lane-kernel unit states once and exports as its LaneUnit (launch.hpp).
#pragma once
#include <atomic>

#include "launch.hpp"

#define CSMPN_CAT2(a, b) a##b
#define CSMPN_CAT(a, b) CSMPN_CAT2(a, b)

namespace csmpn {
constexpr int kMaxDevices = 64;

// Launches Kern. Dynamic LDS beyond 64 KB must be enabled per kernel and device: grow-only, and only as far as needed (a
// kernel may also own static LDS, e.g. compiler-promoted private arrays). One slot per device ordinal and kernel instance,
// guarded for concurrent callers; slot 0 where the ordinal cannot be read or is out of range. The general and wide kernels
// come with a run-time `lds` (a plan result); for the lane families it is constexpr: set once per device.
template <auto Kern, class... Args>
hipError_t launch_kernel(unsigned grid, unsigned block, size_t lds, hipStream_t st, const Args&... args) {
    if (lds > 64 * 1024) {
        static std::atomic<size_t> lds_enabled[kMaxDevices];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
        if (lds > lds_enabled[dev].load(std::memory_order_relaxed)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            lds_enabled[dev].store(lds, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, st, args...);
    return hipGetLastError();
}

// One served shape of a lane-kernel unit: its key, the floats of its weight tables and of one gradient slice (what a slice
// is, is the family's business: launch.hpp), the launcher of its instantiation.
struct LaneEntry {
    LaneShape shape;
    size_t table_floats, slice_floats;
    hipError_t (*launch)(bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io, float* tabs);
};

// The LaneUnit of a unit's shape table: every query and the launch look the shape up in that one table.
template <const auto& Table, hipError_t (*SumSlices)(const SliceSet&, const SliceSet*, hipStream_t) = nullptr>
struct LaneUnitOf {
    static const LaneEntry* find(const LaneShape& s) {
        for (const LaneEntry& e : Table)
            if (e.shape.mode == s.mode && e.shape.nblk == s.nblk && e.shape.channels == s.channels && e.shape.attr == s.attr) return &e;
        return nullptr;
    }
    static size_t table_floats(const LaneShape& s) {
        const LaneEntry* e = find(s);
        return e ? e->table_floats : 0;
    }
    static size_t slice_floats(const LaneShape& s) {
        const LaneEntry* e = find(s);
        return e ? e->slice_floats : 0;
    }
    // *handled = false: no instantiation for this shape (the caller goes on to the other kernel families)
    static hipError_t launch(const LaneShape& s, bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io,
                             float* tabs, bool* handled) {
        const LaneEntry* e = find(s);
        *handled = e != nullptr;
        return e ? e->launch(bwd, pack, grid, st, C, io, tabs) : hipSuccess;
    }
    static constexpr LaneUnit unit{table_floats, slice_floats, launch, SumSlices};
};
}  // namespace csmpn
