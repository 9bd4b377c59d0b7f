// 16-row-tile MFMA-mixing kernels for Cl(3,0), 32 channels (cemlp_pq.hpp): EGCL edge (6 attribute channels) and node (3) programs and
// the standalone CEMLPs of the md17 model (simplex embeddings 60 -> 32 and 90 -> 32 -> 32, head 32 -> 32: md17_cssmpnn.py:85-120,165-176).
#include "cemlp_pq.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<3, 0u>;
static_assert(kPqMaxGroups == (int)kPqGridCap, "slice regions are sized for the grid cap (dispatch.hip: pq_tail)");

template <int MODE, int NA, int NBLK>
hipError_t pq_launch(bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io_in, float* tabs) {
    using CF = PqCfg<ALG_T, 32, MODE, NA, NBLK>;
    RowIO io = io_in;
    io.tabs = tabs;
    hipError_t e = hipSuccess;
    if (pack) e = launch_kernel<pg_pack_kernel<CF, ALG_T>>((CF::tab_floats + 255) / 256, 256, 0, st, Cd, tabs);
    if (e != hipSuccess) return e;
    if (!bwd) return launch_kernel<cemlp_pq_fwd_kernel<ALG_T, CF>>(grid, kPqThreads, sizeof(float) * CF::lds_floats, st, Cd, io);
    // one launch per block (last block first). Block 1's slices are summed by extra workgroups of the block-0 launch (PqAux),
    // block 0's by the fixed-order reduce launch behind it; each block has its own slice region.
    constexpr size_t lds = sizeof(float) * CF::bwd_lds_floats;
    float* part0 = io.slices;
    unsigned nred1 = 0;
    PqAux aux0{nullptr, (int)grid, 0};
    if constexpr (NBLK == 2) {
        constexpr size_t off1 = (size_t)CF::slice_floats(0) * kPqMaxGroups;
        static_assert(off1 + (size_t)CF::slice_floats(1) * kPqMaxGroups == (size_t)CF::slice_both * kPqGridCap,
                      "block 1's slices at the grid cap end where the region the host reserves ends");
        float* part1 = io.slices + off1;
        PqAux aux1{nullptr, (int)grid, 0};
        io.slices = part1;
        e = launch_kernel<cemlp_pq_bwd_kernel<ALG_T, CF, 1>>(grid, kPqThreads, lds, st, Cd, io, aux1);
        if (e != hipSuccess) return e;
        nred1 = (CF::slice_floats(1) + 63) / 64;
        aux0 = PqAux{part1, (int)grid, (int)grid};
        io.slices = part0;
    }
    e = launch_kernel<cemlp_pq_bwd_kernel<ALG_T, CF, 0>>(grid + nred1, kPqThreads, lds, st, Cd, io, aux0);
    if (e != hipSuccess) return e;
    return launch_kernel<pq_reduce_kernel<ALG_T, CF, 0>>((CF::slice_floats(0) + 63) / 64, 256, 0, st, Cd, (const float*)part0, (int)grid);
}

// served shapes, all 32 channels: the EGCL stages (edge with 6 attribute channels, node with 3) and the standalone CEMLPs of
// the md17 model (`attr` = input channels)
template <int MODE, int NBLK, int NA>
constexpr LaneEntry pq_entry() {
    using CF = PqCfg<ALG_T, 32, MODE, NA, NBLK>;
    return {{MODE, NBLK, 32, NA}, CF::tab_floats, CF::slice_both, pq_launch<MODE, NA, NBLK>};
}
constexpr LaneEntry kShapes[] = {pq_entry<MODE_EDGE, 2, 6>(), pq_entry<MODE_NODE, 2, 3>(), pq_entry<MODE_PLAIN, 1, 60>(),
                                 pq_entry<MODE_PLAIN, 2, 90>(), pq_entry<MODE_PLAIN, 1, 32>()};
}  // namespace

const LaneUnit& cemlp_pq_n3() { return LaneUnitOf<kShapes>::unit; }
}  // namespace csmpn
