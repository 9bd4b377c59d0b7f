// 16-row-tile MFMA-mixing kernel instantiations (cemlp_pg.hpp) for one algebra. Included by k_pg_<tag>.hip with
// CSMPN_ALG_N, CSMPN_ALG_NEG and CSMPN_ALG_TAG defined.
#include "cemlp_pg.hpp"
#include "launch_unit.hpp"

namespace csmpn {
namespace {
using ALG_T = Alg<CSMPN_ALG_N, CSMPN_ALG_NEG>;
static_assert(kPgMaxGroups == kPgGridCap, "the host caps the grid at the slices the kernels index");

// block K's backward, then the fixed-order sum of its workgroups' slices
template <class CF, int K>
hipError_t pg_launch_bwd(unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io) {
    const hipError_t e = launch_kernel<cemlp_pg_bwd_kernel<ALG_T, CF, K>>(grid, kPgThreads, sizeof(float) * CF::bwd_lds_floats, st, Cd, io);
    if (e != hipSuccess) return e;
    return launch_kernel<pg_reduce_kernel<ALG_T, CF, K>>((CF::slice_floats(K) + 63) / 64, 256, 0, st, Cd, (const float*)io.slices, (int)grid);
}

template <class CF>
hipError_t pg_launch(bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& Cd, const RowIO& io_in, float* tabs) {
    static_assert((size_t)CF::slice_max * kPgMaxGroups * sizeof(float) <= pg_part_bytes(CF::C),
                  "one slice per workgroup at the grid cap: inside the region the host reserves in front of the tables");
    // pg_tables_overshoot (launch.hpp) is nonzero at 24 channels only: there the tables reach into the general kernels' front
    // part of the workspace, which the family's admission counts in (DESIGN.md section 6, gap 9). Held at today's figure so
    // that the gap cannot widen unnoticed.
    static_assert(CF::tab_floats * sizeof(float) <= pg_tables_bytes(CF::C) + pg_tables_overshoot(CF::C),
                  "weight-fragment tables: inside the region the host reserves, but for the known overshoot");
    RowIO io = io_in;
    io.tabs = tabs;
    hipError_t e = hipSuccess;
    if (pack) e = launch_kernel<pg_pack_kernel<CF, ALG_T>>((CF::tab_floats + 255) / 256, 256, 0, st, Cd, tabs);
    if (e != hipSuccess) return e;
    if (!bwd) return launch_kernel<cemlp_pg_fwd_kernel<ALG_T, CF>>(grid, kPgThreads, sizeof(float) * CF::lds_floats, st, Cd, io);
    // one launch per block (last block first), each followed by the sum of its slices: the blocks' slices take turns in one region
    e = pg_launch_bwd<CF, 1>(grid, st, Cd, io);
    return e != hipSuccess ? e : pg_launch_bwd<CF, 0>(grid, st, Cd, io);
}

// served shapes: 24 / 28 / 32 channels x {edge with 6 attribute channels, node with 3}
template <int C, int MODE, int NA>
constexpr LaneEntry pg_entry() {
    using CF = PgCfg<ALG_T, C, MODE, NA>;
    return {{MODE, 2, C, NA}, CF::tab_floats, CF::slice_max, pg_launch<CF>};
}
#define CSMPN_PG_EGCL(C) pg_entry<C, MODE_EDGE, 6>(), pg_entry<C, MODE_NODE, 3>()
constexpr LaneEntry kShapes[] = {CSMPN_PG_EGCL(24), CSMPN_PG_EGCL(28), CSMPN_PG_EGCL(32)};
#undef CSMPN_PG_EGCL
}  // namespace

const LaneUnit& CSMPN_CAT(cemlp_pg_, CSMPN_ALG_TAG)() { return LaneUnitOf<kShapes>::unit; }
}  // namespace csmpn
