// Host-visible launchers of every kernel family, one set per compiled algebra, and the launch caps and slice bounds the host
// sizes and positions the families' workspace regions by (each unit asserts them against its kernels' own constants).
#pragma once
#include <hip/hip_runtime.h>

#include "cemlp_device.hpp"

namespace csmpn {
constexpr int kMaxLdsBytes = 160 * 1024;

// general row-tile kernels (cemlp_kernel.hpp, cemlp_ps.hpp), wide row-tile kernel (cemlp_wide.hpp), geometric product
#define CSMPN_DECLARE_ALG(tag)                                                                                  \
    bool has_h2_##tag();                                                                                        \
    bool has_ps_##tag();                                                                                        \
    hipError_t launch_cemlp_ps_##tag(int mode, bool bwd, unsigned grid, unsigned block, size_t lds,            \
                                     hipStream_t st, const DevCemlp& C, const RowIO& io);                      \
    hipError_t launch_cemlp_##tag(int mode, int var, int h, bool bwd, unsigned grid, unsigned block, size_t lds,   \
                                  hipStream_t st, const DevCemlp& C, const RowIO& io);                          \
    hipError_t launch_cemlp_wide_##tag(int mode, bool bwd, unsigned grid, unsigned block, size_t lds, hipStream_t st, \
                                       const DevCemlp& C, const RowIO& io);                                    \
    hipError_t launch_gp_##tag(bool bwd, const float* a, const float* b, const float* gout, float* out,        \
                               float* ga, float* gb, long rows, hipStream_t st);

CSMPN_DECLARE_ALG(n2)      // Cl(2,0)
CSMPN_DECLARE_ALG(n3)      // Cl(3,0)
CSMPN_DECLARE_ALG(n4)      // Cl(4,0)
CSMPN_DECLARE_ALG(n5)      // Cl(5,0)
CSMPN_DECLARE_ALG(n5m)     // Cl(4,1): metric (1,1,1,1,-1)
CSMPN_DECLARE_ALG(n4m)     // Cl(3,1): metric (1,1,1,-1)

// ----------------------------------------------------------------------------- lane-kernel families
// The shape a lane-kernel family serves a CEMLP launch by: channels = width of every block's output; attr = attribute
// channels of an EGCL stage (block 0 reads channels + attr input channels in MODE_EDGE, 2 channels + attr in MODE_NODE), under
// MODE_PLAIN the input channels of block 0.
struct LaneShape { int mode, nblk, channels, attr; };
// The slices a backward launched with RowIO::defer_sum left unsummed: its shape, gradient pointers (C), slice region and
// the slices it wrote (= workgroups of the launch). run_rows fills it; the caller owns the region until sum_slices has run.
struct LaneUnit;
struct SliceSet {
    const LaneUnit* unit;   // null: nothing deferred (the launch left complete gradients)
    LaneShape shape;
    DevCemlp C;
    const float* part;
    unsigned nslices;
};
// What one instantiation unit (family x algebra) exports. Both size queries return 0 for a shape the unit does not serve.
struct LaneUnit {
    size_t (*table_floats)(const LaneShape&);   // weight tables the launch packs into the workspace (0: the family has none)
    // one gradient slice of a backward (per workgroup; pl: per wave), all blocks that coexist. The cl, cm and pq entries of
    // dispatch.hip size their regions by it; the pl, plw and pg entries take the bounds below, which those units assert against
    // their slices: there it marks the shape as served and states the exact figure, nothing reads it for sizing
    size_t (*slice_floats)(const LaneShape&);
    // pack: write the weight tables first (pg, pq; plw always does). *handled = false: shape not served, nothing launched.
    hipError_t (*launch)(const LaneShape&, bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& C, const RowIO& io,
                         float* tabs, bool* handled);
    // null: the unit's backwards always sum their slices themselves (they ignore RowIO::defer_sum). Else: grads += the
    // slices of `a` and, if non-null, of `b` (another backward of this unit), in ONE launch where the unit has the pair's
    // kernel; every element summed as the backward's own last kernel would have summed it.
    hipError_t (*sum_slices)(const SliceSet& a, const SliceSet* b, hipStream_t st);
};
inline bool serves(const LaneUnit& u, const LaneShape& s) { return u.table_floats(s) != 0 || u.slice_floats(s) != 0; }
// (an accessor, not an object: a namespace-scope constant would also be emitted into the device code object)
#define CSMPN_DECLARE_LANE_UNIT(family, tag) const LaneUnit& cemlp_##family##_##tag();

// (row, channel)-per-lane kernels (cemlp_cl.hpp)
constexpr int kClMaxFwdGroups = 1024;   // 4-wave workgroups of a forward launch: four per CU (4 waves per SIMD)
// ... of a backward launch: two per CU. One slice of partial sums each: the partial buffer of the cl AND the channel-MFMA
// backwards is laid out for this many slices per block (block 1's start behind them: kClSliceCap of cemlp_cl.hpp)
constexpr int kClMaxBwdGroups = 512;
// These kernels address every array of a launch with a 32-bit byte offset from its base (cemlp_cl.hpp, "addressing"): an
// array may hold at most this many bytes - 4 GiB less a 16 MiB margin for a partial last tile, a lane's place in its row,
// the instruction's immediate offset and the rows a backward wave requests ahead of its last tile (two grid strides of
// tiles: cl_inst.inc checks the sum), so that no offset of a launch wraps. cl_array_fits is the launch condition per array.
constexpr unsigned long long kClMaxArrayBytes = 0xFF000000ull;
constexpr bool cl_array_fits(long rows, int row_floats) {
    return rows >= 0 && (unsigned long long)rows * (unsigned long long)row_floats * 4ull <= kClMaxArrayBytes;
}
static_assert(cl_array_fits(16711680, 64) && !cl_array_fits(16711681, 64), "8 channels of Cl(3,0): 256-byte rows, 16 711 680 of them");
static_assert(cl_array_fits(0, 64) && !cl_array_fits(-1, 64) && !cl_array_fits(1L << 40, 64), "no wrap in the check itself");
CSMPN_DECLARE_LANE_UNIT(cl, n3)

// channel-MFMA kernels (cemlp_cm.hpp)
constexpr int kCmMaxFwdGroups = 768;   // 4-wave workgroups of a forward launch: three per CU
constexpr int kCmMaxBwdGroups = 256;   // ... of a backward launch (one per CU: 512 registers); one slice of partial sums each
CSMPN_DECLARE_LANE_UNIT(cm, n3)

// parity-lane kernels (cemlp_pl.hpp): D = 32 algebras with an odd number of generators, every block 8 output channels
constexpr int kPlMaxBwdGroups = 256;   // one 4-wave workgroup per CU in the backward
CSMPN_DECLARE_LANE_UNIT(pl, n5)
CSMPN_DECLARE_LANE_UNIT(pl, n5m)

// wide parity-lane kernels (cemlp_plw.hpp)
constexpr int kPlwMaxGroups = 256;   // one workgroup per CU
CSMPN_DECLARE_LANE_UNIT(plw, n5)
CSMPN_DECLARE_LANE_UNIT(plw, n5m)

// 16-row-tile MFMA-mixing kernels for D = 32 (cemlp_pg.hpp)
constexpr int kPgGridCap = 256;      // one 8-wave workgroup per CU = gradient slices the kernels index (kPgMaxGroups of cemlp_pg.hpp)
CSMPN_DECLARE_LANE_UNIT(pg, n5)
CSMPN_DECLARE_LANE_UNIT(pg, n5m)

// 16-row-tile MFMA-mixing kernels for Cl(3,0) at 32 channels (cemlp_pq.hpp)
// workgroups a launch may have = gradient slices the workspace region holds (three 4-wave workgroups per CU; kPqMaxGroups of cemlp_pq.hpp)
constexpr unsigned kPqGridCap = 768;
CSMPN_DECLARE_LANE_UNIT(pq, n3)

// ----------------------------------------------------------------------------- the D = 32 families' region at the end of the workspace
// Upper bounds by channel count, not the kernels' exact sizes. Each has two kinds of reader: the family's entry in dispatch.hip
// (its tail need and reservation) and the family's unit (pl_inst.inc, plw_inst.inc, pg_inst.inc), which asserts for every
// shape it serves that its tables and its backward and reduce kernels at the grid cap stay inside.
// the 8-channel parity-lane backward (cemlp_pl.hpp): one slice per wave, 4 waves x kPlMaxBwdGroups workgroups
constexpr size_t pl_part_bytes() { return (size_t)(8 * 768 + 2 * 640) * sizeof(float) * 4 * kPlMaxBwdGroups + 256; }
// gradient slices of the wide parity-lane backward (one slice of weight-gradient MFMA tiles per workgroup); at 8 channels no
// less than the parity-lane backward's, whose shapes the wide family's reservation covers
constexpr size_t plw_part_bytes(int ch) {
    const size_t NG = (ch + 7) / 8, nch0 = 2 * NG + 1;
    const size_t image = 8 * NG * (3 + 3 * 6 + 64) + 16;   // per-channel sums (CP x (3 + 3 G + P)), generous
    const size_t per_cu = 4 / NG > 0 ? 4 / NG : 1;
    const size_t bytes = ((nch0 + 2 * NG) * 12 * 64 * NG + image) * sizeof(float) * kPlwMaxGroups * per_cu + 256;
    return ch == 8 && pl_part_bytes() > bytes ? pl_part_bytes() : bytes;
}
// rotation tables of the wide parity-lane kernels: both blocks at the node stage's width
constexpr size_t plw_tables_bytes(int ch) {
    const size_t NG = (ch + 7) / 8, nch0 = 2 * NG + 1;
    return ((2 * NG * nch0 + 4 * NG * NG) + (2 * NG * NG + 4 * NG * NG)) * 384 * sizeof(float);
}
// The 16-row-tile family (cemlp_pg.hpp) carves the same region: its gradient slices by the wide kernels' bound, its
// weight-fragment tables (up to 368 KB at 28 / 32 channels) by the wide kernels' tables and 64 KB more.
constexpr size_t pg_part_bytes(int ch) { return plw_part_bytes(ch); }
constexpr size_t pg_tables_bytes(int ch) { return plw_tables_bytes(ch) + 65536; }
// ... which the 24-channel tables (312 KB edge, 360 KB node) exceed by up to this much: DESIGN.md section 6, gap 9. Zero
// once pg_tables_bytes is raised, which changes csmpn_cemlp_workspace_bytes.
constexpr size_t pg_tables_overshoot(int ch) { return ch == 24 ? 100352 : 0; }
}  // namespace csmpn
