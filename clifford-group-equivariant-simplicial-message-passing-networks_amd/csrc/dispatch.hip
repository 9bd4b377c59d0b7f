// Kernel families of the CEMLP / EGCL stages: which family serves a launch (one shape recogniser, one ordered table), where
// its regions lie in the caller's buffers (one saved-buffer layout, tail regions of the workspace) and run_rows, which
// walks the table and falls through to the general, parity-split and wide row-tile kernels.
#include <atomic>
#include <cstdio>

#include "plan.hpp"

namespace csmpn {

// ----------------------------------------------------------------------------- sizes of the families' workspace regions
namespace {
// the shape of a stage with block 0 reading i0 input channels, as the lane-kernel units key it (launch.hpp)
LaneShape shape_of(int mode, int nblk, int ch, int i0) {
    return LaneShape{mode, nblk, ch, mode == MODE_EDGE ? i0 - ch : (mode == MODE_NODE ? i0 - 2 * ch : i0)};
}
// 16-row-tile MFMA-mixing kernels for Cl(3,0) (cemlp_pq.hpp): weight-fragment tables + one gradient slice per workgroup
size_t pq_region_bytes(int nblk, int ch, int i0) {
    size_t best = 0;
    for (int mode : {MODE_EDGE, MODE_NODE, MODE_PLAIN}) {
        const LaneShape s = shape_of(mode, nblk, ch, i0);
        const size_t tf = cemlp_pq_n3().table_floats(s);
        if (!tf) continue;
        const size_t b = (tf + cemlp_pq_n3().slice_floats(s) * kPqGridCap) * sizeof(float) + 1024;
        best = b > best ? b : best;
    }
    return best;
}
// floats of one slice of the unit's backward, the larger of the edge and the node stage
size_t egcl_slice_floats(const LaneUnit& u, int nblk, int ch, int i0) {
    const size_t e = u.slice_floats(shape_of(MODE_EDGE, nblk, ch, i0)), n = u.slice_floats(shape_of(MODE_NODE, nblk, ch, i0));
    return n > e ? n : e;
}
}  // namespace
// standalone CEMLPs served by the same family (MODE_PLAIN of cemlp_pq.hpp: the md17 embeddings and head): their saved buffer holds,
// under CSMPN_FLAG_SAVE_STATE, the state regions of the family (one block: nothing else; two blocks: block-1 inputs + hand-over rows)
bool pq_plain_shape(int n, const csmpn_block_params* blocks, int nblk) {
    if (n != 3 || nblk < 1 || nblk > 2 || sw().no_pq || sw().no_cm || sw().no_cm_bwd) return false;
    for (int k = 0; k < nblk; ++k)
        if (blocks[k].out_features != 32 || (k > 0 && blocks[k].in_features != 32)) return false;
    return cemlp_pq_n3().table_floats(LaneShape{MODE_PLAIN, nblk, 32, blocks[0].in_features}) != 0;
}
namespace {
size_t rl_partial_bytes(int n, const csmpn_block_params* blocks, int nblk) {
    if (n != 3 || nblk < 1 || nblk > 2) return 0;
    const int ch = blocks[0].out_features;
    for (int k = 0; k < nblk; ++k)
        if (blocks[k].out_features != ch || (k > 0 && blocks[k].in_features != ch)) return 0;
    // (row, channel)-per-lane backward (cemlp_cl.hpp): one slice per workgroup
    const int i0 = blocks[0].in_features;
    const size_t cl = egcl_slice_floats(cemlp_cl_n3(), nblk, ch, i0) * sizeof(float) * kClMaxBwdGroups;
    // channel-MFMA backward (cemlp_cmb.hpp / cemlp_cmp.hpp): the same region and slice layout
    const size_t cm = egcl_slice_floats(cemlp_cm_n3(), nblk, ch, i0) * sizeof(float) * kClMaxBwdGroups;
    const size_t lane = cm > cl ? cm : cl;
    const size_t pq = pq_region_bytes(nblk, ch, i0);   // the same region serves whichever family takes the launch
    return pq > lane ? pq : lane;
}
// the (row, channel)-per-lane backward hands d/d(block-1 input) from its block-1 launch to its block-0 launch through
// one more [rows, C, D] region behind the saved block inputs (as the wide parity-lane kernels do)
bool cl_shape(int n, const csmpn_block_params* blocks, int nblk) {
    if (n != 3 || nblk != 2) return false;
    const int ch = blocks[0].out_features, i0 = blocks[0].in_features;
    if (blocks[1].out_features != ch || blocks[1].in_features != ch) return false;
    if (egcl_slice_floats(cemlp_cl_n3(), nblk, ch, i0)) return true;
    return !sw().no_cm_bwd && egcl_slice_floats(cemlp_cm_n3(), nblk, ch, i0);
}
}  // namespace

// Shapes whose backward may run block by block on the general kernels (cemlp_kernel.hpp, `phased`): small algebras, more
// than one block, no lane-kernel family of their own. They get a hand-over region as large as the saved inputs behind them.
bool general_phased_shape(int n, const csmpn_block_params* blocks, int nblk) {
    if (n > 3 || nblk < 2 || nblk > CSMPN_MAX_BLOCKS) return false;
    for (int k = 0; k < nblk; ++k)
        if (blocks[k].out_features > 64) return false;   // the wide kernel has no LDS mirror to shrink: no phased form
    if (n == 3 && nblk == 2) {
        const int ch = blocks[0].out_features, i0 = blocks[0].in_features;
        if (blocks[1].out_features == ch && blocks[1].in_features == ch) {
            if (cl_shape(n, blocks, nblk)) return false;
        }
    }
    return true;
}

namespace {
// bytes of the wide parity-lane kernels' rotation tables (cemlp_plw.hpp) and gradient slices, also carved from the END of
// the workspace (never together with the row-per-lane region: different algebras). Upper bounds over the entry points (launch.hpp).
size_t plw_table_bytes(int n, const csmpn_block_params* blocks, int nblk) {
    if (n != 5 || nblk < 1 || nblk > 2) return 0;
    const int ch = blocks[0].out_features;
    if (ch < 8 || ch > 32) return 0;
    if (nblk == 2 && (blocks[1].out_features != ch || blocks[1].in_features != ch)) return 0;
    return plw_tables_bytes(ch) + 256 + plw_part_bytes(ch) + (ch > 16 ? kPgTablesExtraBytes : 0);
}
}  // namespace

size_t family_tail_bytes(int n, const csmpn_block_params* blocks, int nblk) {
    return rl_partial_bytes(n, blocks, nblk) + plw_table_bytes(n, blocks, nblk);
}

// ----------------------------------------------------------------------------- saved-buffer layout
namespace {
// channels (x D floats) per row of the CSMPN_FLAG_SAVE_STATE regions (cemlp_device.hpp: whole row tiles in the kernels' lane
// order, one region per tensor and block, rows rounded up to 16):
//   Cl(3,0) 8 channels (cemlp_cl.hpp)                    s of every block
//   Cl(3,0) 32 channels (cemlp_cm.hpp / cemlp_cmp.hpp / cemlp_pq.hpp)    s, y, R of every block
//   Cl(5,0) / Cl(4,1), 8 .. 32 channels (cemlp_pl.hpp / cemlp_plw.hpp)   s, y, R of every block, channels padded to groups of 8
size_t state_channels(int n, const csmpn_block_params* blocks, int n_blocks) {
    if (pq_plain_shape(n, blocks, n_blocks)) return (size_t)3 * n_blocks * 32;   // cemlp_pq.hpp, MODE_PLAIN: s, y, R of every block
    if (n_blocks != 2) return 0;
    const size_t ch = (size_t)blocks[0].out_features;
    // (17 .. 32 channels: 32 - the 16-row-tile kernels of cemlp_pg.hpp keep 4 channels per wave, 8 waves per tile)
    if (plw_table_bytes(n, blocks, n_blocks)) return (size_t)3 * n_blocks * (ch > 16 ? 32 : (ch + 7) / 8 * 8);
    if (cl_shape(n, blocks, n_blocks)) {
        if (egcl_slice_floats(cemlp_cl_n3(), n_blocks, (int)ch, blocks[0].in_features)) return (size_t)n_blocks * ch;
        // the state regions of the 32-channel kernels exist only while their pair backward is enabled
        if (ch == 32 && !sw().no_cm_bwd) return (size_t)3 * n_blocks * 32;
    }
    return 0;
}
}  // namespace

SavedLayout saved_layout(int n, const csmpn_block_params* blocks, int nblk, int64_t rows, uint32_t flags) {
    SavedLayout L{};
    for (int k = 0; k + 1 < nblk; ++k) L.inputs_ch += (size_t)blocks[k].out_features;
    // Hand-over of d/d(block-1 input) from the block-1 launch to the block-0 launch: one [rows, O, D] region for the wide
    // parity-lane, (row, channel)-per-lane and channel-MFMA backwards. The general kernels' phased backward has one slot per
    // saved input; make_plan takes that form only from sw().phased_min_rows rows on (the same switch, read once), while the
    // 16-row-tile family's standalone CEMLPs hand over through it at every row count.
    if ((nblk == 2 && plw_table_bytes(n, blocks, nblk)) || cl_shape(n, blocks, nblk))
        L.handover_ch = (size_t)blocks[0].out_features;
    else if (general_phased_shape(n, blocks, nblk) && (rows < 0 || rows >= sw().phased_min_rows || pq_plain_shape(n, blocks, nblk)))
        L.handover_ch = L.inputs_ch;
    if (rows < 0 || (flags & CSMPN_FLAG_SAVE_STATE)) L.state_ch = state_channels(n, blocks, nblk);
    if (rows < 0) {   // upper bound per row (the state regions hold up to 15 padding rows more)
        L.total = (L.inputs_ch + L.handover_ch + L.state_ch) << n;
        return L;
    }
    const size_t state_rows = (size_t)((rows + 15) & ~(int64_t)15);
    L.handover_off = (L.inputs_ch * (size_t)rows) << n;
    L.state_off = ((L.inputs_ch + L.handover_ch) * (size_t)rows) << n;
    L.total = L.state_off + ((L.state_ch * state_rows) << n);
    return L;
}

// ----------------------------------------------------------------------------- the families
namespace {

// The stage a launch runs, read off the plan and the input segments once per run_rows call: EGCL edge (I0 = ch + na), EGCL
// node (I0 = 2 ch + na) or a plain CEMLP (na = I0: its input channels).
struct StageShape {
    bool ok;               // EGCL modes: the gathered segments have the layer's width
    int ch, na, i0, nblk;
    bool uniform_width;    // every block ch -> ch (block 0: I0 -> ch)
    bool all_w1_sub;       // every MVLinear weight has one slice per grade
};
StageShape stage_shape(const DevCemlp& C, int mode, const RowIO& io) {
    StageShape S{true, C.b[0].O, C.b[0].I, C.b[0].I, C.nblk, true, true};
    const int ch = S.ch;
    for (int k = 0; k < C.nblk; ++k) {
        if (C.b[k].O != ch || (k > 0 && C.b[k].I != ch)) S.uniform_width = false;
        if (!C.b[k].w1_sub) S.all_w1_sub = false;
    }
    if (mode == MODE_EDGE) {
        S.na = io.nseg > 1 ? io.seg[1].ch : 0;
        if (io.seg[0].ch != ch || S.i0 != ch + S.na) S.ok = false;
    } else if (mode == MODE_NODE) {
        S.na = io.nseg > 2 ? io.seg[2].ch : 0;
        if (io.seg[0].ch != ch || io.seg[1].ch != ch || S.i0 != 2 * ch + S.na) S.ok = false;
    }
    return S;
}

struct Launch {   // one run_rows call as the families see it
    const Plan& plan;
    const AlgOps& A;
    int mode;
    bool bwd, tables_ready;
    StageShape S;
    float* handover;   // hand-over rows behind the saved block inputs (saved_layout)
};
LaneShape lane_shape(const Launch& x) { return LaneShape{x.mode, x.S.nblk, x.S.ch, x.S.na}; }
bool egcl(const Launch& x) { return x.mode != MODE_PLAIN && x.S.ok; }
bool two_uniform_blocks(const Launch& x) { return x.S.nblk == 2 && x.S.uniform_width && x.S.all_w1_sub; }
bool fits(const Plan& plan, size_t bytes) { return plan.workspace && plan.workspace_bytes >= bytes; }
unsigned capped(long groups, long cap) { return (unsigned)(groups < cap ? groups : cap); }

enum DebugFields { kChannelsAttr, kChannelsI0, kI0 };
struct Family {
    const char* name;
    DebugFields debug_fields;
    bool (*eligible)(const Launch& x, const RowIO& io);
    unsigned (*grid)(const Launch& x, long rows);
    // the family's regions at the end of the workspace and in the saved buffer; *tabs: its weight tables
    int (*regions)(const Launch& x, RowIO& io, float** tabs);
    const LaneUnit* (*unit)(const AlgOps& A);   // the instantiation unit that launches (null: the algebra has none)
    void (*kernel_label)(const Launch& x, const RowIO& io);
};

// 16-row-tile MFMA-mixing kernels for Cl(3,0) (cemlp_pq.hpp): two blocks of 32 channels, EGCL edge / node programs, and the
// standalone one- / two-block CEMLPs of the md17 model (embeddings and head)
bool pq_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (sw().no_pq || sw().no_cm || x.plan.id != ALG_N3) return false;
    if (S.nblk != 2 && !(S.nblk == 1 && x.mode == MODE_PLAIN)) return false;
    if (S.ch != 32 || !S.uniform_width || !S.all_w1_sub || !S.ok) return false;
    // standalone CEMLP: one contiguous input of I0 channels; not the fused embedding
    if (x.mode == MODE_PLAIN && (io.nseg != 1 || io.emb_nperm != 0 || io.seg[0].ch != S.i0)) return false;
    if (!cemlp_pq_n3().table_floats(lane_shape(x)) || !fits(x.plan, pq_region_bytes(S.nblk, S.ch, S.i0))) return false;
    // the backward runs on the state its forward saved (CSMPN_FLAG_SAVE_STATE, in ITS lane order); without the flag the
    // forward still serves (it writes the row-major block-1 inputs) and the wave-pair backward (cemlp_cmp.hpp) recomputes
    return !x.bwd || (io.saved && io.save_state && !sw().no_cm_bwd);
}
unsigned pq_grid(const Launch&, long rows) {
    // one 16-row tile per workgroup iteration, three 4-wave workgroups per CU (backward: a workgroup ends with one slice of
    // weight-gradient tiles, 62-78 KB; measured with 1 / 2 / 3 tiles per workgroup on launches below the cap: md17 step
    // 2.11 / 2.28 / 2.43 ms, M32 1.024 / 1.008 / 1.012e8 edges/s: one tile)
    return capped((rows + 15) / 16, kPqGridCap);
}
int pq_regions(const Launch& x, RowIO& io, float** tabs) {
    *tabs = reinterpret_cast<float*>(tail_region(x.plan, cemlp_pq_n3().table_floats(lane_shape(x)) * sizeof(float) + 16, 256));
    io.slices = reinterpret_cast<float*>(reinterpret_cast<char*>(*tabs) - cemlp_pq_n3().slice_floats(lane_shape(x)) * sizeof(float) * kPqGridCap);
    if (x.bwd) io.handover = x.handover;
    return CSMPN_OK;
}
void pq_label(const Launch& x, const RowIO&) {
    note_kernel("csmpn::cemlp_pq_%s_kernel<%s, ...> (mode %d, %d channels, %d %s channels, %d block%s)", x.bwd ? "bwd" : "fwd", x.A.name,
                x.mode, x.S.ch, x.S.na, x.mode == MODE_PLAIN ? "input" : "attribute", x.S.nblk, x.S.nblk > 1 ? "s" : "");
}

// 16-row-tile MFMA-mixing kernels (cemlp_pg.hpp): Cl(5,0) / Cl(4,1), two blocks of 24 / 28 / 32 channels, EGCL edge / node programs
bool pg_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (sw().no_pg || !x.A.pg || !two_uniform_blocks(x) || S.ch <= 16 || S.ch > 32 || !egcl(x)) return false;
    const size_t tf = x.A.pg->table_floats(lane_shape(x));
    if (tf == 0 || !fits(x.plan, tf * sizeof(float) + plw_part_bytes(S.ch) + 1024)) return false;
    // the backward of this family runs on the state its forward saved (CSMPN_FLAG_SAVE_STATE, in ITS lane order): without
    // the flag the forward still serves (it writes the row-major block-1 inputs every backward reads) and the wide
    // parity-lane backward recomputes from them
    return !x.bwd || (io.saved && io.save_state);
}
unsigned pg_grid(const Launch&, long rows) { return capped((rows + 15) / 16, kPgGridCap); }   // one 16-row tile per workgroup iteration, one 8-wave workgroup per CU
int pg_regions(const Launch& x, RowIO& io, float** tabs) {
    *tabs = reinterpret_cast<float*>(tail_region(x.plan, x.A.pg->table_floats(lane_shape(x)) * sizeof(float) + 16, 256));
    io.slices = reinterpret_cast<float*>(reinterpret_cast<char*>(*tabs) - plw_part_bytes(x.S.ch));
    if (x.bwd) io.handover = x.handover;
    return CSMPN_OK;
}
void pg_label(const Launch& x, const RowIO&) {
    note_kernel("csmpn::cemlp_pg_%s_kernel<%s, ...> (mode %d, %d channels, %d attribute channels)", x.bwd ? "bwd" : "fwd", x.A.name, x.mode,
                x.S.ch, x.S.na);
}

// wide parity-lane kernels (cemlp_plw.hpp): Cl(5,0) / Cl(4,1), one or two blocks of 16 / 24 / 28 / 32 channels, EGCL edge / node
// programs and standalone CEMLPs of at most 8 input channels (the one input chunk; with the embed descriptor: the fused embedding)
bool plw_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (sw().no_plw || !x.A.plw || S.nblk < 1 || S.nblk > 2) return false;
    // 8 channels belong to cemlp_pl.hpp; the one-group wide kernels take them only on request (round 2 measured them 4-5x
    // slower - compiled for four waves per SIMD by mistake, 1.3 KB of scratch; with the launch bounds repaired they are on a
    // par: S3 1.339 against 1.333 ms)
    if ((S.ch <= 8 && !(S.ch == 8 && sw().plw8)) || S.ch > 32 || !S.uniform_width || !S.all_w1_sub || !S.ok) return false;
    if (x.mode == MODE_PLAIN && (S.na < 1 || S.na > 8 || io.nseg != 1)) return false;
    const size_t tf = x.A.plw->table_floats(lane_shape(x));
    if (tf == 0 || !fits(x.plan, tf * sizeof(float) + plw_part_bytes(S.ch) + 1024)) return false;
    return !(x.bwd && S.nblk > 1 && !io.saved);
}
unsigned plw_grid(const Launch& x, long rows) {
    const long per_cu = 4 / ((x.S.ch + 7) / 8) > 0 ? 4 / ((x.S.ch + 7) / 8) : 1;   // workgroups of NG waves per CU at one wave per SIMD
    // one 4-row tile per workgroup iteration; forward: twice the workgroups where LDS allows
    return capped((rows + 3) / 4, (x.bwd ? kPlwMaxGroups : 2 * kPlwMaxGroups) * per_cu);
}
int plw_regions(const Launch& x, RowIO& io, float** tabs) {
    *tabs = reinterpret_cast<float*>(tail_region(x.plan, x.A.plw->table_floats(lane_shape(x)) * sizeof(float) + 16, 256));
    io.slices = reinterpret_cast<float*>(reinterpret_cast<char*>(*tabs) - plw_part_bytes(x.S.ch));
    if (x.bwd && x.S.nblk > 1) io.handover = x.handover;
    return CSMPN_OK;
}
void plw_label(const Launch& x, const RowIO&) {   // the wide kernels' template arguments live in plw_inst.inc: family + shape
    note_kernel("csmpn::cemlp_plw_%s_kernel<%s, ...> (mode %d, %d channels, %d attribute channels, %d blocks)", x.bwd ? "bwd" : "fwd",
                x.A.name, x.mode, x.S.ch, x.S.na, x.S.nblk);
}

// parity-lane kernels (cemlp_pl.hpp): Cl(5,0) / Cl(4,1), two blocks of 8 channels, the EGCL attribute widths of S3
bool pl_eligible(const Launch& x, const RowIO& io) {
    if (sw().no_pl || !x.A.pl || !two_uniform_blocks(x) || x.S.ch != 8 || !egcl(x)) return false;
    if (x.bwd && !io.saved) return false;
    return serves(*x.A.pl, lane_shape(x));
}
unsigned pl_grid(const Launch& x, long rows) {
    const long tiles = (rows + 3) / 4;   // 4 rows per wave tile; one / two 4-wave workgroups per CU
    return capped((tiles + 3) / 4, x.bwd ? kPlMaxBwdGroups : 512);
}
int pl_regions(const Launch& x, RowIO& io, float**) {
    if (!x.bwd) return CSMPN_OK;
    // per-wave slices of parameter-gradient sums: at the end of the workspace (as the wide kernels' region)
    const size_t pb = plw_part_bytes(8);
    if (!fits(x.plan, pb + 1024)) return fail(CSMPN_ERR_INVALID, "workspace too small for the parity-lane backward");
    io.slices = reinterpret_cast<float*>(tail_region(x.plan, pb + 16, 256));
    return CSMPN_OK;
}
void pl_label(const Launch& x, const RowIO& io) {
    note_kernel("csmpn::cemlp_pl_kernel<%s, %d, %d, %d, %s, %s>", x.A.name, x.mode, x.S.nblk, x.S.i0, x.bwd ? "true" : "false",
                x.bwd && io.save_state ? "true" : "false");
}

// (row, channel)-per-lane kernels (cemlp_cl.hpp): Cl(3,0), two blocks of 8 channels, the EGCL attribute widths of S1.
// CSMPN_NO_CL=1 leaves these shapes to the general kernels (A/B measurements, parity tests of both paths).
bool cl_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (sw().no_cl || x.plan.id != ALG_N3 || !two_uniform_blocks(x) || !egcl(x)) return false;
    if (x.bwd && !io.saved) return false;
    if (!serves(cemlp_cl_n3(), lane_shape(x))) return false;
    // 32-bit byte offsets (launch.hpp): the row arrays of the launch (the state regions round the rows up to 16) and, in
    // the edge program, the node tables it gathers from and scatters into. Larger launches go to the general kernels.
    const int row_floats = S.ch * x.A.D;
    if (!cl_array_fits(io.rows + 16, row_floats)) return false;
    // (a caller that does not state the tables' rows is not served: a resource of no records reads zeros)
    if (x.mode == MODE_EDGE && (io.gather_rows <= 0 || !cl_array_fits(io.gather_rows, row_floats))) return false;
    return !x.bwd || fits(x.plan, cemlp_cl_n3().slice_floats(lane_shape(x)) * sizeof(float) * kClMaxBwdGroups);
}
unsigned cl_grid(const Launch& x, long rows) {
    const long rows_per_wave = 64 / x.S.ch;
    const long tiles = (rows + rows_per_wave - 1) / rows_per_wave;
    // tile t belongs to wave t % (4 grid): four 4-wave workgroups per CU in the forward (~100 VGPRs), two in a
    // block backward (<= 256)
    long cap = x.bwd ? kClMaxBwdGroups : kClMaxFwdGroups;
    // experiments: fewer resident workgroups (never more: the partial buffer has kClMaxBwdGroups slices)
    const long cap_f = sw().cl_cap_fwd, cap_b = sw().cl_cap_bwd;
    if (!x.bwd && cap_f > 0 && cap_f < 4096) cap = cap_f;
    if (x.bwd && cap_b > 0 && cap_b < cap) cap = cap_b;
    return capped((tiles + 3) / 4, cap);
}
int cl_regions(const Launch& x, RowIO& io, float**) {
    if (!x.bwd) return CSMPN_OK;
    const size_t pb = cemlp_cl_n3().slice_floats(lane_shape(x)) * sizeof(float) * kClMaxBwdGroups;
    io.rl_partials = reinterpret_cast<float*>(tail_region(x.plan, pb, 16));
    io.handover = x.handover;
    return CSMPN_OK;
}
void cl_label(const Launch& x, const RowIO& io) {
    note_kernel("csmpn::cemlp_cl_%s_kernel<%s, %d, %d, %d, %d%s>", x.bwd ? "bwd" : "fwd", x.A.name, x.S.ch, x.mode, x.S.nblk, x.S.na,
                !x.bwd ? "" : (io.save_state ? ", true" : ", false"));
}

// channel-MFMA kernels (cemlp_cm.hpp): Cl(3,0), two blocks of 16 channels (S2) or 32 channels (md17), the EGCL attribute
// widths (6, 3). CSMPN_NO_CM=1 leaves these shapes to the general kernels (A/B measurements, parity tests of both paths);
// CSMPN_NO_CM_BWD=1 their backward only.
bool cm_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (sw().no_cm || x.plan.id != ALG_N3 || !two_uniform_blocks(x) || !egcl(x)) return false;
    if (x.bwd && !io.saved) return false;
    if (!serves(cemlp_cm_n3(), lane_shape(x))) return false;
    return !x.bwd || (!sw().no_cm_bwd && fits(x.plan, cemlp_cm_n3().slice_floats(lane_shape(x)) * sizeof(float) * kClMaxBwdGroups));
}
unsigned cm_grid(const Launch& x, long rows) {
    const long tiles = (rows + 15) / 16;   // tile t (16 rows) belongs to wave t % (4 grid)
    const long cap = x.bwd ? kCmMaxBwdGroups : (x.S.ch == 16 ? kCmMaxFwdGroups : 256);   // 32 channels: one workgroup per CU
    // tiles per workgroup and pass: 4 (one per wave), 8 in the 16-channel backward (8-wave workgroups), 2 in the
    // 32-channel backward (a wave PAIR per tile: with 4 the 59 tiles of an md17 batch's node launch went to 15
    // workgroups, two tiles after each other per pair, while 241 CUs idled)
    const long per_group = !x.bwd ? 4 : (x.S.ch == 32 ? 2 : 4);
    return capped((tiles + per_group - 1) / per_group, cap);
}
int cm_regions(const Launch& x, RowIO& io, float**) {
    if (!x.bwd) return CSMPN_OK;
    const size_t pb = cemlp_cm_n3().slice_floats(lane_shape(x)) * sizeof(float) * kClMaxBwdGroups;
    io.rl_partials = reinterpret_cast<float*>(tail_region(x.plan, pb, 16));
    io.handover = x.handover;
    return CSMPN_OK;
}
void cm_label(const Launch& x, const RowIO& io) {
    note_kernel("csmpn::cemlp_%s_kernel<%s, %d, %d, %d, %d%s>", !x.bwd ? "cm_fwd" : (x.S.ch == 32 ? "cmp" : "cmb"), x.A.name, x.S.ch, x.mode,
                x.S.nblk, x.S.na, x.bwd && x.S.ch == 32 ? (io.save_state && x.S.nblk > 1 ? ", true" : ", false") : "");
}

// In dispatch order: the first eligible family whose launcher has the instantiation takes the launch.
const Family kFamilies[] = {
    {"pq", kChannelsAttr, pq_eligible, pq_grid, pq_regions, [](const AlgOps&) { return &cemlp_pq_n3(); }, pq_label},
    {"pg", kChannelsAttr, pg_eligible, pg_grid, pg_regions, [](const AlgOps& A) { return A.pg; }, pg_label},
    {"plw", kChannelsAttr, plw_eligible, plw_grid, plw_regions, [](const AlgOps& A) { return A.plw; }, plw_label},
    {"pl", kI0, pl_eligible, pl_grid, pl_regions, [](const AlgOps& A) { return A.pl; }, pl_label},
    {"cl", kChannelsI0, cl_eligible, cl_grid, cl_regions, [](const AlgOps&) { return &cemlp_cl_n3(); }, cl_label},
    {"cm", kChannelsI0, cm_eligible, cm_grid, cm_regions, [](const AlgOps&) { return &cemlp_cm_n3(); }, cm_label},
};

void debug_line(const Family& F, const Launch& x, unsigned grid, long rows) {
    char shape[64];
    if (F.debug_fields == kI0) snprintf(shape, sizeof(shape), "i0=%d", x.S.i0);
    else snprintf(shape, sizeof(shape), "channels=%d %s=%d", x.S.ch, F.debug_fields == kChannelsAttr ? "attr" : "i0",
                  F.debug_fields == kChannelsAttr ? x.S.na : x.S.i0);
    fprintf(stderr, "[csmpn] %s mode=%d bwd=%d %s grid=%u rows=%ld\n", F.name, x.mode, (int)x.bwd, shape, grid, rows);
}

Launch make_launch(const Plan& plan, int mode, bool bwd, bool tables_ready, const RowIO& io, float* handover) {
    return Launch{plan, alg_ops(plan.id), mode, bwd, tables_ready, stage_shape(plan.C, mode, io), handover};
}
}  // namespace

bool plw_serves(const Plan& plan, int mode, bool bwd, const RowIO& io) {
    return plw_eligible(make_launch(plan, mode, bwd, false, io, nullptr), io);
}

int run_rows(const Plan& plan, int mode, bool bwd, const RowIO& io_in, hipStream_t st, bool need_pack, bool tables_ready,
             SliceSet* deferred) {
    if (deferred) deferred->unit = nullptr;
    if (io_in.rows <= 0) return CSMPN_OK;
    const AlgOps& A = alg_ops(plan.id);
    RowIO io = io_in;
    io.stamps = g_stamps;
    // the caller's saved buffer: where the hand-over rows start, and whether it has state regions at all (no kernel may
    // write state the buffer was not sized for: CSMPN_NO_CM_BWD=1 takes the 32-channel Cl(3,0) regions away)
    const SavedLayout SL = saved_layout(A.n, plan.blocks, plan.C.nblk, io.rows, io.save_state ? CSMPN_FLAG_SAVE_STATE : 0);
    if (!SL.state_ch) io.save_state = 0;
    float* const handover = io.saved ? const_cast<float*>(io.saved) + SL.handover_off : nullptr;
    const Launch x = make_launch(plan, mode, bwd, tables_ready, io, handover);
    for (const Family& F : kFamilies) {
        if (!F.eligible(x, io)) continue;
        const unsigned grid = F.grid(x, io.rows);
        float* tabs = nullptr;
        const int rc = F.regions(x, io, &tabs);
        if (rc) return rc;
        if (sw().debug) debug_line(F, x, grid, io.rows);
        bool handled = false;
        const LaneUnit* const unit = F.unit(A);
        io.defer_sum = (bwd && deferred && unit->sum_slices && io.rl_partials) ? 1 : 0;
        // the 16-row-tile families' weight tables: packed unless the stage's forward left them in this workspace
        HIP_TRY(unit->launch(lane_shape(x), bwd, !(bwd && tables_ready), grid, st, plan.C, io, tabs, &handled));
        if (handled) {
            if (io.defer_sum) *deferred = SliceSet{unit, lane_shape(x), plan.C, io.rl_partials, grid};
            F.kernel_label(x, io);
            return CSMPN_OK;
        }
    }
    if (A.D == 32 && bwd && mode != MODE_PLAIN && io.rows >= 4096 && !sw().quiet) {
        // a D = 32 EGCL stage outside the parity-lane widths: served, but by the general row-tile kernels whose backward
        // spills (4.9-5.8 KB of scratch per lane: DESIGN.md §4.6) - say so once instead of being silently slow
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "[csmpn] note: Cl(5,0) / Cl(4,1) layer with %d channels runs on the general row-tile kernels (slow path: "
                            "their backward spills registers). The parity-lane kernels serve two-block EGCL layers of 8, 16, 24, 28 "
                            "or 32 channels. (CSMPN_QUIET=1 silences this note.)\n", plan.C.b[0].O);
    }
    if (io.row_store && !plan.det_general)
        return fail(CSMPN_ERR_UNSUPPORTED,
                    "CSMPN_FLAG_DETERMINISTIC: this shape is served neither by the lane kernels (Cl(3,0) 8 / 16 channels, "
                    "Cl(5,0) / Cl(4,1) 8 / 16 / 24 / 28 / 32 channels; two blocks with saved block inputs) nor by the deterministic "
                    "form of the general kernels (n <= 3, tiles and gradient mirror resident in LDS)");
    // Per-workgroup copies of the gradient tensors at the end of the workspace: always in deterministic mode, and (round 3)
    // for every backward of the small algebras - the parameter-gradient atomics of ALL row tiles onto one copy were the
    // bulk of the md17-width backward (M32 node stage 1.04 -> 0.53 ms with private copies); CSMPN_NO_SLICED_GRADS=1: off.
    DetSlices det{nullptr, 0, kDetGroups};
    if (bwd && (io.row_store || (!sw().no_sliced && (plan.id == ALG_N2 || plan.id == ALG_N3) && !plan.ps && plan.var != VAR_GLOBAL && !plan.wide))) {
        const int rc = det_slices(plan, io.row_store != 0, det);
        if (rc) return rc;
    }
    if (bwd && plan.C.phased) io.handover = handover;   // hand-over region of the phased backward: behind the saved inputs, laid out like them
    // general row-tile kernels from here on: they read packed weight fragments (the lane kernels above do not)
    if (need_pack) {
        const int rcp = run_pack(plan, st);
        if (rcp) return rcp;
    }
    const long R = 16 * plan.H;
    const long ntiles = (io.rows + R - 1) / R;
    // few tiles (e.g. the node update of a 10k-node complex): fewer row tiles per workgroup,
    // so that the tiles spread over all CUs instead of filling a few of them
    DevCemlp Cd = plan.C;
    unsigned threads = plan.threads;
    size_t lds_bytes = plan.lds_bytes;
    if (plan.var != VAR_GLOBAL && Cd.RT > 1 && !bwd) {   // backward: per-workgroup mirror flush outweighs the spread (measured)
        long rt = (ntiles + 255) / 256;
        if (rt < 1) rt = 1;
        if (rt < Cd.RT) {
            lds_bytes -= (size_t)(Cd.RT - rt) * Cd.tile_floats * 4;
            Cd.RT = (int)rt;
            threads = (unsigned)(Cd.RT * Cd.MT * 64);
        }
    }
    long grid = (ntiles + Cd.RT - 1) / Cd.RT;
    if (grid > (long)plan.grid_cap) grid = plan.grid_cap;
    if (det.base && grid > det.groups) grid = det.groups;
    if (sw().debug && plan.wide)
        fprintf(stderr, "[csmpn] wide mode=%d bwd=%d CT=%d MT=%d threads=%u lds=%zu grid=%ld tile_floats=%d rows=%ld\n", mode, (int)bwd,
                Cd.CT, Cd.MT, threads, lds_bytes, grid, Cd.tile_floats, io.rows);
    else if (sw().debug)
        fprintf(stderr, "[csmpn] mode=%d bwd=%d var=%d ps=%d share=%d phased=%d H=%d MT=%d RT=%d threads=%u lds=%zu grid=%ld tile_floats=%d mirror=%d rows=%ld\n",
                mode, (int)bwd, plan.var, (int)plan.ps, Cd.share_inz, (int)(bwd && Cd.phased), plan.H, Cd.MT, Cd.RT, threads, lds_bytes, grid,
                Cd.tile_floats, Cd.mirror_floats, io.rows);
    if (det.base) {
        const int rc = det_launch_begin(plan, det, grid, Cd, st);
        if (rc) return rc;
    }
    const char* const dir = bwd ? "true" : "false";
    if (plan.wide) {
        HIP_TRY(A.launch_cemlp_wide(mode, bwd, (unsigned)grid, threads, lds_bytes, st, Cd, io));
        note_kernel("csmpn::cemlp_wide_kernel<%s, %d, %s> (%d channel tiles on %d waves, tiles in %s)", A.name, mode, dir, Cd.CT, Cd.MT,
                    Cd.gtiles ? "global scratch" : "LDS");
    } else if (plan.ps) {
        HIP_TRY(A.launch_cemlp_ps(mode, bwd, (unsigned)grid, threads, lds_bytes, st, Cd, io));
        note_kernel("csmpn::cemlp_ps_kernel<%s, %d, %s>", A.name, mode, dir);
    } else {
        HIP_TRY(A.launch_cemlp(mode, plan.var, plan.H, bwd, (unsigned)grid, threads, lds_bytes, st, Cd, io));
        note_kernel("csmpn::cemlp_kernel<%s, %d, %d, %d, %s>", A.name, mode, plan.var, plan.H, dir);
    }
    return det.base ? det_reduce(plan, det, grid, st) : CSMPN_OK;
}

}  // namespace csmpn
