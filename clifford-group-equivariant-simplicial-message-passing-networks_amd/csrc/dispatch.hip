// Kernel families of the CEMLP / EGCL stages, one row of kFamilies each: which launches the family serves, what a launch takes
// at the end of the caller's workspace (TailNeed: read by admission, placement and the reservation of
// csmpn_cemlp_workspace_bytes alike), which regions of the saved buffer belong to it (SavedNeed); the saved-buffer layout
// built from those rows; and run_rows, which walks the table and falls through to the general, parity-split and wide
// row-tile kernels.
#include <atomic>
#include <cstdio>

#include "plan.hpp"

namespace csmpn {
namespace {

// ----------------------------------------------------------------------------- what a family is asked about
// A stage as the sizing entry points see it (no metric, no mode): block 0 reads i0 channels and writes ch; uniform: every
// later block ch -> ch. Computed once per query and once per run_rows call.
struct SizeKey { int n, nblk, ch, i0; bool uniform; };
SizeKey size_key(int n, const csmpn_block_params* blocks, int nblk) {
    SizeKey k{n, nblk, nblk > 0 ? blocks[0].out_features : 0, nblk > 0 ? blocks[0].in_features : 0, nblk > 0};
    for (int j = 1; j < nblk; ++j)
        if (blocks[j].out_features != k.ch || blocks[j].in_features != k.ch) k.uniform = false;
    return k;
}
// the shape of the key's stage under `mode`, as the lane-kernel units key it (launch.hpp)
LaneShape shape_of(int mode, const SizeKey& k) {
    return LaneShape{mode, k.nblk, k.ch, mode == MODE_EDGE ? k.i0 - k.ch : (mode == MODE_NODE ? k.i0 - 2 * k.ch : k.i0)};
}
constexpr int kModes[] = {MODE_EDGE, MODE_NODE, MODE_PLAIN};
bool n3_shape(const SizeKey& k) { return k.n == 3 && k.nblk <= 2 && k.uniform; }                                // Cl(3,0) families
bool d32_shape(const SizeKey& k) { return k.n == 5 && k.nblk <= 2 && k.uniform && k.ch >= 8 && k.ch <= 32; }    // Cl(5,0) / Cl(4,1) families
bool egcl_slices(const LaneUnit& u, const SizeKey& k) {   // the unit's backward serves the key's edge or node stage
    return u.slice_floats(shape_of(MODE_EDGE, k)) || u.slice_floats(shape_of(MODE_NODE, k));
}

// What a launch takes at the end of the workspace: weight tables, their end `pad` bytes before the workspace's and their start
// rounded down to `align`, and the gradient slices of a backward at the family's grid cap directly in front of them (no
// tables: the slices in their place). A launch is admitted where the workspace holds asks() bytes; a reservation is the
// largest asks() over the modes of a stage. All zero: the launch takes nothing.
struct TailNeed {
    size_t table_bytes, slice_bytes, pad, align, slack;
    size_t bytes() const { return table_bytes + slice_bytes; }
    size_t asks() const { return bytes() + slack; }
};
// tables and slices of the table-bearing families and of pl, which shares their region. exact: sizes of the launch's own unit;
// else the channel-count bounds of launch.hpp, where the sizing side has no metric and so no unit to ask
TailNeed padded(size_t table_bytes, size_t slice_bytes, bool exact) {
    return TailNeed{table_bytes, slice_bytes, kTailPad, kTailAlign, exact ? kAdmitSlack : kBoundSlack};
}
float* carve(const Plan& plan, const TailNeed& t, float** tabs) {   // places *tabs, returns the slices
    if (!t.table_bytes) return reinterpret_cast<float*>(tail_region(plan, t.slice_bytes + t.pad, t.align));
    char* const tb = tail_region(plan, t.table_bytes + t.pad, t.align);
    *tabs = reinterpret_cast<float*>(tb);
    return reinterpret_cast<float*>(tb - t.slice_bytes);
}

// The saved-buffer regions of a shape a family claims, in channels per row: the hand-over of d/d(block-1 input) from the
// block-1 launch to the block-0 launch, one [rows, C, D] region behind the saved block inputs (0: none of its own - the
// general kernels' phased slots where the shape has them, at every row count), and the CSMPN_FLAG_SAVE_STATE regions
// (cemlp_device.hpp: whole row tiles in the kernels' lane order, one region per tensor and block, rows rounded up to 16).
struct SavedNeed { bool claimed; size_t handover_ch, state_ch; };

// The stage a launch runs, read off the plan and the input segments once per run_rows call: EGCL edge (I0 = ch + na), EGCL
// node (I0 = 2 ch + na) or a plain CEMLP (na = I0: its input channels).
struct StageShape {
    bool ok;               // EGCL modes: the gathered segments have the layer's width
    int ch, na, i0, nblk;
    bool uniform_width;    // every block ch -> ch (block 0: I0 -> ch)
    bool all_w1_sub;       // every MVLinear weight has one slice per grade
};
StageShape stage_shape(const DevCemlp& C, const SizeKey& k, int mode, const RowIO& io) {
    StageShape S{true, k.ch, k.i0, k.i0, k.nblk, k.uniform, true};
    const int ch = S.ch;
    for (int j = 0; j < C.nblk; ++j)
        if (!C.b[j].w1_sub) S.all_w1_sub = false;
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
    SizeKey key;
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
    bool (*eligible)(const Launch& x, const RowIO& io);   // shape, switches, saved buffer; the workspace is tail's business
    unsigned (*grid)(const Launch& x, long rows);
    // the instantiation unit that launches (null: the algebra has none). A null: the sizing side, which has no metric - the
    // Cl(3,0) families answer with their one unit, the D = 32 families with none
    const LaneUnit* (*unit)(const AlgOps* A);
    TailNeed (*tail)(const LaneUnit* u, const LaneShape& s, bool bwd);
    float* RowIO::*slices;          // where the kernels look for the slices
    const char* too_small;          // a workspace below tail's asks(): this error (null: the family declines)
    bool (*reserves)(const SizeKey& k);    // the stages csmpn_cemlp_workspace_bytes reserves tail's asks() for
    SavedNeed (*saved)(const SizeKey& k);  // null: no saved-buffer regions of its own
    int handover_blocks;            // a backward of at least this many blocks gets the hand-over rows (0: none does)
    void (*kernel_label)(const Launch& x, const RowIO& io);
};

// 16-row-tile MFMA-mixing kernels for Cl(3,0) (cemlp_pq.hpp): two blocks of 32 channels, EGCL edge / node programs, and the
// standalone one- / two-block CEMLPs of the md17 model (embeddings and head). CSMPN_NO_PQ=1 and CSMPN_NO_CM=1 leave their
// shapes to the channel-MFMA and the general kernels.
bool pq_on() { return !sw().no_pq && !sw().no_cm; }
bool pq_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (!pq_on() || x.plan.id != ALG_N3) return false;
    if (S.nblk != 2 && !(S.nblk == 1 && x.mode == MODE_PLAIN)) return false;
    if (S.ch != 32 || !S.uniform_width || !S.all_w1_sub || !S.ok) return false;
    // standalone CEMLP: one contiguous input of I0 channels; not the fused embedding
    if (x.mode == MODE_PLAIN && (io.nseg != 1 || io.emb_nperm != 0 || io.seg[0].ch != S.i0)) return false;
    if (!cemlp_pq_n3().table_floats(lane_shape(x))) return false;
    // the backward runs on the state its forward saved (CSMPN_FLAG_SAVE_STATE, in ITS lane order; run_rows honours the flag
    // only where the saved buffer has state regions: pq_saved, cm_saved); without the flag the forward still serves (it
    // writes the row-major block-1 inputs) and the wave-pair backward (cemlp_cmp.hpp) recomputes
    return !x.bwd || (io.saved && io.save_state);
}
unsigned pq_grid(const Launch&, long rows) {
    // one 16-row tile per workgroup iteration, three 4-wave workgroups per CU (backward: a workgroup ends with one slice of
    // weight-gradient tiles, 62-78 KB; measured with 1 / 2 / 3 tiles per workgroup on launches below the cap: md17 step
    // 2.11 / 2.28 / 2.43 ms, M32 1.024 / 1.008 / 1.012e8 edges/s: one tile)
    return capped((rows + 15) / 16, kPqGridCap);
}
// weight-fragment tables + one gradient slice per workgroup, both as the unit states them
TailNeed pq_tail(const LaneUnit* u, const LaneShape& s, bool) {
    const size_t tf = u->table_floats(s);
    return tf ? padded(tf * sizeof(float), u->slice_floats(s) * sizeof(float) * kPqGridCap, true) : TailNeed{};
}
// the standalone CEMLPs (MODE_PLAIN): s, y, R of every block; a two-block one hands over through the phased slot. (The EGCL
// shapes' regions are the channel-MFMA family's, whose backward serves them without save-state: cm_saved.)
SavedNeed pq_saved(const SizeKey& k) {
    if (!pq_on() || sw().no_cm_bwd || !n3_shape(k) || k.ch != 32 || !cemlp_pq_n3().table_floats(shape_of(MODE_PLAIN, k))) return {};
    return {true, 0, (size_t)3 * k.nblk * 32};
}
void pq_label(const Launch& x, const RowIO&) {
    note_kernel("csmpn::cemlp_pq_%s_kernel<%s, ...> (mode %d, %d channels, %d %s channels, %d block%s)", x.bwd ? "bwd" : "fwd", x.A.name,
                x.mode, x.S.ch, x.S.na, x.mode == MODE_PLAIN ? "input" : "attribute", x.S.nblk, x.S.nblk > 1 ? "s" : "");
}

// 16-row-tile MFMA-mixing kernels (cemlp_pg.hpp): Cl(5,0) / Cl(4,1), two blocks of 24 / 28 / 32 channels, EGCL edge / node programs
bool pg_eligible(const Launch& x, const RowIO& io) {
    const StageShape& S = x.S;
    if (sw().no_pg || !x.A.pg || !two_uniform_blocks(x) || S.ch <= 16 || S.ch > 32 || !egcl(x)) return false;
    if (!x.A.pg->table_floats(lane_shape(x))) return false;
    // the backward of this family runs on the state its forward saved (CSMPN_FLAG_SAVE_STATE, in ITS lane order): without
    // the flag the forward still serves (it writes the row-major block-1 inputs every backward reads) and the wide
    // parity-lane backward recomputes from them
    return !x.bwd || (io.saved && io.save_state);
}
unsigned pg_grid(const Launch&, long rows) { return capped((rows + 15) / 16, kPgGridCap); }   // one 16-row tile per workgroup iteration, one 8-wave workgroup per CU
// A launch's own tables may exceed the bound the reservation is made of by pg_tables_overshoot(channels) (launch.hpp; asserted
// in pg_inst.inc) and then reach into the front part of the workspace, which admission counts in: DESIGN.md section 6, gap 9.
TailNeed pg_tail(const LaneUnit* u, const LaneShape& s, bool) {
    return padded(u ? u->table_floats(s) * sizeof(float) : pg_tables_bytes(s.channels), pg_part_bytes(s.channels), u != nullptr);
}
bool pg_reserves(const SizeKey& k) { return d32_shape(k) && k.ch > 16; }   // by channel count, whatever the attribute width
// s, y, R of both blocks at 32 channels: the kernels keep 4 channels per wave, 8 waves per tile
SavedNeed pg_saved(const SizeKey& k) { return pg_reserves(k) && k.nblk == 2 ? SavedNeed{true, (size_t)k.ch, 3 * 2 * 32} : SavedNeed{}; }
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
    if (!x.A.plw->table_floats(lane_shape(x))) return false;
    return !(x.bwd && S.nblk > 1 && !io.saved);
}
unsigned plw_grid(const Launch& x, long rows) {
    const long per_cu = 4 / ((x.S.ch + 7) / 8) > 0 ? 4 / ((x.S.ch + 7) / 8) : 1;   // workgroups of NG waves per CU at one wave per SIMD
    // one 4-row tile per workgroup iteration; forward: twice the workgroups where LDS allows
    return capped((rows + 3) / 4, (x.bwd ? kPlwMaxGroups : 2 * kPlwMaxGroups) * per_cu);
}
// rotation tables + one gradient slice per workgroup (the slices by the bound also at a launch)
TailNeed plw_tail(const LaneUnit* u, const LaneShape& s, bool) {
    return padded(u ? u->table_floats(s) * sizeof(float) : plw_tables_bytes(s.channels), plw_part_bytes(s.channels), u != nullptr);
}
// by channel count, whatever the attribute width; 8 channels included: the reservation and the regions of the parity-lane family
bool plw_reserves(const SizeKey& k) { return d32_shape(k); }
// s, y, R of both blocks, channels padded to groups of 8
SavedNeed plw_saved(const SizeKey& k) {
    return d32_shape(k) && k.nblk == 2 ? SavedNeed{true, (size_t)k.ch, (size_t)3 * 2 * ((k.ch + 7) / 8 * 8)} : SavedNeed{};
}
void plw_label(const Launch& x, const RowIO&) {   // the wide kernels' template arguments live in plw_inst.inc: family + shape
    note_kernel("csmpn::cemlp_plw_%s_kernel<%s, ...> (mode %d, %d channels, %d attribute channels, %d blocks)", x.bwd ? "bwd" : "fwd",
                x.A.name, x.mode, x.S.ch, x.S.na, x.S.nblk);
}

// parity-lane kernels (cemlp_pl.hpp): Cl(5,0) / Cl(4,1), two blocks of 8 channels, the EGCL attribute widths of S3. Their saved
// buffer is the wide family's at 8 channels (plw_saved: the same regions), and so is the larger reservation.
bool pl_eligible(const Launch& x, const RowIO& io) {
    if (sw().no_pl || !x.A.pl || !two_uniform_blocks(x) || x.S.ch != 8 || !egcl(x)) return false;
    if (x.bwd && !io.saved) return false;
    return serves(*x.A.pl, lane_shape(x));
}
unsigned pl_grid(const Launch& x, long rows) {
    const long tiles = (rows + 3) / 4;   // 4 rows per wave tile; one / two 4-wave workgroups per CU
    return capped((tiles + 3) / 4, x.bwd ? kPlMaxBwdGroups : 512);
}
// per-wave slices of parameter-gradient sums, by the bound; the forward takes nothing
TailNeed pl_tail(const LaneUnit* u, const LaneShape&, bool bwd) { return bwd ? padded(0, pl_part_bytes(), u != nullptr) : TailNeed{}; }
bool pl_reserves(const SizeKey& k) { return d32_shape(k) && k.nblk == 2 && k.ch == 8; }
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
    return x.mode != MODE_EDGE || (io.gather_rows > 0 && cl_array_fits(io.gather_rows, row_floats));
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
// the backward's partial sums: one slice per workgroup as the unit states it, 16-byte aligned, nothing else. The channel-MFMA
// backwards (cemlp_cmb.hpp / cemlp_cmp.hpp) share the region and its slice layout: cm's row reads this function too.
TailNeed cl_tail(const LaneUnit* u, const LaneShape& s, bool bwd) {
    return bwd ? TailNeed{0, u->slice_floats(s) * sizeof(float) * kClMaxBwdGroups, 0, 16, 0} : TailNeed{};
}
// s of both blocks
SavedNeed cl_saved(const SizeKey& k) {
    return n3_shape(k) && k.nblk == 2 && egcl_slices(cemlp_cl_n3(), k) ? SavedNeed{true, (size_t)k.ch, (size_t)2 * k.ch} : SavedNeed{};
}
void cl_label(const Launch& x, const RowIO& io) {
    note_kernel("csmpn::cemlp_cl_%s_kernel<%s, %d, %d, %d, %d%s>", x.bwd ? "bwd" : "fwd", x.A.name, x.S.ch, x.mode, x.S.nblk, x.S.na,
                !x.bwd ? "" : (io.save_state ? ", true" : ", false"));
}

// channel-MFMA kernels (cemlp_cm.hpp): Cl(3,0), two blocks of 16 channels (S2) or 32 channels (md17), the EGCL attribute
// widths (6, 3). CSMPN_NO_CM=1 leaves these shapes to the general kernels (A/B measurements, parity tests of both paths);
// CSMPN_NO_CM_BWD=1 their backward only, and with it their saved-buffer regions: the backward runs where cm_saved claims them.
SavedNeed cm_saved(const SizeKey& k) {   // 32 channels (cemlp_cmp.hpp, cemlp_pq.hpp): s, y, R of both blocks; 16: no state
    if (sw().no_cm_bwd || !n3_shape(k) || k.nblk != 2 || !egcl_slices(cemlp_cm_n3(), k)) return {};
    return {true, (size_t)k.ch, k.ch == 32 ? (size_t)3 * 2 * 32 : 0};
}
bool cm_eligible(const Launch& x, const RowIO& io) {
    if (sw().no_cm || x.plan.id != ALG_N3 || !two_uniform_blocks(x) || !egcl(x)) return false;
    if (x.bwd && !io.saved) return false;
    if (!serves(cemlp_cm_n3(), lane_shape(x))) return false;
    return !x.bwd || cm_saved(x.key).claimed;
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
void cm_label(const Launch& x, const RowIO& io) {
    note_kernel("csmpn::cemlp_%s_kernel<%s, %d, %d, %d, %d%s>", !x.bwd ? "cm_fwd" : (x.S.ch == 32 ? "cmp" : "cmb"), x.A.name, x.S.ch, x.mode,
                x.S.nblk, x.S.na, x.bwd && x.S.ch == 32 ? (io.save_state && x.S.nblk > 1 ? ", true" : ", false") : "");
}

// In dispatch order: the first eligible family whose launcher has the instantiation takes the launch.
// Only one of the Cl(3,0) and one of the D = 32 families can take a stage, so a reservation is the largest of the rows'.
const Family kFamilies[] = {
    {"pq", kChannelsAttr, pq_eligible, pq_grid, [](const AlgOps*) { return &cemlp_pq_n3(); }, pq_tail, &RowIO::slices, nullptr, n3_shape,
     pq_saved, 1, pq_label},
    {"pg", kChannelsAttr, pg_eligible, pg_grid, [](const AlgOps* A) { return A ? A->pg : nullptr; }, pg_tail, &RowIO::slices, nullptr,
     pg_reserves, pg_saved, 1, pg_label},
    {"plw", kChannelsAttr, plw_eligible, plw_grid, [](const AlgOps* A) { return A ? A->plw : nullptr; }, plw_tail, &RowIO::slices, nullptr,
     plw_reserves, plw_saved, 2, plw_label},
    {"pl", kI0, pl_eligible, pl_grid, [](const AlgOps* A) { return A ? A->pl : nullptr; }, pl_tail, &RowIO::slices,
     "workspace too small for the parity-lane backward", pl_reserves, nullptr, 0, pl_label},
    {"cl", kChannelsI0, cl_eligible, cl_grid, [](const AlgOps*) { return &cemlp_cl_n3(); }, cl_tail, &RowIO::rl_partials, nullptr, n3_shape,
     cl_saved, 1, cl_label},
    {"cm", kChannelsI0, cm_eligible, cm_grid, [](const AlgOps*) { return &cemlp_cm_n3(); }, cl_tail, &RowIO::rl_partials, nullptr, n3_shape,
     cm_saved, 1, cm_label},
};

SavedNeed family_saved(const SizeKey& k) {   // of the first family that claims the shape
    for (const Family& F : kFamilies) {
        const SavedNeed s = F.saved ? F.saved(k) : SavedNeed{};
        if (s.claimed) return s;
    }
    return {};
}
}  // namespace

// ----------------------------------------------------------------------------- sizing: workspace tail and saved buffer
size_t family_tail_bytes(int n, const csmpn_block_params* blocks, int nblk) {
    const SizeKey k = size_key(n, blocks, nblk);
    size_t best = 0;
    for (const Family& F : kFamilies)
        for (int mode : kModes) {
            const size_t b = F.reserves(k) ? F.tail(F.unit(nullptr), shape_of(mode, k), true).asks() : 0;
            best = b > best ? b : best;
        }
    return best;
}

// the standalone CEMLPs whose saved buffer has state regions: capi.hip honours CSMPN_FLAG_SAVE_STATE for them
bool pq_plain_shape(int n, const csmpn_block_params* blocks, int nblk) { return nblk >= 1 && pq_saved(size_key(n, blocks, nblk)).claimed; }

// Shapes whose backward may run block by block on the general kernels (cemlp_kernel.hpp, `phased`): small algebras, more
// than one block, no lane-kernel family with a hand-over region of its own. They get a hand-over region as large as the
// saved inputs behind them.
bool general_phased_shape(int n, const csmpn_block_params* blocks, int nblk) {
    if (n > 3 || nblk < 2 || nblk > CSMPN_MAX_BLOCKS) return false;
    for (int k = 0; k < nblk; ++k)
        if (blocks[k].out_features > 64) return false;   // the wide kernel has no LDS mirror to shrink: no phased form
    return !family_saved(size_key(n, blocks, nblk)).handover_ch;
}

SavedLayout saved_layout(int n, const csmpn_block_params* blocks, int nblk, int64_t rows, uint32_t flags) {
    SavedLayout L{};
    for (int k = 0; k + 1 < nblk; ++k) L.inputs_ch += (size_t)blocks[k].out_features;
    // The general kernels' phased backward has one hand-over slot per saved input; make_plan takes that form only from
    // sw().phased_min_rows rows on (the same switch, read once), a family that claims the shape without a region of its
    // own (pq_saved) hands over through it at every row count.
    const SavedNeed s = family_saved(size_key(n, blocks, nblk));
    if (s.handover_ch) L.handover_ch = s.handover_ch;
    else if (general_phased_shape(n, blocks, nblk) && (rows < 0 || rows >= sw().phased_min_rows || s.claimed)) L.handover_ch = L.inputs_ch;
    if (rows < 0 || (flags & CSMPN_FLAG_SAVE_STATE)) L.state_ch = s.state_ch;
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

// ----------------------------------------------------------------------------- run_rows
namespace {
void debug_line(const Family& F, const Launch& x, unsigned grid, long rows) {
    char shape[64];
    if (F.debug_fields == kI0) snprintf(shape, sizeof(shape), "i0=%d", x.S.i0);
    else snprintf(shape, sizeof(shape), "channels=%d %s=%d", x.S.ch, F.debug_fields == kChannelsAttr ? "attr" : "i0",
                  F.debug_fields == kChannelsAttr ? x.S.na : x.S.i0);
    fprintf(stderr, "[csmpn] %s mode=%d bwd=%d %s grid=%u rows=%ld\n", F.name, x.mode, (int)x.bwd, shape, grid, rows);
}

Launch make_launch(const Plan& plan, int mode, bool bwd, bool tables_ready, const RowIO& io, float* handover) {
    const AlgOps& A = alg_ops(plan.id);
    const SizeKey k = size_key(A.n, plan.blocks, plan.C.nblk);
    return Launch{plan, A, mode, bwd, tables_ready, k, stage_shape(plan.C, k, mode, io), handover};
}
}  // namespace

bool plw_serves(const Plan& plan, int mode, bool bwd, const RowIO& io) {
    const Launch x = make_launch(plan, mode, bwd, false, io, nullptr);
    return plw_eligible(x, io) && fits(plan, plw_tail(x.A.plw, lane_shape(x), bwd).asks());
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
        const LaneUnit* const unit = F.unit(&A);
        const TailNeed t = F.tail(unit, lane_shape(x), bwd);
        if (t.bytes() && !fits(plan, t.asks())) {
            if (!F.too_small) continue;
            return fail(CSMPN_ERR_INVALID, "%s", F.too_small);
        }
        const unsigned grid = F.grid(x, io.rows);
        float* tabs = nullptr;
        if (t.bytes()) io.*F.slices = carve(plan, t, &tabs);
        if (bwd && F.handover_blocks && x.S.nblk >= F.handover_blocks) io.handover = handover;
        if (sw().debug) debug_line(F, x, grid, io.rows);
        bool handled = false;
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
