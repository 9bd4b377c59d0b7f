// Host side of the CEMLP / EGCL entry points, shared by capi.hip (C-ABI), plan.hip (LDS / tile planner of the general and
// wide kernels) and dispatch.hip (kernel families, buffer layout, run_rows).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/csmpn_hip.h"
#include "capi_common.hpp"
#include "cemlp_kernel.hpp"
#include "launch.hpp"

#define fail csmpn_fail

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(CSMPN_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace csmpn {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int rup(int a, int b) { return cdiv(a, b) * b; }

// Every environment switch of the library, read ONCE per process (capi.hip). They select kernel families for A/B measurements
// and parity tests of the slower paths or bound a launch for experiments; none of them changes results beyond summation
// order. Documented in INTEGRATION.md ("Debug switches").
struct Switches {
    bool no_cl;          // CSMPN_NO_CL=1       Cl(3,0) 8-channel layers leave the (row, channel)-per-lane kernels (cemlp_cl.hpp) for the general ones
    bool no_cm;          // CSMPN_NO_CM=1       16 / 32-channel Cl(3,0) layers leave the channel-MFMA kernels (cemlp_cm*.hpp)
    bool no_cm_bwd;      // CSMPN_NO_CM_BWD=1   ... their backward only (forward stays). The size of the saved region the caller allocates depends on it
    bool no_pl;          // CSMPN_NO_PL=1       8-channel Cl(5,0) / Cl(4,1) layers leave the parity-lane kernels (cemlp_pl.hpp)
    bool no_plw;         // CSMPN_NO_PLW=1      wide Cl(5,0) / Cl(4,1) layers leave the wide parity-lane kernels (cemlp_plw.hpp)
    bool plw8;           // CSMPN_PLW8=1        8 channels on the wide parity-lane kernels with one group
    bool no_pg;          // CSMPN_NO_PG=1       24 / 28 / 32-channel Cl(5,0) / Cl(4,1) layers leave the 16-row-tile MFMA-mixing kernels (cemlp_pg.hpp)
    bool no_pq;          // CSMPN_NO_PQ=1       32-channel Cl(3,0) layers leave the 16-row-tile MFMA-mixing kernels (cemlp_pq.hpp) for the channel-MFMA ones
    bool no_share;       // CSMPN_NO_SHARE=1    general kernels: z does not alias the input tile
    bool no_phased;      // CSMPN_NO_PHASED=1   general kernels: backward of all blocks per tile instead of block by block
    bool no_sliced;      // CSMPN_NO_SLICED_GRADS=1  general kernels: parameter-gradient atomics onto one copy
    bool debug;          // CSMPN_DEBUG         one line per launch on stderr: family, mode, shape, grid
    bool quiet;          // CSMPN_QUIET         no note when a D = 32 layer runs on the general kernels
    int force_ps;        // CSMPN_FORCE_PS=0|1  parity-split layout of the general kernels off / on (-1: by algebra)
    int force_h;         // CSMPN_FORCE_H=1|2   row halves per tile of the general kernels (0: by row count)
    int min_lds_tiles;   // CSMPN_MIN_LDS_TILES resident row tiles below which the general kernels leave the LDS variant
    long phased_min_rows;   // CSMPN_PHASED_MIN_ROWS  rows from which the phased backward is taken (default 4096)
    long cl_cap_fwd, cl_cap_bwd;   // CSMPN_CL_CAP_FWD / _BWD  fewer resident workgroups of the cl kernels (experiments)
};
const Switches& sw();
void note_kernel(const char* fmt, ...);   // name of the kernel the calling thread dispatched last (csmpn_last_kernel)
extern unsigned long long* g_stamps;      // diagnostic builds: device buffer of cycle accumulators

// ----------------------------------------------------------------------------- compiled algebras
enum AlgId { ALG_NONE = -1, ALG_N2, ALG_N3, ALG_N4, ALG_N5, ALG_N5M, ALG_N4M, ALG_COUNT };
AlgId alg_id(const float* metric, int n);

// What the host needs of one compiled algebra; the D = 32 families (pl, plw, pg) are null elsewhere.
struct AlgOps {
    int n, D, paths;
    bool h2, ps;         // has 32-row-tile (H = 2) / parity-split instantiations of the general kernels
    const char* name;
    hipError_t (*launch_cemlp)(int mode, int var, int h, bool bwd, unsigned grid, unsigned block, size_t lds, hipStream_t st,
                               const DevCemlp& C, const RowIO& io);
    hipError_t (*launch_cemlp_ps)(int mode, bool bwd, unsigned grid, unsigned block, size_t lds, hipStream_t st, const DevCemlp& C,
                                  const RowIO& io);
    hipError_t (*launch_cemlp_wide)(int mode, bool bwd, unsigned grid, unsigned block, size_t lds, hipStream_t st, const DevCemlp& C,
                                    const RowIO& io);
    hipError_t (*launch_gp)(bool bwd, const float* a, const float* b, const float* gout, float* out, float* ga, float* gb, long rows,
                            hipStream_t st);
    const LaneUnit *pl, *plw, *pg;   // parity-lane, wide parity-lane, 16-row-tile MFMA-mixing units
};
const AlgOps& alg_ops(AlgId id);

// ----------------------------------------------------------------------------- planner of the general and wide kernels (plan.hip)
struct Plan {
    AlgId id;
    const csmpn_block_params* blocks;   // the caller's blocks (C holds their device view)
    DevCemlp C;
    PackDesc P;
    size_t pack_f4;       // f4 elements of packed weights
    unsigned threads;
    size_t lds_bytes;
    unsigned grid_cap;    // workgroups that fit on the chip at once
    int var;              // VAR_WAVE / VAR_GROUP / VAR_GROUP_NM / VAR_GLOBAL
    int H;                // row halves per tile
    bool ps;              // parity-split kernels (cemlp_ps.hpp): 16-row tiles, 8 channels x 2 blade parities
    bool det_general;     // deterministic mode on the general row-tile kernels: one row tile per workgroup, mirror slices
    bool wide;            // 65..256 output channels: the wide row-tile kernel (cemlp_wide.hpp), CT channel tiles on MT waves
    void* workspace;      // the caller's workspace (packed weights in front, the families' regions at its end)
    size_t workspace_bytes;
};
// bwd / stage_rowlen decide the footprint. stage_rowlen: dense staging row length needed in buf_g (edge forward scatter).
int make_plan(AlgId id, const csmpn_block_params* blocks, const csmpn_block_grads* grads, int nblk, void* workspace,
              size_t workspace_bytes, bool bwd, int stage_rowlen, bool use_saved, long rows, Plan& plan, bool deterministic = false);
int run_pack(const Plan& plan, hipStream_t st);
// bytes of packed weights + global tile scratch the general / wide kernels may need in front of the workspace, over the
// entry points and both directions (no metric: upper bound)
size_t plan_front_bytes(int n, const csmpn_block_params* blocks, int nblk);

// A region carved from the END of the workspace: `bytes` long, start rounded down to `align` (a power of two).
inline char* tail_region(const Plan& plan, size_t bytes, size_t align) {
    return static_cast<char*>(plan.workspace) + ((plan.workspace_bytes - bytes) & ~(align - 1));
}
// A lane family's tables and slices (TailNeed of dispatch.hip) end kTailPad bytes, one float4 of margin, before the end of
// the workspace and start on a multiple of kTailAlign, the tables' alignment for the kernels' vector loads: with the start
// rounded down, the region reaches less than kTailSlack further from the end than its own bytes. The sizing side
// (csmpn_cemlp_workspace_bytes) reserves bytes + kTailSlack behind the front part for whichever region a launch takes.
constexpr size_t kTailPad = 16, kTailAlign = 256;
constexpr size_t kTailSlack = kTailPad + kTailAlign;
// What a launch asks of the workspace beyond its tables and slices before it carves them: kTailSlack rounded up to 1 KB.
constexpr size_t kAdmitSlack = 1024;
// What a reservation stated by launch.hpp's channel-count bounds adds to them: one more alignment step.
constexpr size_t kBoundSlack = kTailAlign;

// The ten parameter-gradient tensors of block B in reference order: f(pointer slot, floats, present). G grades, P paths.
template <class Block, class F>
inline void for_each_grad_tensor(Block& B, int G, int P, F&& f) {
    f(B.gW1, (B.w1_sub ? G : 1) * B.O * B.I, true); f(B.gWR, G * B.O * B.O, true); f(B.gWL, G * B.O * B.O, true);
    f(B.gb1, B.O, B.has_b1 != 0); f(B.gsa, B.O * G, true); f(B.gsb, B.O * G, true); f(B.gw, B.O * P, true);
    f(B.gan, B.O * G, true); f(B.gbL, B.O, true); f(B.gla, B.O, true);
}
// floats of one copy of all blocks' gradient tensors (each block rounded up to 4): the LDS mirror and a deterministic slice
int mirror_total(int G, int P, const csmpn_block_params* blocks, int nblk);

// Per-workgroup copies of the gradient tensors at the end of the workspace (deterministic mode, and every backward of the
// small algebras): det_reduce adds the copies in a fixed order.
constexpr int kDetGroups = 512;
struct DetSlices {
    float* base;      // null: no copies (atomics onto the one copy)
    int floats;       // of one copy
    int groups;       // copies = most workgroups of the launch
};
size_t det_slice_bytes(int n, const csmpn_block_params* blocks, int nblk);   // reserved for them
int det_slices(const Plan& plan, bool required, DetSlices& S);
int det_launch_begin(const Plan& plan, const DetSlices& S, long grid, DevCemlp& Cd, hipStream_t st);   // zero the copies, point Cd's gradients at copy 0
int det_reduce(const Plan& plan, const DetSlices& S, long grid, hipStream_t st);

// ----------------------------------------------------------------------------- families and buffer layout (dispatch.hip)
// The saved buffer of one CEMLP launch, in channels (x D floats per row): the inputs of blocks 1.., the hand-over region(s)
// of the block-by-block backwards, the CSMPN_FLAG_SAVE_STATE regions (whole 16-row tiles). rows < 0: the per-row upper bound.
struct SavedLayout {
    size_t inputs_ch, handover_ch, state_ch;
    size_t handover_off, state_off, total;   // floats
};
SavedLayout saved_layout(int n, const csmpn_block_params* blocks, int nblk, int64_t rows, uint32_t flags);
bool pq_plain_shape(int n, const csmpn_block_params* blocks, int nblk);
bool general_phased_shape(int n, const csmpn_block_params* blocks, int nblk);
size_t family_tail_bytes(int n, const csmpn_block_params* blocks, int nblk);   // the lane families' region at the end of the workspace

// tables_ready: CSMPN_FLAG_WEIGHTS_PACKED on a backward entry point - the weight-fragment tables of the 16-row-tile families,
// written by the stage's forward into the same workspace, are still there and the backward does not pack again.
// deferred (a backward; may be null): where the family's unit can leave its slice sum to the caller (LaneUnit::sum_slices) it
// does, and *deferred says what is left to sum; deferred->unit stays null where the launch left complete gradients.
int run_rows(const Plan& plan, int mode, bool bwd, const RowIO& io_in, hipStream_t st, bool need_pack, bool tables_ready = false,
             SliceSet* deferred = nullptr);
// the fused embedding is served by the wide parity-lane kernels only
bool plw_serves(const Plan& plan, int mode, bool bwd, const RowIO& io);

}  // namespace csmpn
