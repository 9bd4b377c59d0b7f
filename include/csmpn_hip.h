/* csmpn_hip.h — C-ABI of the MI355X (gfx950) implementation of the Clifford
 * geometric-product / CEMLP / shared simplicial message-passing hot path.
 *
 * The reference exposes this path as a PyTorch nn.Module surface, not an FFI;
 * each entry point below cites the reference interface it replaces
 * (paths relative to the reference repository root):
 *
 *   csmpn_algebra_tables      CliffordAlgebra.__init__ / construct_gmt /
 *                             geometric_product_paths
 *                             (csmpn/algebra/cliffordalgebra.py:11-42,238-252,
 *                              csmpn/algebra/metric.py:18-120)
 *   csmpn_geometric_product_* CliffordAlgebra.geometric_product
 *                             (csmpn/algebra/cliffordalgebra.py:44-54), full-blade form
 *   csmpn_cemlp_*             CEMLP.forward and autograd through it: MVLinear,
 *                             MVSiLU, SteerableGeometricProductLayer (+ Normalization-
 *                             Layer), MVLayerNorm (csmpn/models/cegnn_utils.py:34-213,287-338)
 *   csmpn_egcl_*              EGCL.forward = PyG propagate: gather h_i/h_j, message
 *                             (edge CEMLP), scatter sum|mean over edge_index[1],
 *                             update (node CEMLP + residual)
 *                             (csmpn/models/cegnn_utils.py:216-284)
 *   csmpn_csr_build           the sort PyG/torch_scatter do not need but the
 *                             segmented scatter here does; one-time per complex
 *
 * Conventions: extern "C", plain pointers and sizes, int status return
 * (0 = ok, non-zero = error, message via csmpn_last_error()). All data
 * pointers are DEVICE pointers to contiguous fp32 (indices int32) unless a
 * parameter says "host". Every launch is asynchronous on the caller-supplied
 * hipStream_t (passed as void*). No entry point allocates device memory: the
 * caller provides the workspace (csmpn_*_workspace_bytes). Parameter tensors
 * are read in the reference's own state_dict layouts;
 * gradient tensors are ACCUMULATED (+=) in the same layouts and must be
 * zero-initialised by the caller when a fresh gradient is wanted.
 */
#ifndef CSMPN_HIP_H
#define CSMPN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSMPN_MAX_BLOCKS 4
#define CSMPN_OK 0
#define CSMPN_ERR_UNSUPPORTED 1
#define CSMPN_ERR_INVALID 2
#define CSMPN_ERR_HIP 3

/* flags of the compute entry points */
#define CSMPN_FLAG_NO_VALIDATE 2u    /* csmpn_csr_build, csmpn_embed_cemlp_*: skip the (synchronous) range check of the index table */
#define CSMPN_FLAG_WEIGHTS_PACKED 1u /* forward entry points: the workspace already holds this
                                       CEMLP's packed weights (left there by an earlier forward with
                                       the same parameters): skip the pack kernel. csmpn_egcl_edge_backward /
                                       csmpn_egcl_node_backward: the workspace is the one the stage's FORWARD
                                       ran on, with the same parameters and untouched since - the 16-row-tile
                                       kernel families (Cl(5,0) / Cl(4,1) at 24-32 channels, Cl(3,0) at 32) then
                                       reuse the weight-fragment tables that forward packed; every other
                                       backward packs for its own tile layout and ignores the flag. */

#define CSMPN_FLAG_DETERMINISTIC 4u  /* csmpn_egcl_edge_forward/backward: no float atomics. The edge rows are
                                       not scattered: `agg` (forward) / `gh` (backward) is an [E, C, D] table in
                                       SORTED edge order, to be summed by csmpn_segment_reduce in a fixed order
                                       (the reference runs under torch.use_deterministic_algorithms(True),
                                       engineer/utils/seed.py:30). Honoured by the kernels whose parameter-gradient
                                       sums are atomic-free: Cl(3,0) with 8 or 16 channels, Cl(5,0) / Cl(4,1) with
                                       8 / 16 / 24 / 28 / 32 channels (two blocks, saved block inputs) and, since round 3,
                                       every Cl(2,0) / Cl(3,0) shape on the general kernels (one row tile per workgroup,
                                       per-workgroup copies of the gradient tensors + fixed-order sums; slower than the
                                       default), 65..256 channels included (at most max(128 MiB, 16 copies) of them).
                                       Every other shape returns CSMPN_ERR_UNSUPPORTED. Also accepted by
                                       csmpn_egcl_node_forward/backward and csmpn_cemlp_forward/backward, where it only
                                       selects the atomic-free parameter sums.
                                       Deterministic coverage of the library (same inputs -> same bits, run after run):
                                         - the EGCL stages and csmpn_egcl_backward with this flag, on the shapes above;
                                         - standalone CEMLPs (csmpn_cemlp_forward/backward) with this flag, on the same shapes;
                                         - csmpn_embed_cemlp_forward/backward WITHOUT any flag: the wide parity-lane kernels
                                           sum the vertex orders in registers, map tiles to workgroups statically and add
                                           their parameter gradients from per-workgroup slices in a fixed order - nothing
                                           in that path depends on the order of arrival, so the entry points take no such flag;
                                         - csmpn_mvlinear_backward_det and csmpn_type_attr_backward_det (entry points of
                                           their own: they need scratch the plain forms do not take); every forward,
                                           csmpn_mvlinear_backward's d/dx, csmpn_simplex_rows, csmpn_segment_reduce and the
                                           readout entry points have fixed-order sums as they are;
                                         - the four standalone small layers through csmpn_mvsilu_backward_det,
                                           csmpn_mvnorm_backward_det, csmpn_mvlayernorm_forward_det / _backward_det and
                                           csmpn_wgp_backward_det (the other forwards of these layers work lane by lane).
                                       The plain forms csmpn_mvsilu_backward, csmpn_mvnorm_backward, csmpn_mvlayernorm_forward /
                                       _backward, csmpn_wgp_backward, csmpn_mvlinear_backward and csmpn_type_attr_backward add
                                       their parameter gradients (MVLayerNorm: also the row sums) with float atomics. */
#define CSMPN_FLAG_SAVE_STATE 8u     /* csmpn_egcl_{edge,node}_{forward,backward}, csmpn_embed_cemlp_{forward,backward} (two-block
                                      * modules), round 4; csmpn_cemlp_{forward,backward}, round 5, for the standalone Cl(3,0) CEMLPs
                                      * of 32 channels the 16-row-tile family serves (1 or 2 blocks; 32, 60 or 90 input channels:
                                      * csmpn_cemlp_saved_floats(..., CSMPN_FLAG_SAVE_STATE) > the size without the flag tells)
                                      * and ignored by them for every other shape: the forward ALSO stores, per block,
                                      * what the backward would otherwise recompute, in "state regions" behind the saved block
                                      * inputs and the hand-over region (csmpn_cemlp_saved_floats sizes them), and the backward
                                      * called with the same flag reads them:
                                      *   Cl(3,0), 8 channels: s = the block's output in front of its layer norm - no linear_left
                                      *     mix, no geometric product in the recompute (S1: edge forward +2.5 us, edge backward
                                      *     -6.5 us; y and R as well: measured a wash there);
                                      *   Cl(3,0), 32 channels and Cl(5,0) / Cl(4,1), 8 .. 32 channels: y (MVLinear output), R
                                      *     (linear_right output) and s - no channel mix and no geometric product at all in the
                                      *     recompute; these kernels run at 5-10 % of the HBM roofline, the extra rows travel
                                      *     under the arithmetic.
                                      * The state regions are private to the kernels (whole row tiles in the kernels' lane order).
                                      * Ignored by every other shape. Only for a saved buffer laid out for exactly the rows of the
                                      * call (csmpn_cemlp_saved_floats(.., rows) floats; not a slice of a larger one): the
                                      * regions are addressed by the call's row count. */

/* One CEMLP block = Sequential(MVLinear, MVSiLU, SteerableGeometricProductLayer,
 * MVLayerNorm) (cegnn_utils.py:177-207). Pointers in reference layouts.
 * Limits of every CEMLP / EGCL entry point: 1..CSMPN_MAX_BLOCKS blocks, out_features 1..256 (65..256: the wide
 * row-tile kernel), in_features unbounded; out_features > 256 returns CSMPN_ERR_UNSUPPORTED. */
typedef struct csmpn_block_params {
    int32_t in_features;
    int32_t out_features;
    int32_t lin_subspaces;   /* 1: lin_w is [O,I,G]; 0: [O,I] (MVLinear subspaces=False) */
    int32_t reserved;
    const float* lin_w;      /* layers.k.0.weight */
    const float* lin_b;      /* layers.k.0.bias [1,O,1] or NULL */
    const float* silu_a;     /* layers.k.1.a [1,O,G] */
    const float* silu_b;     /* layers.k.1.b [1,O,G] */
    const float* gp_w;       /* layers.k.2.weight [O,P] */
    const float* norm_a;     /* layers.k.2.normalization.a [O,G] */
    const float* right_w;    /* layers.k.2.linear_right.weight [O,O,G] */
    const float* left_w;     /* layers.k.2.linear_left.weight [O,O,G] */
    const float* left_b;     /* layers.k.2.linear_left.bias [1,O,1] */
    const float* ln_a;       /* layers.k.3.a [1,O] */
} csmpn_block_params;

/* Gradient accumulators, same shapes as csmpn_block_params' tensors. */
typedef struct csmpn_block_grads {
    float* lin_w;
    float* lin_b;            /* NULL iff lin_b is NULL */
    float* silu_a;
    float* silu_b;
    float* gp_w;
    float* norm_a;
    float* right_w;
    float* left_w;
    float* left_b;
    float* ln_a;
} csmpn_block_grads;

/* Algebra: metric is a HOST array of n floats, every entry +1 or -1,
 * 2 <= n <= 5 for the device entry points (csmpn_metric_supported). */
int csmpn_metric_supported(const float* metric_host, int n);

/* Host-side table construction (any diagonal metric, n <= 8). All outputs are
 * HOST arrays: cayley [D*D*D] (left,out,right), index_to_bitmap [D],
 * bitmap_to_index [D], grades [D] (int64), subspaces [n+1] (int64),
 * paths [(n+1)^3] (uint8, (grade_left, grade_out, grade_right)). Any output
 * pointer may be NULL. */
int csmpn_algebra_tables(const float* metric_host, int n, float* cayley, int64_t* index_to_bitmap,
                         int64_t* bitmap_to_index, int64_t* grades, int64_t* subspaces, uint8_t* paths);

/* out[r, :] = a[r, :] * b[r, :] (geometric product), rows x D. Backward:
 * ga += d/da, gb += d/db given gout. */
int csmpn_geometric_product_forward(const float* metric_host, int n, const float* a, const float* b,
                                    float* out, int64_t rows, void* stream);
int csmpn_geometric_product_backward(const float* metric_host, int n, const float* a, const float* b,
                                     const float* gout, float* ga, float* gb, int64_t rows, void* stream);

/* Workspace (bytes) for a CEMLP of these blocks; covers packed weights and
 * per-launch scratch for any entry point below that takes this CEMLP (65..256 output channels: the wide kernel's
 * global row-tile scratch with its parking region and, for n <= 3, the deterministic gradient copies). */
size_t csmpn_cemlp_workspace_bytes(int n, const csmpn_block_params* blocks, int n_blocks);

/* Saved block inputs (optional, every forward/backward pair below): the forward writes the
 * inputs of blocks 1..n_blocks-1 ([rows, O_{k-1}, D] each, back to back; rows = rows / n_edges /
 * n_nodes of the call, in the kernel's own row order) into save_inputs when it is non-NULL, and
 * the backward reads them from saved_inputs instead of recomputing the earlier blocks (one
 * block forward less per row, and a smaller LDS footprint). NULL on either side = recompute.
 * Floats per row: csmpn_cemlp_saved_floats_per_row(); for two-block Cl(5,0) CEMLPs of 9 .. 32 channels, for the
 * two-block 8-channel Cl(3,0) EGCL shapes (edge model 14 -> 8 -> 8, node model 19 -> 8 -> 8) and for multi-block CEMLPs of
 * the small algebras (n <= 3) outside the lane-kernel shapes this includes a second region of the same size behind the
 * saved inputs that the backward uses as scratch (a block's phase / launch hands d/d(its input) to the previous block's
 * there): the buffer is written by the backward although the pointer is const. */
size_t csmpn_cemlp_saved_floats_per_row(int n, const csmpn_block_params* blocks, int n_blocks);
/* Floats of the saved buffer of ONE launch over `rows` rows (round 4): rows * csmpn_cemlp_saved_floats_per_row() minus the
 * regions a launch of that size never touches - the general kernels' hand-over region exists only for launches that can
 * take the block-by-block backward (rows >= its threshold, default 4096; CSMPN_PHASED_MIN_ROWS): a 940-row node stage of a
 * multi-block CEMLP of the small algebras pays half. A buffer of this size is valid for forward and backward of that
 * launch. flags (ABI version 2): with CSMPN_FLAG_SAVE_STATE the state regions of that flag are included - pass the flag
 * here iff the forward / backward pair will be called with it (they are 3-4x the block inputs on the D = 32 and 32-channel
 * shapes: H28 248 instead of 56 channels x 32 floats per edge); without it the buffer holds block inputs + hand-over only.
 * The regions are counted with the rows rounded up to a multiple of 16 (whole row tiles): for those shapes the result may
 * exceed rows * per-row figure by up to 15 rows of state. */
size_t csmpn_cemlp_saved_floats(int n, const csmpn_block_params* blocks, int n_blocks, int64_t rows, uint32_t flags);

/* y[rows, O_last, D] = CEMLP(x[rows, I_0, D]). */
int csmpn_cemlp_forward(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks,
                        const float* x, int64_t rows, float* y, float* save_inputs, void* workspace, size_t workspace_bytes,
                        uint32_t flags, void* stream);

/* gx[rows, I_0, D] = d<gy,y>/dx (overwritten; may be NULL), grads += d/dparams.
 * Recomputes the forward in-kernel from x. */
int csmpn_cemlp_backward(const float* metric_host, int n, const csmpn_block_params* blocks,
                         const csmpn_block_grads* grads, int n_blocks, const float* x, const float* gy,
                         int64_t rows, float* gx, const float* saved_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* Standalone MVLinear (csmpn/models/cegnn_utils.py:287-338; the callers outside a CEMLP: the
 * projection heads hulls_cssmpnn.py:71-73 and the first stage of the simplex feature embeddings):
 *   y[b,o,d] = sum_i W[o,i,grade(d)] x[b,i,d] (+ bias[o] on blade 0)
 * weight is [O,I,G] (subspaces != 0) or [O,I]; bias [O] or NULL. The grade table depends on n only
 * (blade order metric.py:18-29), so every metric with n <= 5 generators is served. Backward: gx
 * [rows,I,D] overwritten (may be NULL), g_weight += d/dW (may be NULL), g_bias += d/dbias (may be NULL). */
int csmpn_mvlinear_forward(int n, const float* x, const float* weight, const float* bias, int64_t rows,
                           int32_t in_features, int32_t out_features, int32_t subspaces, float* y, void* stream);
int csmpn_mvlinear_backward(int n, const float* x, const float* weight, const float* gy, int64_t rows,
                            int32_t in_features, int32_t out_features, int32_t subspaces, float* gx, float* g_weight,
                            float* g_bias, void* stream);
/* csmpn_mvlinear_backward without float atomics: the (element, row slab) launch stores its partial sums to
 * workspace[slab][element] and a second launch adds the slabs in ascending order INTO g_weight / g_bias (+=, as above); gx as
 * above. Slab size and count depend on (rows, in_features, out_features, subspaces) only, so the result is the same bits
 * in every run and every process. At most 512 slabs: csmpn_mvlinear_backward_det_bytes() =
 * min(ceil(rows / 8), 512) * (weight elements + out_features) * 4 bytes - non-decreasing in rows, constant from 4089 rows
 * on (2.4 MB for a 35 -> 32 layer without subspaces, whatever the row count); host-only, 0 for sizes the entry point rejects
 * and for rows <= 0. The workspace needs no initialisation (every word read was written by the call); NULL or too small:
 * CSMPN_ERR_INVALID (not needed when g_weight and g_bias are both NULL). rows == 0: CSMPN_OK, nothing touched. Nothing is
 * allocated. */
size_t csmpn_mvlinear_backward_det_bytes(int n, int64_t rows, int32_t in_features, int32_t out_features, int32_t subspaces);
int csmpn_mvlinear_backward_det(int n, const float* x, const float* weight, const float* gy, int64_t rows,
                                int32_t in_features, int32_t out_features, int32_t subspaces, float* gx, float* g_weight,
                                float* g_bias, void* workspace, size_t workspace_bytes, void* stream);

/* The four small layers on their own (inside a CEMLP they are fused into the row programs; no
 * reference model calls them alone - these entry points give the nn.Modules a device forward /
 * backward). Rows are [rows, channels, D] float32, D = 2^n; metric entries +-1, n = 2..5 (the
 * signatures csmpn_metric_supported accepts); channels <= 256. Backward: gx overwritten, parameter
 * gradients ACCUMULATED (+=, float atomics: one per parameter and workgroup).
 *   MVSiLU, invariant "mag2" (cegnn_utils.py:53-83): a, b [channels, n+1]
 *     y_d = sigmoid(a[c,g] u_g + b[c,g]) x_d,  g = grade(d), u_0 = x_0, u_g = q_g(x) for g > 0
 *   NormalizationLayer (cegnn_utils.py:34-51): a [channels, n+1]
 *     y_d = x_d / (sigmoid(a[c,g]) (|x|_g - 1) + 1 + 1e-6),  |x|_g = (q_g(x)^2 + 1e-16)^(1/4)
 *   MVLayerNorm (cegnn_utils.py:86-96): a [channels]
 *     y[c] = a[c] x[c] / (mean_c |x[c]| + 1e-6),  |x| over all blades
 *   weighted geometric product of SteerableGeometricProductLayer (cegnn_utils.py:126-152):
 *     weight [channels, P] (P = number of grade paths, cliffordalgebra.py:238-252)
 *     y_j = sum_{(i,k)->j} sign(i,k) weight[c, path(grade i, grade j, grade k)] z_i r_k */
int csmpn_mvsilu_forward(const float* metric_host, int n, const float* x, const float* a, const float* b, int64_t rows,
                         int32_t channels, float* y, void* stream);
int csmpn_mvsilu_backward(const float* metric_host, int n, const float* x, const float* a, const float* b, const float* gy,
                          int64_t rows, int32_t channels, float* gx, float* g_a, float* g_b, void* stream);
int csmpn_mvnorm_forward(const float* metric_host, int n, const float* x, const float* a, int64_t rows, int32_t channels,
                         float* y, void* stream);
int csmpn_mvnorm_backward(const float* metric_host, int n, const float* x, const float* a, const float* gy, int64_t rows,
                          int32_t channels, float* gx, float* g_a, void* stream);
int csmpn_mvlayernorm_forward(const float* metric_host, int n, const float* x, const float* a, int64_t rows,
                              int32_t channels, float* y, void* stream);
int csmpn_mvlayernorm_backward(const float* metric_host, int n, const float* x, const float* a, const float* gy,
                               int64_t rows, int32_t channels, float* gx, float* g_a, void* stream);
int csmpn_wgp_forward(const float* metric_host, int n, const float* z, const float* r, const float* weight, int64_t rows,
                      int32_t channels, float* y, void* stream);
int csmpn_wgp_backward(const float* metric_host, int n, const float* z, const float* r, const float* weight,
                       const float* gy, int64_t rows, int32_t channels, float* gz, float* gr, float* g_weight, void* stream);

/* The same four layers without float atomics, neither in LDS nor in memory (entry points of their own: the backward
 * forms need scratch the plain forms do not take). Arguments, results and limits as the plain forms; the forwards of
 * MVSiLU, NormalizationLayer and the weighted product have no sum across lanes and no _det twin.
 *   Within a workgroup: every lane parks its contributions to the parameter gradients in LDS slots of its own, and one
 *     lane per parameter entry adds the slots of its channel's lanes in ascending lane order - an order fixed by (rows,
 *     channels) alone. MVLayerNorm's sum of a row's channel norms (forward and backward) and of a_c <gy_c, x_c>
 *     (backward) is taken the same way: parked, then added by the row's first lane in ascending channel order.
 *   Across workgroups: every workgroup stores one partial row to workspace[workgroup][entry]; a second launch adds the
 *     partial rows in ascending workgroup order INTO g_* (+=, as the plain forms). Entries per row: MVSiLU 2 (n+1) C,
 *     NormalizationLayer (n+1) C, MVLayerNorm C, weighted product P C.
 *   At most 512 partial rows. A tile is what one workgroup of the plain form covers: 256 consecutive (row, channel)
 *     elements, for MVLayerNorm floor(256 / C) whole rows; tiles = ceil(rows * C / 256), for MVLayerNorm
 *     ceil(rows / floor(256 / C)). Up to 512 tiles every workgroup takes one; beyond, a workgroup walks a contiguous
 *     range of ceil(tiles / 512) tiles and accumulates in tile order, so the scratch stops growing with the rows:
 *     csmpn_small_layer_det_bytes() = min(tiles, 512) * entries * 4 bytes - non-decreasing in rows, constant from the
 *     first row count with 512 tiles on (29.4 MB at most: the weighted product on n = 5, 256 channels; 1.3 MB for it on
 *     Cl(3,0) with 32 channels).
 *   Launch shape, tile ranges and the cap depend on (op, n, rows, channels) only: the same bits in every run and process.
 *   Every shape the plain forms serve is served (the six compiled signatures, 1..256 channels; rows up to 2^40): there
 *     is no fallback. 257 channels: CSMPN_ERR_INVALID, as the plain forms. rows == 0: CSMPN_OK, nothing touched.
 *   The workspace needs no initialisation (every word read was written by the same call); NULL or smaller than
 *     csmpn_small_layer_det_bytes(): CSMPN_ERR_INVALID before anything is launched. Nothing is allocated.
 *     csmpn_small_layer_det_bytes is host-only; 0 for sizes the entry points reject, an unknown op and rows <= 0.
 *   LDS: static, at most 56 * 257 * 4 = 57 568 bytes per workgroup (the weighted product on n = 5: P = 56 path weights
 *     per lane, 256 lanes) - below the 64 KB a launch gets without further ado.
 *   Lanes past rows * channels of a ragged tile park nothing, and their slots are not among those added. */
#define CSMPN_LAYER_MVSILU 0
#define CSMPN_LAYER_MVNORM 1
#define CSMPN_LAYER_MVLAYERNORM 2
#define CSMPN_LAYER_WGP 3
size_t csmpn_small_layer_det_bytes(int op, int n, int64_t rows, int32_t channels);
int csmpn_mvsilu_backward_det(const float* metric_host, int n, const float* x, const float* a, const float* b, const float* gy,
                              int64_t rows, int32_t channels, float* gx, float* g_a, float* g_b, void* workspace,
                              size_t workspace_bytes, void* stream);
int csmpn_mvnorm_backward_det(const float* metric_host, int n, const float* x, const float* a, const float* gy, int64_t rows,
                              int32_t channels, float* gx, float* g_a, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_mvlayernorm_forward_det(const float* metric_host, int n, const float* x, const float* a, int64_t rows,
                                  int32_t channels, float* y, void* stream);
int csmpn_mvlayernorm_backward_det(const float* metric_host, int n, const float* x, const float* a, const float* gy,
                                   int64_t rows, int32_t channels, float* gx, float* g_a, void* workspace, size_t workspace_bytes,
                                   void* stream);
int csmpn_wgp_backward_det(const float* metric_host, int n, const float* z, const float* r, const float* weight, const float* gy,
                           int64_t rows, int32_t channels, float* gz, float* gr, float* g_weight, void* workspace,
                           size_t workspace_bytes, void* stream);

/* One-time per complex: sort the E directed adjacencies by target (stable radix sort).
 * edge_index is the reference's [2,E] int64 (row 0 = source j, row 1 = target i).
 * Outputs (device): perm[E] (sorted position -> original edge id), src_sorted[E],
 * dst_sorted[E] (int32), in_degree[N] (int32), row_ptr[N+1] (int32).
 * workspace: csmpn_csr_workspace_bytes(E, N) bytes of device memory. Inside one target's
 * segment the edges keep ascending original id, so the result (and the summation order
 * downstream) is deterministic. Every index is range-checked against [0, N): an entry outside
 * returns CSMPN_ERR_INVALID (PyG's scatter asserts in that case); the check costs one host
 * synchronisation per call - complexes are static and the result is cached by the caller -
 * and is skipped with CSMPN_FLAG_NO_VALIDATE (out-of-range entries are then mapped to node 0). */
size_t csmpn_csr_workspace_bytes(int64_t n_edges, int64_t n_nodes);
int csmpn_csr_build(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, int32_t* perm,
                    int32_t* src_sorted, int32_t* dst_sorted, int32_t* in_degree, int32_t* row_ptr,
                    void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* Deterministic mode, one-time per complex: the sorted edge positions ordered by SOURCE (stable, so
 * ascending sorted position inside one source's segment). order[E], row_ptr_src[N+1] (device, int32);
 * workspace as for csmpn_csr_build. */
int csmpn_csr_source_order(const int32_t* src_sorted, int64_t n_edges, int64_t n_nodes, int32_t* order,
                           int32_t* row_ptr_src, void* workspace, size_t workspace_bytes, void* stream);

/* Fixed-order segmented sum of a row table (the replacement of PyG's scatter under
 * deterministic algorithms):
 *   out[v] (+)= sum_{k in [add_ptr[v], add_ptr[v+1])} rows[add_order ? add_order[k] : k]
 *             - sum_{k in [sub_ptr[v], sub_ptr[v+1])} rows[sub_order ? sub_order[k] : k]
 * rows [*, row_floats], out [N, row_floats] (16-byte aligned, row_floats % 4 == 0); either
 * (ptr, order) pair may be NULL; accumulate != 0 adds to out instead of overwriting it. */
int csmpn_segment_reduce(const float* rows, int64_t row_floats, int64_t n_nodes, const int32_t* add_ptr,
                         const int32_t* add_order, const int32_t* sub_ptr, const int32_t* sub_order, float* out,
                         int32_t accumulate, void* stream);

/* EGCL message + aggregate (cegnn_utils.py:254-262 + PyG scatter):
 *   agg[v] += sum_{e: dst_e = v} EdgeCEMLP(cat_c[h[dst_e] - h[src_e], edge_attr[perm_e]])
 * agg [N, O, D] must be zeroed by the caller. edge_attr [E, A, D] in ORIGINAL edge
 * order (or NULL when A = 0). The mean's 1/max(deg,1) is applied by the node
 * entry points. */
int csmpn_egcl_edge_forward(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks,
                            const float* h, int32_t channels, const float* edge_attr, int32_t attr_channels,
                            const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted,
                            int64_t n_edges, int64_t n_nodes, float* agg, float* save_inputs, void* workspace,
                            size_t workspace_bytes, uint32_t flags, void* stream);

/* Backward of the above. g_agg [N,O,D] is d/d(agg) (already divided by the degree
 * for aggr=mean). gh [N,C,D] += (scatter of +g to dst, -g to src);
 * g_edge_attr [E,A,D] (original order, overwritten) may be NULL. */
int csmpn_egcl_edge_backward(const float* metric_host, int n, const csmpn_block_params* blocks,
                             const csmpn_block_grads* grads, int n_blocks, const float* h, int32_t channels,
                             const float* edge_attr, int32_t attr_channels, const int32_t* perm,
                             const int32_t* src_sorted, const int32_t* dst_sorted, int64_t n_edges,
                             int64_t n_nodes, const float* g_agg, float* gh, float* g_edge_attr,
                             const float* saved_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* EGCL update (cegnn_utils.py:264-275):
 *   out[v] = (residual ? h[v] : 0) + NodeCEMLP(cat_c[h[v], agg[v] * s_v, node_attr[v]])
 * s_v = 1/max(in_degree[v],1) if mean_aggr else 1. node_attr [N,T,D] or NULL. */
int csmpn_egcl_node_forward(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks,
                            const float* h, int32_t channels, const float* agg, int32_t agg_channels,
                            const float* node_attr, int32_t attr_channels, const int32_t* in_degree,
                            int32_t mean_aggr, int32_t residual, int64_t n_nodes, float* out,
                            float* save_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* Backward of the above: gh [N,C,D] (overwritten) = d/dh incl. residual,
 * g_agg [N,O,D] (overwritten) = d/d(agg) incl. the mean scale,
 * g_node_attr [N,T,D] (overwritten) may be NULL. */
int csmpn_egcl_node_backward(const float* metric_host, int n, const csmpn_block_params* blocks,
                             const csmpn_block_grads* grads, int n_blocks, const float* h, int32_t channels,
                             const float* agg, int32_t agg_channels, const float* node_attr,
                             int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr,
                             int32_t residual, int64_t n_nodes, const float* g_out, float* gh, float* g_agg,
                             float* g_node_attr, const float* saved_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* The whole backward of one EGCL layer: csmpn_egcl_node_backward, then csmpn_egcl_edge_backward on the same stream, with
 * the arguments the two take between them (g_agg and gh are the hand-over between the stages: g_agg [N,O,D] is overwritten
 * by the node stage and read by the edge stage, gh [N,C,D] is overwritten by the node stage and accumulated into by the edge
 * stage). Results are bit-identical to the two separate calls. Each stage has its own saved buffer, workspace and flags
 * (CSMPN_FLAG_WEIGHTS_PACKED, CSMPN_FLAG_SAVE_STATE as on the separate entry points).
 * Where both stages end with a sum over per-workgroup gradient slices (the Cl(3,0) 8-channel kernels), the node stage's sum
 * is not launched in front of the edge stage: one launch behind it sums both stages' slices, every element in the order
 * the separate calls use. For that the two workspaces must not overlap (the node slices wait in the node workspace; with
 * overlapping workspaces the stages run as the separate calls do), and nothing else may write the node workspace on
 * another stream during the call. Every other shape, and CSMPN_FLAG_DETERMINISTIC on either stage: the two stages as
 * the separate entry points run them; with the flag on the edge stage, g_edge_rows is that stage's [E,C,D] per-edge table
 * (csmpn_egcl_edge_backward's gh in that mode), else it is unused and may be NULL. */
int csmpn_egcl_backward(const float* metric_host, int n, const csmpn_block_params* edge_blocks,
                        const csmpn_block_grads* edge_grads, int n_edge_blocks, const csmpn_block_params* node_blocks,
                        const csmpn_block_grads* node_grads, int n_node_blocks, const float* h, int32_t channels,
                        const float* agg, int32_t agg_channels, const float* edge_attr, int32_t edge_attr_channels,
                        const float* node_attr, int32_t node_attr_channels, const int32_t* perm, const int32_t* src_sorted,
                        const int32_t* dst_sorted, const int32_t* in_degree, int32_t mean_aggr, int32_t residual,
                        int64_t n_edges, int64_t n_nodes, const float* g_out, float* gh, float* g_agg, float* g_edge_attr,
                        float* g_node_attr, float* g_edge_rows, const float* edge_saved_inputs, void* edge_workspace,
                        size_t edge_workspace_bytes, uint32_t edge_flags, const float* node_saved_inputs, void* node_workspace,
                        size_t node_workspace_bytes, uint32_t node_flags, void* stream);

/* Input rows of the simplex feature embedding (hulls_cssmpnn.py:96-125, md17_cssmpnn.py:85-120):
 * row r lists verts_per_row vertices (rows of the per-simplex feature tensors) in ONE vertex order;
 * block b contributes verts_per_row * channels_b channels (vertex by vertex), embedded at its grade:
 *   out[r][off_b + v * K_b + k][gstart(grade_b) + t] = blocks[b].data[verts[r][v]][k][t],  0 elsewhere.
 * out [n_rows, sum_b verts_per_row * K_b, 2^n]; blocks[b].data [n_feature_rows, K_b, C(n, grade_b)]. */
typedef struct csmpn_vertex_block {
    const float* data;
    int32_t channels;
    int32_t grade;
} csmpn_vertex_block;
int csmpn_simplex_rows(int n, const csmpn_vertex_block* blocks, int n_blocks, const int64_t* verts, int64_t n_rows,
                       int32_t verts_per_row, int64_t n_feature_rows, float* out, void* stream);

/* Index tables of the embedding stage, rebuilt on the device for a batch of new topology and unchanged row counts (what
 * SimplicialBatch.plan() builds on the host with nonzero / indexing / bincount), so that a captured training step can be
 * replayed on it: no allocation, no host round trip, every launch on `stream`.
 *   inputs (device, int64): x_ind [n_rows, x_ind_cols] (vertex ids local to the row's graph; x_ind_cols > max_dim),
 *     node_types [n_rows], x_ind_batch [n_rows] (graph of every row), x_ind_ptr [n_graphs + 1] (first row of every graph);
 *   n_expected (HOST, int64 [max_dim + 1]): the row count n_d of every dimension = the lengths of the output buffers;
 *   rows / verts / verts_i32 (HOST arrays of max_dim + 1 DEVICE pointers; verts_i32 or single entries of it may be NULL,
 *     rows[d] / verts[d] may be NULL where n_d = 0):
 *     rows[d]  int64 [n_d]: the rows of type d, ascending (a stable compaction by type, implemented as a scan);
 *     verts[d] int64 [n_d * (d+1)!, d+1]: for every such row r in that order and every vertex order pi in lexicographic
 *              order (itertools.permutations(range(d+1))), x_ind[r, pi[j]] + x_ind_ptr[x_ind_batch[r]]; verts_i32[d]: the
 *              same values as int32;
 *   graph_of_vertex int64 [n_0] = x_ind_batch[rows[0]]; vertices_per_graph int64 [n_graphs] = its histogram;
 *   types_i32 int32 [n_rows] (may be NULL) = node_types.
 * Safety: vertex rows are clamped to [0, n_rows) and graph ids to [0, n_graphs); a row whose rank among the rows of its
 * type is not below n_d writes nothing, so a wrong n_expected never writes outside a buffer. Such findings are OR-ed into
 * *status (device, may be NULL; never read by the call, never cleared by it): bit d (d = 0..3) = the batch holds another
 * number of rows of type d than n_expected[d] (fewer: the tail of the tables keeps its old contents), bit 4 = a type
 * outside [0, max_dim] (the row is in no table), bit 5 = a vertex row or graph id was clamped.
 * max_dim <= 3 (24 vertex orders); larger: CSMPN_ERR_UNSUPPORTED. n_rows, n_graphs in [1, 2^31).
 * workspace: csmpn_simplex_tables_workspace_bytes(n_rows, max_dim) bytes of device memory (host-only query; 0 for sizes
 * the entry point rejects); needs no initialisation. */
size_t csmpn_simplex_tables_workspace_bytes(int64_t n_rows, int32_t max_dim);
int csmpn_simplex_tables(const int64_t* x_ind, int32_t x_ind_cols, const int64_t* node_types, const int64_t* x_ind_batch,
                         const int64_t* x_ind_ptr, int64_t n_rows, int64_t n_graphs, int32_t max_dim,
                         const int64_t* n_expected, int64_t* const* rows, int64_t* const* verts, int32_t* const* verts_i32,
                         int64_t* graph_of_vertex, int64_t* vertices_per_graph, int32_t* types_i32, uint32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Vietoris-Rips lift of a batch on the device at a fixed capacity: the structure tensors of exactly the batch that
 *   pad_batch(collate([rips_complex(points_g, dis, max_dim) for g]), BatchCapacity(capacity_rows, capacity_edges))
 * builds on the host (csmpn/data/complexes.py; the filler simplices and filler self-loop adjacencies behind the real part
 * included), written into buffers of the capacity's shapes: no allocation, no host round trip, every launch on `stream`, no
 * atomics on the outputs - every position is computed from popcounts of 64-bit neighbour masks and scans.
 *   points (device, float [n_graphs * verts_per_graph, point_dim], the vertices of graph g contiguous); vertices a and b are
 *     close iff sum_k ((double)p_a[k] - (double)p_b[k])^2 <= dis^2, summed in double over k ascending (a NaN is close to
 *     nothing); dis >= 0;
 *   capacity_rows (HOST, int64 [max_dim + 1]): rows per dimension; capacity_rows[0] == n_graphs * verts_per_graph;
 *   outputs (device, int64): x_ind [rows, x_ind_cols] (x_ind_cols > max_dim; the columns behind a simplex's vertices are 0),
 *     node_types / batch / x_ind_batch [rows] with rows = sum of capacity_rows, ptr / x_ind_ptr [n_graphs + 1],
 *     edge_index [2, capacity_edges], edge_types [capacity_edges, 2] (may be NULL),
 *     counts [max_dim + 2] (may be NULL): the real rows of every dimension, then the real adjacencies.
 * A graph's real rows: its vertices, the close pairs (a < b) and, for max_dim = 2, the triples (a < b < c) with all pairs
 * close, both in lexicographic order; its adjacencies in the order of lift() + to_complex().
 * A batch that does not fit leaves EVERY output as it was and ORs into *status (device, may be NULL; never read, never
 * cleared by the call): bit d (d = 1, 2) = more d-simplices than capacity_rows[d], bit 3 = more adjacencies than
 * capacity_edges, bit 4 = filler adjacencies are needed but the batch leaves no filler row to carry them.
 * Limits: max_dim in {1, 2} and verts_per_graph <= 64, else CSMPN_ERR_UNSUPPORTED; verts_per_graph > max_dim,
 * n_graphs * verts_per_graph, the sum of capacity_rows and capacity_edges in [1, 2^31) ([0, 2^31) for the last), else
 * CSMPN_ERR_INVALID. Arguments are checked before the first HIP call.
 * workspace: csmpn_rips_lift_workspace_bytes(...) bytes of device memory (host-only query; 0 for sizes the entry point
 * rejects); needs no initialisation. */
size_t csmpn_rips_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim);
int csmpn_rips_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, double dis, int32_t max_dim,
                    const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                    int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                    int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The same lift of the clique complex of the k-nearest-neighbour graph: the structure tensors of exactly the batch that
 *   pad_batch(collate([knn_clique_complex(points_g, k, max_dim) for g]), BatchCapacity(capacity_rows, capacity_edges))
 * builds on the host. Every argument but `k`, every contract (three launches on `stream`, no allocation, no host round trip,
 * no atomic on an output), the status bits 1..4 of a batch that does not fit (every output is left as it was), the limits
 * and the workspace are those of csmpn_rips_lift; k < 1: CSMPN_ERR_INVALID.
 *   With s(a, b) = sum_j ((double)p_a[j] - (double)p_b[j])^2, summed in double over j ascending (a NaN sum counts as
 *   +infinity), the rank of b for a is the number of vertices c outside {a, b} of the graph with s(a, c) < s(a, b), or
 *   s(a, c) == s(a, b) and c < b: ties - coincident points and NaN vertices among them - go to the smaller index. b is a
 *   neighbour of a iff that rank is below k (k >= verts_per_graph - 1: every other vertex); {a, b} is an edge iff b is a
 *   neighbour of a or a one of b; the 2-simplices (max_dim = 2) are the triples whose three pairs are edges.
 * A graph's adjacencies are those of csmpn_rips_lift in its order WITHOUT the 0_0 block over the non-edges: 6 n1 + 12 n2 for
 * n1 edges and n2 triangles. */
size_t csmpn_knn_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim);
int csmpn_knn_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t k, int32_t max_dim,
                   const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                   int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                   int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The same lift of the convex-hull complex of verts_per_graph points in R^point_dim, and the hull's volume: the structure
 * tensors of exactly the batch that
 *   pad_batch(collate([hull_complex(points_g, max_dim, method="exact") for g]), BatchCapacity(capacity_rows, capacity_edges))
 * builds on the host. Every argument of csmpn_rips_lift but `dis`, every contract (three launches on `stream`, no allocation,
 * no host round trip, no atomic on an output), the status bits 1..4 of a batch that does not fit (every output, `volume`
 * included, is left as it was) and the adjacency order with the 0_0 block over the non-edges are those of csmpn_rips_lift.
 *   With n = point_dim, a candidate is an n-subset F = (f_0 < ... < f_{n-1}) of a graph's vertices. Its rows are
 *   M_i = p_{f_{i+1}} - p_{f_0}, i = 0..n-2; its normal is N_j = (-1)^(n-1+j) det(M without column j), a determinant being
 *   the Laplace expansion along its first row over the columns ascending, ((M[c0] d0 - M[c1] d1) + M[c2] d2) - ...; and
 *   side(F, q) = sum_j N_j (q_j - p_{f_0, j}), j ascending. All of it in double on the float points, every product, sum and
 *   difference rounded once, none contracted. F is a facet iff side(F, q) > 0 for every vertex q of the graph outside F, or
 *   < 0 for every one; a zero or a NaN makes F no facet. Coplanar point sets, coincident points and NaN vertices therefore
 *   give fewer facets, or none: what qhull does with degenerate input (merged or joggled facets) is NOT restated. On points
 *   in general position this is the facet set of the hull. The 1-simplices are the pairs and, for max_dim = 2, the
 *   2-simplices the triples that lie in a facet (a triple whose three pairs are edges need not be one).
 *   volume (device, float [n_graphs], may be NULL): (sum over the facets of |side(F, p_0)|) / n!, summed in double in the
 *   fixed order csmpn.data.complexes.hull_facets states: the same bits in every call.
 * Limits: point_dim in 2..5 and verts_per_graph <= 16, else CSMPN_ERR_UNSUPPORTED; verts_per_graph > point_dim, else
 * CSMPN_ERR_INVALID; otherwise those of csmpn_rips_lift.
 * workspace: csmpn_hull_lift_workspace_bytes(...) bytes (larger than the other two lifts': the facet tables; 0 for sizes the
 * entry point rejects); needs no initialisation. */
size_t csmpn_hull_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim);
int csmpn_hull_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim,
                    const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                    int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                    int64_t* counts, uint32_t* status, float* volume, void* workspace, size_t workspace_bytes, void* stream);

/* The same lift of the thresholded clique complex of ANY graph G on the verts_per_graph points of a graph of the batch: the
 * structure tensors of exactly the batch that
 *   pad_batch(collate([clique_complex(points_g, edges_g, edge_th, tri_th, max_dim) for g]), BatchCapacity(capacity_rows, capacity_edges))
 * builds on the host. Every argument of csmpn_knn_lift, every contract (every launch and memset on `stream`, no allocation, no
 * host round trip, no atomic on an output - capturable in a HIP graph), the status bits 1..4 of a batch that does not fit (every
 * output is left as it was), the limits and the adjacency order without the 0_0 block over the non-edges are those of
 * csmpn_knn_lift.
 *   The graph: exactly one of edge_list != NULL and k >= 1 (both or neither: CSMPN_ERR_INVALID). k >= 1: G is the symmetrised
 *   k-nearest-neighbour graph of csmpn_knn_lift. edge_list (device, int64 [2, n_list], n_list in [0, 2^31)): {a, b} is an
 *   edge of G iff (a, b) or (b, a) is listed, the ends being GLOBAL vertex ids g * verts_per_graph + a; duplicates and both
 *   directions are harmless, a self-loop is ignored, an entry (-1, -1) is padding and is skipped (one buffer serves lists of
 *   changing length). An end outside [0, n_graphs * verts_per_graph) or two ends in different graphs make the batch invalid:
 *   bit 5 of *status alone is ORed in and every output is left as it was.
 *   The rule, all of it in double on the float points, every product, sum and difference rounded once, none contracted,
 *   every sum over j ascending; a NaN s or g counts as +infinity:
 *     E_keep = the edges {a, b} of G with s(a, b) = sum_j (p_a[j] - p_b[j])^2 <= edge_th^2;
 *     T_keep = the triples a < b < c whose three pairs are edges of G (not of E_keep) with g = uu vv - uv uv <= 4 tri_th^2,
 *       u = p_b - p_a, v = p_c - p_a, uu = sum_j u_j^2, vv = sum_j v_j^2, uv = sum_j u_j v_j (g = 4 area^2; any point_dim);
 *     1-simplices = E_keep and the three pairs of every triple of T_keep (a kept triangle brings back an edge that edge_th
 *       removed, for max_dim = 1 too); 2-simplices (max_dim = 2) = T_keep. Three 1-simplices need not bound a 2-simplex: the
 *       triangles and cofaces of an edge come from T_keep.
 *   edge_th and tri_th are >= 0 or +infinity (NaN or negative: CSMPN_ERR_INVALID); with both +infinity every comparison
 *   holds, a NaN included, and the k source gives the very bits of csmpn_knn_lift.
 * workspace: csmpn_clique_lift_workspace_bytes(...) bytes (the largest of the four lifts': a table of verts_per_graph^2 masks
 * per graph and G's masks; 0 for sizes the entry point rejects); needs no initialisation. */
size_t csmpn_clique_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim);
int csmpn_clique_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t k,
                      const int64_t* edge_list, int64_t n_list, double edge_th, double tri_th, int32_t max_dim,
                      const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                      int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                      int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The Rips lift of point clouds of up to 4096 vertices per graph: the structure tensors of exactly the batch that
 *   pad_batch(collate([rips_complex(points_g, dis, max_dim, vertex_block) for g]), BatchCapacity(capacity_rows, capacity_edges))
 * builds on the host, written into buffers of the capacity's shapes: no allocation, no host round trip, every launch on
 * `stream` (five; four for max_dim = 1), no atomic anywhere - every position is computed from popcounts of the neighbour
 * masks (ceil(verts_per_graph / 64) 64-bit words per vertex), a table of per-word ranks and scans, so the outputs hold the
 * same bits in every call. One wave per vertex: a single graph of 4096 vertices fills the device.
 *   points, the rule (vertices a and b are close iff sum_k ((double)p_a[k] - (double)p_b[k])^2 <= dis^2, summed in double over
 *     k ascending, every difference, product and sum rounded once, none contracted; a NaN vertex is close to nothing;
 *     dis >= 0), capacity_rows, the outputs, a graph's real rows and the fillers are those of csmpn_rips_lift;
 *   vertex_block = 1: a graph's adjacencies are those of csmpn_rips_lift, with the V (V - 1) - n1 entries of the 0_0 block
 *     over the non-edges: V (V - 1) + 5 n1 + 12 n2 for n1 edges and n2 triangles; vertex_block = 0: the same order WITHOUT
 *     that block, 6 n1 + 12 n2, the layout of csmpn_knn_lift (lift(..., vertex_block=False)); any other value:
 *     CSMPN_ERR_INVALID. On verts_per_graph <= 64 (accepted too) vertex_block = 1 gives the bits of csmpn_rips_lift.
 * A batch that does not fit leaves EVERY output as it was and ORs the bits 1..4 of csmpn_rips_lift into *status. A graph with
 * more than 2^31 - 1 triangles is counted as one with 2^31 - 1, which no capacity admits (bit 2).
 * Limits: max_dim in {1, 2} and verts_per_graph <= 4096 (kCloudMaxVerts in csrc/lift.hip: the workspace holds
 * verts_per_graph^2 / 8 bytes of masks per graph and the pair test is quadratic; beyond it a cell grid is the tool), else
 * CSMPN_ERR_UNSUPPORTED; every other check, its code and its place are those of csmpn_rips_lift, vertex_block being checked
 * behind dis. Arguments are checked before the first HIP call.
 * workspace: csmpn_cloud_lift_workspace_bytes(...) bytes of device memory (host-only query; 0 for sizes the entry point
 * rejects): with B = n_graphs, V = verts_per_graph, W = ceil(V / 64): 512 + 8 B V W (masks) + 4 B V W (ranks) + 4 x 4 B V
 * (degrees, upper degrees, triangle and coface counts per vertex, then their prefixes) + 24 B bytes, every part rounded up to
 * 256; needs no initialisation. */
size_t csmpn_cloud_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim);
int csmpn_cloud_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, double dis, int32_t vertex_block,
                     int32_t max_dim, const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols,
                     int64_t* node_types, int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index,
                     int64_t* edge_types, int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The kNN clique lift of point clouds of up to 4096 vertices per graph: the structure tensors of exactly the batch that
 *   pad_batch(collate([knn_clique_complex(points_g, k, max_dim) for g]), BatchCapacity(capacity_rows, capacity_edges))
 * builds on the host, written into buffers of the capacity's shapes. The rule is word for word that of csmpn_knn_lift:
 * s(a, b) summed in double over j ascending, every difference, product and sum rounded once, none contracted, a NaN sum
 * counting as +infinity; rank(a, b) = the number of c outside {a, b} with s(a, c) < s(a, b), or s(a, c) == s(a, b) and c < b; b
 * is a neighbour of a iff rank(a, b) < k (k >= verts_per_graph - 1: every other vertex); {a, b} is an edge iff either names
 * the other; the 2-simplices are the triples whose three pairs are edges; the adjacencies are those of
 * lift(..., vertex_block=False), 6 n1 + 12 n2. On verts_per_graph <= 64 (accepted too) the call writes the very bits of
 * csmpn_knn_lift.
 *   The neighbours are selected, not ranked: a wave per vertex finds the k-th smallest s(a, .) by bisection on its bit
 *   pattern (32 counting passes of two bits each) and takes the ties at that value in ascending index; a second kernel makes
 *   the masks symmetric by reading, for every b, the one word of b's mask that holds bit a. From there on the kernels are those
 *   of csmpn_cloud_lift with vertex_block = 0.
 * Contracts, those of csmpn_cloud_lift: every launch on `stream` (six; five for max_dim = 1), no allocation, no host round
 * trip, no atomic anywhere - the outputs hold the same bits in every call and the call can be captured in a HIP graph. A batch
 * that does not fit leaves EVERY output as it was and ORs the bits 1..4 of csmpn_rips_lift into *status; a graph's triangle
 * count saturates at 2^31 - 1, which no capacity admits (bit 2).
 * Limits: max_dim in {1, 2} and verts_per_graph <= 4096 (kCloudMaxVerts), else CSMPN_ERR_UNSUPPORTED; k < 1:
 * CSMPN_ERR_INVALID, checked where csmpn_knn_lift checks it; every other check, its code and its place are those of
 * csmpn_cloud_lift. Arguments are checked before the first HIP call.
 * workspace: csmpn_cloud_knn_lift_workspace_bytes(...) bytes of device memory (host-only query; 0 for sizes the entry point
 * rejects): that of csmpn_cloud_lift plus 8 B V W bytes, rounded up to 256, for the masks before they are made symmetric;
 * needs no initialisation. */
size_t csmpn_cloud_knn_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim);
int csmpn_cloud_knn_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t k, int32_t max_dim,
                         const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                         int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                         int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Fused simplex feature embedding (round 3; hulls_cssmpnn.py:96-125: vertex features of every d-simplex in all (d+1)!
 * vertex orders -> CEMLP -> sum over the orders), for the two standalone programs the wide parity-lane kernels are
 * instantiated for (Cl(5,0) / Cl(4,1), blocks of 28 output channels; in_features = verts_per_row * channels_per_vertex = 2
 * with one block, or 3 with two blocks: the edge and triangle embeddings of the convex-hulls model);
 * every other shape - 16 / 24 / 32 channels and other input widths included - returns CSMPN_ERR_UNSUPPORTED (the caller
 * composes csmpn_simplex_rows + csmpn_cemlp_* + a sum).
 *   vertex_feat [n_feature_rows, channels_per_vertex, D]  the embedded (full multivector) features of every batch row;
 *   verts [n_rows, verts_per_row] int32: row r = vertex order r % n_orders of simplex r / n_orders (n_rows = n_simplices * n_orders);
 *   out [n_simplices, O, D]: out[s] = sum over its n_orders rows of CEMLP(concat_v vertex_feat[verts[r][v]]).
 * Neither the [n_rows, I, D] input rows nor the [n_rows, O, D] per-order outputs exist in memory; the sum is taken in
 * registers in row order (no atomics). n_orders in {1, 2, 6}. save_inputs / saved_inputs as for csmpn_cemlp_* (rows = n_rows).
 * n_vertex_rows = n_feature_rows (ABI version 2). Every entry of verts must lie in [0, n_vertex_rows): both entry points
 * range-check the table (one synchronous host round trip on `stream`, as csmpn_csr_build) and return CSMPN_ERR_INVALID
 * otherwise; a caller that has validated its table once per batch passes CSMPN_FLAG_NO_VALIDATE (required inside a stream
 * capture). The kernels clamp the ids into [0, n_vertex_rows) in any case: a bad id reads a wrong row, never out of bounds.
 * backward: d/d(parameters) only (the features are data); g_out [n_simplices, O, D]. */
int csmpn_embed_cemlp_forward(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks,
                              const float* vertex_feat, int64_t n_vertex_rows, int32_t channels_per_vertex, const int32_t* verts,
                              int32_t verts_per_row, int32_t n_orders, int64_t n_rows, float* out, float* save_inputs,
                              void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);
int csmpn_embed_cemlp_backward(const float* metric_host, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                               int n_blocks, const float* vertex_feat, int64_t n_vertex_rows, int32_t channels_per_vertex,
                               const int32_t* verts, int32_t verts_per_row, int32_t n_orders, int64_t n_rows, const float* g_out,
                               const float* saved_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* Vector readout + loss of the trajectory task models (round 5; md17_cssmpnn.py:165-176, motion_cssmpnn.py:150-168,
 * nba_cssmpnn.py:176-191): the final MVLinear of the head restricted to the vector blades, the residual on the positions, the
 * distance to the target and the per-graph losses in one launch (fixed-order sums, no atomics).
 *   x [n_rows, C, D]; vertex_rows [V] int32 = row of x of every vertex (NULL: row v = vertex v, n_rows == V);
 *   weight [O, C, weight_stride] (layers' MVLinear.weight [O, C, G], subspaces = True: the grade-1 entry is used; the bias
 *   sits on blade 0 and does not reach the vector blades); loc [V, O, n] or NULL; target [V_t, O, n]; target_row [V] int32 =
 *   row of target of every vertex, -1 = not scored (NBA: the ball) (NULL: row v); vertex_ptr [B + 1] int32: the vertices of
 *   graph b are vertex_ptr[b] .. vertex_ptr[b + 1] - 1.
 *   pred[v][o][a]   = sum_c weight[o][c][1] x[row(v)][c][1 + a] (+ loc[v][o][a])                       [V, O, n]
 *   d               = pred - target over the cnt_b scored vertices of graph b
 *   per_graph[b]    = ( sum |d|^2 / (cnt_b O),  sum |d| / (cnt_b O),  sum_v |d[v][O - 1]| / cnt_b )     [B, 3]  (MSE, ADE, FDE)
 *   per_vertex[v]   = sum_{o, a} d^2 / (O n)  (0 if not scored)                                         [V]
 * backward: given g_per_graph [B, 3] and / or g_per_vertex [V] (either may be NULL): gx [n_rows, C, D] is WRITTEN (zero
 * outside the vector blades of the vertex rows; vertex_of_row [n_rows] int32 = vertex of a row or -1, NULL with vertex_rows
 * NULL), g_weight [O, C, weight_stride] is ACCUMULATED at the grade-1 entries; gpred_scratch [V, O, n] floats of scratch;
 * graph_of_vertex [V] int32. A zero distance contributes no ADE / FDE gradient (the reference's sqrt backward gives NaN there).
 * Limits: C <= 64, O <= 1024, O * C <= 4096. */
int csmpn_readout_traj_forward(int n, const float* x, int32_t channels, const int32_t* vertex_rows, int64_t n_vertices,
                               const float* weight, int32_t out_channels, int32_t weight_stride, const float* loc, const float* target,
                               const int32_t* target_row, const int32_t* vertex_ptr, int64_t n_graphs, float* pred, float* per_graph,
                               float* per_vertex, void* stream);
int csmpn_readout_traj_backward(int n, const float* x, int32_t channels, int64_t n_rows, const int32_t* vertex_rows,
                                const int32_t* vertex_of_row, int64_t n_vertices, const float* weight, int32_t out_channels,
                                int32_t weight_stride, const float* pred, const float* target, const int32_t* target_row,
                                const int32_t* graph_of_vertex, const int32_t* vertex_ptr, const float* g_per_graph,
                                const float* g_per_vertex, float* gpred_scratch, float* gx, float* g_weight, void* stream);

/* Node / edge attributes of the simplicial task models from per-type features (md17_cssmpnn.py:122-133 embed_simplex_types:
 * sim_type_embedding(node_types) embedded as scalars, edge attribute = (source, target) attributes side by side):
 *   node_attr[s][k][0]     = table[types[s]][k]                 [n_nodes, K, D], the other blades 0
 *   edge_attr[e][k][0]     = table[types[src[e]]][k]            [n_edges, 2 K, D]
 *   edge_attr[e][K + k][0] = table[types[dst[e]]][k]
 * table [n_types, K] (nn.Embedding.weight; n_types * K <= 64), types [n_nodes] in [0, n_types), src / dst = edge_index[0] /
 * edge_index[1] (original edge order), all int32. backward: g_table[t][k] += the blade-0 gradients of every row that read
 * table[t][k] (accumulated: the caller zeroes g_table; either gradient may be NULL; float atomics on n_types * K values). */
int csmpn_type_attr_forward(int n, const float* table, int32_t n_types, int32_t k, const int32_t* types, int64_t n_nodes,
                            const int32_t* src, const int32_t* dst, int64_t n_edges, float* node_attr, float* edge_attr, void* stream);
int csmpn_type_attr_backward(int n, int32_t n_types, int32_t k, const int32_t* types, int64_t n_nodes, const int32_t* src,
                             const int32_t* dst, int64_t n_edges, const float* g_node_attr, const float* g_edge_attr, float* g_table,
                             void* stream);
/* csmpn_type_attr_backward without float atomics (none in LDS either): every workgroup sums the n_types * K bins of a
 * contiguous chunk of the n_nodes + n_edges rows in ascending row order (an edge's source before its target) and stores them
 * as one row of 64 floats in the workspace; a second launch adds the rows in ascending order INTO g_table (+=). Chunk size
 * and workgroup count depend on (K, n_nodes + n_edges) only. csmpn_type_attr_backward_det_bytes() =
 * min(ceil((n_nodes + n_edges) / floor(256 / K)), 256) * 256 bytes (at most 64 KB; non-decreasing in the rows, constant
 * from 256 * floor(256 / K) rows on; host-only; 0 for sizes the entry point rejects and for no rows). Workspace, errors and
 * the empty call as csmpn_mvlinear_backward_det; type ids are clamped as in the plain form. */
size_t csmpn_type_attr_backward_det_bytes(int32_t n_types, int32_t k, int64_t n_nodes, int64_t n_edges);
int csmpn_type_attr_backward_det(int n, int32_t n_types, int32_t k, const int32_t* types, int64_t n_nodes, const int32_t* src,
                                 const int32_t* dst, int64_t n_edges, const float* g_node_attr, const float* g_edge_attr,
                                 float* g_table, void* workspace, size_t workspace_bytes, void* stream);

/* Scalar readout + loss of the convex-hulls model (hulls_cssmpnn.py:93,155-164):
 *   pred_g = mean_{s in graph g} (sum_c weight[c * weight_stride] * x[s][c][0]) + bias,  loss_g = (pred_g - target_g)^2
 * weight points at MVLinear.weight[0] (out_features = 1; weight_stride = n+1 with subspaces, else 1),
 * bias at MVLinear.bias or NULL. The simplices of graph g are rows [graph_ptr[g], graph_ptr[g+1]).
 * channel_sums [n_graphs, channels] receives sum_s x[s][c][0] (the weight gradient is coef^T channel_sums).
 * backward: gx[s][c][d] = (d == 0) ? coef[graph(s)] * weight[c * weight_stride] : 0 (overwritten), with
 * coef_g = dL/dloss_g * 2 (pred_g - target_g) / max(count_g, 1) computed by the caller. Rows at or behind
 * graph_ptr[n_graphs] (n_rows may exceed it: the filler rows of a padded batch) belong to no graph: they are not read by
 * the forward and get gx = 0. */
int csmpn_readout_mse_forward(int n, const float* x, const float* weight, int32_t weight_stride, const float* bias,
                              int64_t n_rows, int32_t channels, const int32_t* graph_ptr, int64_t n_graphs,
                              const float* target, float* pred, float* loss, float* channel_sums, void* stream);
int csmpn_readout_mse_backward(int n, const float* weight, int32_t weight_stride, int64_t n_rows, int32_t channels,
                               const int32_t* graph_ptr, int64_t n_graphs, const float* coef, float* gx, void* stream);

/* ---------------------------------------------------------------------------------------------------------- float64
 * CEMLP and the EGCL stages on contiguous float64 device tensors (parameters, attributes and gradients float64 too; the
 * metric stays a host array of floats, the index tables int32): one kernel family of its own (csrc/cemlp_f64.hpp,
 * "f64" in the CSMPN_DEBUG dispatch log), built for correctness and a fixed summation order. The arithmetic is that of
 * the C++ twin (oracle/cpu_twin/csmpn_cpu.cpp) in double, with the reference's float64 constants 1e-16 and 1e-6.
 * Bit-reproducible: no float atomic on any output or gradient - tiles map to workgroups statically, every workgroup
 * adds its parameter gradients into its own slice of the workspace, a second launch adds the slices in ascending order
 * INTO the gradient tensors (+=), and the edge stage writes row tables in sorted edge order which the fixed-order segment
 * sum below turns into agg / gh (the call sequence of CSMPN_FLAG_DETERMINISTIC). No flags, no saved buffers: the backward
 * recomputes the forward from its inputs.
 * Limits: every signature csmpn_signature_supported accepts ("run-time signature" below says which kernel serves which;
 * else CSMPN_ERR_UNSUPPORTED), 1..CSMPN_MAX_BLOCKS
 * blocks, out_features of every block 1..64 (one row of a block must fit the LDS; above: CSMPN_ERR_UNSUPPORTED),
 * in_features unbounded (input rows are streamed).
 * Workspace: with D = 2^n, G = n + 1, P grade paths, per block s_k = O I (G | 1) + 3 O + 3 O G + O P + 2 O O G doubles of
 * gradient slice, maxO the widest out_features, maxW the widest in_ or out_features, r = 8 (7 maxO D + 5 maxO G + 3 maxO + 2)
 * bytes of LDS per row: tile rows R = min(32, 65536 / r), or 163840 / r where that is 0; tiles = ceil(rows / R);
 * grid = min(tiles, 512), or min(tiles, 256) where R r > 65536;
 *   bytes = 8 grid (sum_k s_k + R D sum_k I_k + 2 R D maxW)
 * (0 for rows = 0 and for arguments the entry points reject). Needs no initialisation.
 * Argument checks (all in front of the first HIP call - a rejected call launches nothing and writes nothing): null
 * pointers, block count, chained widths, a workspace smaller than the query, negative rows / n_edges / n_nodes:
 * CSMPN_ERR_INVALID; n outside 2..5, a metric entry other than +1 / -1, a width above 64: CSMPN_ERR_UNSUPPORTED. Data pointers may be null where
 * the row count is 0. Every entry point is capturable (no allocation, no host synchronisation). */
typedef struct csmpn_block_params_f64 {
    int32_t in_features;
    int32_t out_features;
    int32_t lin_subspaces;
    int32_t reserved;
    const double* lin_w;
    const double* lin_b;     /* or NULL */
    const double* silu_a;
    const double* silu_b;
    const double* gp_w;
    const double* norm_a;
    const double* right_w;
    const double* left_w;
    const double* left_b;
    const double* ln_a;
} csmpn_block_params_f64;

typedef struct csmpn_block_grads_f64 {   /* any pointer may be NULL: that gradient is not wanted */
    double* lin_w;
    double* lin_b;
    double* silu_a;
    double* silu_b;
    double* gp_w;
    double* norm_a;
    double* right_w;
    double* left_w;
    double* left_b;
    double* ln_a;
} csmpn_block_grads_f64;

size_t csmpn_cemlp_f64_workspace_bytes(int n, const csmpn_block_params_f64* blocks, int n_blocks, int64_t rows);

/* y [rows, O, D] = CEMLP of x [rows, I, D]; backward: gx (or NULL) and the parameter gradients (+=) from x and gy. */
int csmpn_cemlp_forward_f64(const float* metric_host, int n, const csmpn_block_params_f64* blocks, int n_blocks, const double* x,
                            int64_t rows, double* y, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_cemlp_backward_f64(const float* metric_host, int n, const csmpn_block_params_f64* blocks,
                             const csmpn_block_grads_f64* grads, int n_blocks, const double* x, const double* gy, int64_t rows,
                             double* gx, void* workspace, size_t workspace_bytes, void* stream);

/* Edge stage, workspace for n_edges rows. Forward: msg_rows [E, O, D], row e = the message of sorted edge e (sum it over
 * row_ptr with the segment sum below to get agg). Backward: g_edge_rows [E, C, D], row e = d/d(h_i - h_j) of sorted edge e
 * (gh += segment sum: + by target over row_ptr, - by source order), g_edge_attr [E, A, D] in ORIGINAL edge order or NULL. */
int csmpn_egcl_edge_forward_f64(const float* metric_host, int n, const csmpn_block_params_f64* blocks, int n_blocks,
                                const double* h, int32_t channels, const double* edge_attr, int32_t attr_channels,
                                const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted, int64_t n_edges,
                                int64_t n_nodes, double* msg_rows, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_egcl_edge_backward_f64(const float* metric_host, int n, const csmpn_block_params_f64* blocks,
                                 const csmpn_block_grads_f64* grads, int n_blocks, const double* h, int32_t channels,
                                 const double* edge_attr, int32_t attr_channels, const int32_t* perm, const int32_t* src_sorted,
                                 const int32_t* dst_sorted, int64_t n_edges, int64_t n_nodes, const double* g_agg,
                                 double* g_edge_rows, double* g_edge_attr, void* workspace, size_t workspace_bytes, void* stream);

/* Node stage, workspace for n_nodes rows; semantics of the float32 stage: input (h, agg / max(in_degree, 1) under
 * mean_aggr, node_attr), out = CEMLP (+ h under residual). Backward: gh = d/dh of the node model (+ g_out under residual),
 * g_agg (mean scale applied), g_node_attr or NULL. */
int csmpn_egcl_node_forward_f64(const float* metric_host, int n, const csmpn_block_params_f64* blocks, int n_blocks,
                                const double* h, int32_t channels, const double* agg, int32_t agg_channels,
                                const double* node_attr, int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr,
                                int32_t residual, int64_t n_nodes, double* out, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_egcl_node_backward_f64(const float* metric_host, int n, const csmpn_block_params_f64* blocks,
                                 const csmpn_block_grads_f64* grads, int n_blocks, const double* h, int32_t channels,
                                 const double* agg, int32_t agg_channels, const double* node_attr, int32_t attr_channels,
                                 const int32_t* in_degree, int32_t mean_aggr, int32_t residual, int64_t n_nodes,
                                 const double* g_out, double* gh, double* g_agg, double* g_node_attr, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* The contract of csmpn_segment_reduce on doubles (no alignment requirement; row_doubles >= 1). */
int csmpn_segment_reduce_f64(const double* rows, int64_t row_doubles, int64_t n_nodes, const int32_t* add_ptr,
                             const int32_t* add_order, const int32_t* sub_ptr, const int32_t* sub_order, double* out,
                             int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------- run-time signature
 * CEMLP and the EGCL stages on EVERY signature Cl(p,q) with p + q = n in 2..5 (60 metrics of +1 / -1 entries, in any
 * order of the generators): one kernel family (csrc/cemlp_sig.hpp, "sig" in the CSMPN_DEBUG dispatch log) that takes the
 * signature as a kernel argument. Design, order of summation, limits, contracts and call sequence are those of the float64
 * family above (no atomics, no flags, no saved buffers, the backward recomputes the forward, parameter gradients +=, row
 * tables summed by the fixed-order segment sum, capturable, bit-reproducible); only the sign of a blade product and of the
 * quadratic form are looked up from a table that each workgroup expands from the signature.
 *   float64: the seven *_f64 entry points above serve every such signature - the six compiled algebras on their own kernel
 *     (on the sig kernel too when the environment has CSMPN_FORCE_SIG=1, read once per process: a test and A/B switch, the
 *     bits are the same), every other signature on the sig kernel. Plan and workspace are the float64 formula, unchanged.
 *   float32: the seven *_sig entry points below, on contiguous float tensors; they accept all 60 signatures, the six
 *     compiled ones included. csmpn_segment_reduce sums their row tables. The float32 entry points further up
 *     (csmpn_cemlp_forward, ...) are unchanged and still reject a signature that is not compiled.
 * csmpn_signature_supported: 1 when n is in 2..5 and every entry of the host array is exactly +1 or -1, else 0 (NULL: 0).
 * csmpn_metric_supported keeps its meaning: the six compiled algebras, which every other entry point needs.
 * Workspace of the float32 family: with D, G, P, s_k, maxO, maxW as in the float64 formula, t = 16 ceil((D D + D) / 16) bytes
 * of sign table, r = 4 (7 maxO D + 5 maxO G + 3 maxO + 2) bytes of LDS per row: tile rows R = min(32, (65536 - t) / r), or
 * (163840 - t) / r where that is 0; tiles = ceil(rows / R); grid = min(tiles, 512), or min(tiles, 256) where R r + t > 65536;
 *   bytes = 4 grid (sum_k s_k + R D sum_k I_k + 2 R D maxW)
 * (0 for rows = 0 and for arguments the entry points reject). Needs no initialisation.
 * Argument checks, codes and their place in front of the first HIP call: those of the float64 family; a metric that
 * csmpn_signature_supported rejects: CSMPN_ERR_UNSUPPORTED. */
int csmpn_signature_supported(const float* metric_host, int n);

size_t csmpn_cemlp_sig_workspace_bytes(int n, const csmpn_block_params* blocks, int n_blocks, int64_t rows);

int csmpn_cemlp_forward_sig(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks, const float* x,
                            int64_t rows, float* y, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_cemlp_backward_sig(const float* metric_host, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                             int n_blocks, const float* x, const float* gy, int64_t rows, float* gx, void* workspace,
                             size_t workspace_bytes, void* stream);
int csmpn_egcl_edge_forward_sig(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks, const float* h,
                                int32_t channels, const float* edge_attr, int32_t attr_channels, const int32_t* perm,
                                const int32_t* src_sorted, const int32_t* dst_sorted, int64_t n_edges, int64_t n_nodes,
                                float* msg_rows, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_egcl_edge_backward_sig(const float* metric_host, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                                 int n_blocks, const float* h, int32_t channels, const float* edge_attr, int32_t attr_channels,
                                 const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted, int64_t n_edges,
                                 int64_t n_nodes, const float* g_agg, float* g_edge_rows, float* g_edge_attr, void* workspace,
                                 size_t workspace_bytes, void* stream);
int csmpn_egcl_node_forward_sig(const float* metric_host, int n, const csmpn_block_params* blocks, int n_blocks, const float* h,
                                int32_t channels, const float* agg, int32_t agg_channels, const float* node_attr,
                                int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr, int32_t residual,
                                int64_t n_nodes, float* out, void* workspace, size_t workspace_bytes, void* stream);
int csmpn_egcl_node_backward_sig(const float* metric_host, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                                 int n_blocks, const float* h, int32_t channels, const float* agg, int32_t agg_channels,
                                 const float* node_attr, int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr,
                                 int32_t residual, int64_t n_nodes, const float* g_out, float* gh, float* g_agg,
                                 float* g_node_attr, void* workspace, size_t workspace_bytes, void* stream);

/* Last error message of the calling thread (never NULL). */
const char* csmpn_last_error(void);

/* Diagnostic: the kernel the calling thread's last CEMLP / EGCL-stage entry point dispatched ("" before the first
 * launch), spelled as rocprofv3 prints it where the family's template arguments are known at the dispatch site, e.g.
 * "csmpn::cemlp_cl_bwd_kernel<csmpn::Alg<3, 0u>, 8, 1, 2, 6>". bench.py reports it as roofline.kernel. */
const char* csmpn_last_kernel(void);

/* Library/ABI version and the gfx target it was built for. */
int csmpn_abi_version(void);
const char* csmpn_build_target(void);

#ifdef __cplusplus
}
#endif
#endif /* CSMPN_HIP_H */
