// C-ABI of the library (declared in include/csmpn_hip.h): the entry points, their argument checks and the per-process
// state (error text, environment switches, last kernel name). Planning: plan.hip; kernel families and buffer layout: dispatch.hip.
#include <mutex>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plan.hpp"

using namespace csmpn;

thread_local char g_csmpn_err[512] = "";

int csmpn_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_csmpn_err, sizeof(g_csmpn_err), fmt, ap);
    va_end(ap);
    return code;
}


namespace csmpn {
thread_local char g_last_kernel[192] = "";
void note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_kernel, sizeof(g_last_kernel), fmt, ap);
    va_end(ap);
}
const Switches& sw() {
    static const Switches s = [] {
        auto flag = [](const char* n) { const char* v = getenv(n); return v && atoi(v) != 0; };
        auto num = [](const char* n, long d) { const char* v = getenv(n); return v ? atol(v) : d; };
        Switches r;
        r.no_cl = flag("CSMPN_NO_CL"); r.no_cm = flag("CSMPN_NO_CM"); r.no_cm_bwd = flag("CSMPN_NO_CM_BWD");
        r.no_pl = flag("CSMPN_NO_PL"); r.no_plw = flag("CSMPN_NO_PLW"); r.plw8 = flag("CSMPN_PLW8");
        r.no_pg = flag("CSMPN_NO_PG"); r.no_pq = flag("CSMPN_NO_PQ");
        r.no_share = flag("CSMPN_NO_SHARE"); r.no_phased = flag("CSMPN_NO_PHASED"); r.no_sliced = flag("CSMPN_NO_SLICED_GRADS");
        r.debug = getenv("CSMPN_DEBUG") != nullptr;
        r.quiet = getenv("CSMPN_QUIET") != nullptr;
        r.force_ps = getenv("CSMPN_FORCE_PS") ? (atoi(getenv("CSMPN_FORCE_PS")) != 0) : -1;
        r.force_h = getenv("CSMPN_FORCE_H") ? (atoi(getenv("CSMPN_FORCE_H")) == 2 ? 2 : 1) : 0;
        r.min_lds_tiles = (int)num("CSMPN_MIN_LDS_TILES", 1);
        r.phased_min_rows = num("CSMPN_PHASED_MIN_ROWS", 16L * 256);
        r.cl_cap_fwd = num("CSMPN_CL_CAP_FWD", 0); r.cl_cap_bwd = num("CSMPN_CL_CAP_BWD", 0);
        return r;
    }();
    return s;
}
unsigned long long* g_stamps = nullptr;
}  // namespace csmpn

// =============================================================================== C-ABI
extern "C" {

const char* csmpn_last_error(void) { return g_csmpn_err; }
const char* csmpn_last_kernel(void) { return g_last_kernel; }

#ifdef CSMPN_STAMPS
/* diagnostic library only (`make stamps`, never shipped): device buffer of 25 uint64 per-phase cycle sums + wave count */
void csmpn_debug_set_stamps(void* device_u64x25) { g_stamps = static_cast<unsigned long long*>(device_u64x25); }
#endif
int csmpn_abi_version(void) { return 2; }   // 2 (round 5): csmpn_embed_cemlp_* take n_vertex_rows, csmpn_cemlp_saved_floats takes flags;
                                            // CSMPN_FLAG_WEIGHTS_PACKED has a meaning on the EGCL / CEMLP backward entry points, CSMPN_FLAG_SAVE_STATE on csmpn_cemlp_*
const char* csmpn_build_target(void) { return "gfx950"; }

int csmpn_metric_supported(const float* metric_host, int n) { return alg_id(metric_host, n) != ALG_NONE ? 1 : 0; }

int csmpn_algebra_tables(const float* metric, int n, float* cayley, int64_t* index_to_bitmap, int64_t* bitmap_to_index,
                         int64_t* grades, int64_t* subspaces, uint8_t* paths) {
    if (!metric || n < 1 || n > 8) return fail(CSMPN_ERR_INVALID, "n=%d not in 1..8", n);
    const int D = 1 << n, G = n + 1;
    std::vector<int> bm(D), idx(D), gr(D);
    int pos = 0;
    for (int g = 0; g <= n; ++g) {
        // combinations of g generators in lexicographic order (metric.py:18-29)
        std::vector<int> comb(g);
        for (int t = 0; t < g; ++t) comb[t] = t;
        while (true) {
            int b = 0;
            for (int t = 0; t < g; ++t) b |= 1 << comb[t];
            bm[pos] = b; gr[pos] = g; idx[b] = pos; ++pos;
            int t = g - 1;
            while (t >= 0 && comb[t] == n - g + t) --t;
            if (t < 0) break;
            ++comb[t];
            for (int u = t + 1; u < g; ++u) comb[u] = comb[u - 1] + 1;
        }
    }
    if (index_to_bitmap) for (int i = 0; i < D; ++i) index_to_bitmap[i] = bm[i];
    if (bitmap_to_index) for (int i = 0; i < D; ++i) bitmap_to_index[i] = idx[i];
    if (grades) for (int i = 0; i < D; ++i) grades[i] = gr[i];
    if (subspaces) {
        for (int g = 0; g < G; ++g) subspaces[g] = 0;
        for (int i = 0; i < D; ++i) subspaces[gr[i]] += 1;
    }
    if (cayley) memset(cayley, 0, sizeof(float) * (size_t)D * D * D);
    if (paths) memset(paths, 0, (size_t)G * G * G);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            const unsigned a = (unsigned)bm[i], b = (unsigned)bm[k];
            // metric.py:50-79: reordering sign times the metric of the shared generators
            int s = 0;
            for (unsigned t = a >> 1; t; t >>= 1) s += popcount_u(t & b);
            float coeff = (s & 1) ? -1.0f : 1.0f;
            for (int bit = 0; bit < n; ++bit)
                if ((a & b) >> bit & 1u) coeff *= metric[bit];
            const int j = idx[a ^ b];
            if (cayley) cayley[((size_t)i * D + j) * D + k] = coeff;
            if (paths && coeff != 0.0f) paths[(gr[i] * G + gr[j]) * G + gr[k]] = 1;
        }
    return CSMPN_OK;
}

int csmpn_geometric_product_forward(const float* metric, int n, const float* a, const float* b, float* out,
                                    int64_t rows, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    HIP_TRY(alg_ops(id).launch_gp(false, a, b, nullptr, out, nullptr, nullptr, rows, (hipStream_t)stream));
    return CSMPN_OK;
}

int csmpn_geometric_product_backward(const float* metric, int n, const float* a, const float* b, const float* gout,
                                     float* ga, float* gb, int64_t rows, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    HIP_TRY(alg_ops(id).launch_gp(true, a, b, gout, nullptr, ga, gb, rows, (hipStream_t)stream));
    return CSMPN_OK;
}

size_t csmpn_cemlp_saved_floats(int n, const csmpn_block_params* blocks, int n_blocks, int64_t rows, uint32_t flags) {
    if (rows <= 0 || !blocks || n_blocks < 1 || n_blocks > CSMPN_MAX_BLOCKS || n < 1 || n > 8) return 0;
    return saved_layout(n, blocks, n_blocks, rows, flags).total;
}

// upper bound per row (the state regions hold up to 15 padding rows more: csmpn_cemlp_saved_floats is exact)
size_t csmpn_cemlp_saved_floats_per_row(int n, const csmpn_block_params* blocks, int n_blocks) {
    if (!blocks || n_blocks < 1 || n_blocks > CSMPN_MAX_BLOCKS || n < 1 || n > 8) return 0;
    return saved_layout(n, blocks, n_blocks, -1, CSMPN_FLAG_SAVE_STATE).total;
}

size_t csmpn_cemlp_workspace_bytes(int n, const csmpn_block_params* blocks, int n_blocks) {
    if (!blocks || n_blocks < 1 || n_blocks > CSMPN_MAX_BLOCKS || n < 1 || n > 8) return 0;
    // behind the general / wide kernels' front part: a lane family's region or the deterministic copies (never together: the
    // larger one; widths above 64 channels have no lane family)
    const size_t tail = family_tail_bytes(n, blocks, n_blocks), det = det_slice_bytes(n, blocks, n_blocks);
    return plan_front_bytes(n, blocks, n_blocks) + (tail > det ? tail : det) + kTailSlack;
}

int csmpn_cemlp_forward(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* x,
                        int64_t rows, float* y, float* save_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    Plan plan;
    int rc = make_plan(id, blocks, nullptr, n_blocks, workspace, workspace_bytes, false, 0, false, rows, plan,
                       (flags & CSMPN_FLAG_DETERMINISTIC) != 0);
    if (rc) return rc;
    const bool need_pack = !(flags & CSMPN_FLAG_WEIGHTS_PACKED);   // packed fragments are a matter of the general kernels: run_rows
    RowIO io;
    memset(&io, 0, sizeof(io));
    io.rows = rows; io.nseg = 1;
    io.seg[0].a = x; io.seg[0].ch = blocks[0].in_features; io.seg[0].off = 0;
    io.y = y; io.save = save_inputs;
    // CSMPN_FLAG_SAVE_STATE: honoured for the shapes whose saved buffer has state regions (pq_plain_shape), ignored otherwise
    io.save_state = ((flags & CSMPN_FLAG_SAVE_STATE) && pq_plain_shape(n, blocks, n_blocks)) ? 1 : 0;
    return run_rows(plan, MODE_PLAIN, false, io, (hipStream_t)stream, need_pack);
}

int csmpn_cemlp_backward(const float* metric, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                         int n_blocks, const float* x, const float* gy, int64_t rows, float* gx, const float* saved_inputs, void* workspace,
                         size_t workspace_bytes, uint32_t flags, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    Plan plan;
    int rc = make_plan(id, blocks, grads, n_blocks, workspace, workspace_bytes, true, 0, saved_inputs != nullptr, rows, plan,
                       (flags & CSMPN_FLAG_DETERMINISTIC) != 0);
    if (rc) return rc;
    // fragments packed by the forward are only valid for the forward's own layout choice (a forward
    // with LDS-staged raw weights packs nothing): the backward packs for itself; no-op for VAR_WAVE
    const bool need_pack = true;
    RowIO io;
    memset(&io, 0, sizeof(io));
    io.rows = rows; io.nseg = 1;
    io.seg[0].a = x; io.seg[0].ch = blocks[0].in_features; io.seg[0].off = 0;
    io.gy = gy; io.gx[0] = gx; io.saved = saved_inputs;
    io.row_store = (flags & CSMPN_FLAG_DETERMINISTIC) ? 1 : 0;   // standalone CEMLP: no row table, atomic-free parameter sums only
    // CSMPN_FLAG_SAVE_STATE: honoured exactly where csmpn_cemlp_forward honours it (include/csmpn_hip.h: the shapes of the
    // 16-row-tile family, whose standalone forward writes the state regions); everywhere else the standalone forward writes
    // no state, so a backward that honoured the flag would read rows nobody wrote
    io.save_state = ((flags & CSMPN_FLAG_SAVE_STATE) && pq_plain_shape(n, blocks, n_blocks)) ? 1 : 0;
    const bool tables_ready = io.save_state && (flags & CSMPN_FLAG_WEIGHTS_PACKED) != 0;
    return run_rows(plan, MODE_PLAIN, true, io, (hipStream_t)stream, need_pack, tables_ready);
}

// Fused simplex embedding (include/csmpn_hip.h): MODE_PLAIN of the wide parity-lane kernels with the embed descriptor
__global__ void index_range_kernel(const int* __restrict__ idx, long n, int hi, int* __restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (idx[i] < 0 || idx[i] >= hi)) atomicOr(flag, 1);
}
__device__ int g_range_flag;            // written by index_range_kernel, read back under g_range_mutex
static std::mutex g_range_mutex;

// every entry of idx[0, n) in [0, hi)? One host round trip (callers that have validated their tables pass
// CSMPN_FLAG_NO_VALIDATE; the kernels clamp in any case)
static int check_index_range(const int32_t* idx, int64_t n, int64_t hi, hipStream_t st, const char* what) {
    if (n <= 0) return CSMPN_OK;
    std::lock_guard<std::mutex> lock(g_range_mutex);
    int* flag = nullptr;
    hipError_t e = hipGetSymbolAddress(reinterpret_cast<void**>(&flag), HIP_SYMBOL(g_range_flag));
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e != hipSuccess) return fail(CSMPN_ERR_HIP, "%s validation: %s", what, hipGetErrorString(e));
    hipLaunchKernelGGL(index_range_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx, (long)n,
                       (int)(hi > 0x7fffffff ? 0x7fffffff : hi), flag);
    int host_flag = 0;
    e = hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(CSMPN_ERR_HIP, "%s validation: %s", what, hipGetErrorString(e));
    if (host_flag) return fail(CSMPN_ERR_INVALID, "%s has entries outside [0, %lld)", what, (long long)hi);
    return CSMPN_OK;
}

static int embed_io(const AlgId id, const csmpn_block_params* blocks, const float* vertex_feat, int64_t n_vertex_rows, int32_t kpv,
                    const int32_t* verts, int32_t nv, int32_t n_orders, int64_t n_rows, uint32_t flags, hipStream_t st, RowIO& io) {
    if (id != ALG_N5 && id != ALG_N5M) return fail(CSMPN_ERR_UNSUPPORTED, "fused embedding: Cl(5,0) / Cl(4,1) only");
    if (n_orders != 1 && n_orders != 2 && n_orders != 6) return fail(CSMPN_ERR_UNSUPPORTED, "fused embedding: 1, 2 or 6 vertex orders");
    if (!vertex_feat || !verts || kpv < 1 || nv < 1 || nv * kpv != blocks[0].in_features || nv * kpv > 8)
        return fail(CSMPN_ERR_UNSUPPORTED, "fused embedding: verts_per_row * channels_per_vertex must equal in_features (<= 8)");
    if (n_rows % n_orders) return fail(CSMPN_ERR_INVALID, "fused embedding: n_rows %ld is not a multiple of n_orders %d", (long)n_rows, n_orders);
    if (n_vertex_rows < 1 || n_vertex_rows > 0x7fffffff)
        return fail(CSMPN_ERR_INVALID, "fused embedding: n_vertex_rows %lld not in [1, 2^31)", (long long)n_vertex_rows);
    if (!(flags & CSMPN_FLAG_NO_VALIDATE)) {
        const int rc = check_index_range(verts, n_rows * nv, n_vertex_rows, st, "fused embedding: verts");
        if (rc) return rc;
    }
    memset(&io, 0, sizeof(io));
    io.rows = n_rows; io.nseg = 1;
    io.seg[0].a = vertex_feat; io.seg[0].ch = blocks[0].in_features; io.seg[0].off = 0;
    io.emb_verts = verts; io.emb_nperm = n_orders; io.emb_nv = nv; io.emb_k = kpv; io.emb_nrows = (int)n_vertex_rows;
    return CSMPN_OK;
}

int csmpn_embed_cemlp_forward(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* vertex_feat,
                              int64_t n_vertex_rows, int32_t channels_per_vertex, const int32_t* verts, int32_t verts_per_row, int32_t n_orders,
                              int64_t n_rows, float* out, float* save_inputs, void* workspace, size_t workspace_bytes,
                              uint32_t flags, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    RowIO io;
    int rc = embed_io(id, blocks, vertex_feat, n_vertex_rows, channels_per_vertex, verts, verts_per_row, n_orders, n_rows, flags,
                      (hipStream_t)stream, io);
    if (rc) return rc;
    Plan plan;
    if ((rc = make_plan(id, blocks, nullptr, n_blocks, workspace, workspace_bytes, false, 0, false, n_rows, plan))) return rc;
    io.y = out; io.save = save_inputs;
    if (!plw_serves(plan, MODE_PLAIN, false, io))
        return fail(CSMPN_ERR_UNSUPPORTED, "fused embedding: shape not served by the wide parity-lane kernels");
    io.save_state = (flags & CSMPN_FLAG_SAVE_STATE) ? 1 : 0;   // two-block modules: y, R, s of the blocks (as the EGCL stages)
    return run_rows(plan, MODE_PLAIN, false, io, (hipStream_t)stream, false);
}

int csmpn_embed_cemlp_backward(const float* metric, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                               int n_blocks, const float* vertex_feat, int64_t n_vertex_rows, int32_t channels_per_vertex,
                               const int32_t* verts, int32_t verts_per_row, int32_t n_orders, int64_t n_rows, const float* g_out,
                               const float* saved_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    RowIO io;
    int rc = embed_io(id, blocks, vertex_feat, n_vertex_rows, channels_per_vertex, verts, verts_per_row, n_orders, n_rows, flags,
                      (hipStream_t)stream, io);
    if (rc) return rc;
    Plan plan;
    if ((rc = make_plan(id, blocks, grads, n_blocks, workspace, workspace_bytes, true, 0, saved_inputs != nullptr, n_rows, plan))) return rc;
    io.gy = g_out; io.saved = saved_inputs;
    if (!plw_serves(plan, MODE_PLAIN, true, io))
        return fail(CSMPN_ERR_UNSUPPORTED, "fused embedding: shape not served by the wide parity-lane kernels (two blocks need saved inputs)");
    io.save_state = (flags & CSMPN_FLAG_SAVE_STATE) ? 1 : 0;
    return run_rows(plan, MODE_PLAIN, true, io, (hipStream_t)stream, false);
}

static int edge_io(const csmpn_block_params* blocks, const float* h, int channels, const float* edge_attr, int attr_channels,
                   const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, uint32_t flags, RowIO& io) {
    if (attr_channels > 0 && !edge_attr && E > 0) return fail(CSMPN_ERR_INVALID, "edge_attr is null");   // an empty edge list carries no attribute rows
    if (channels + attr_channels != blocks[0].in_features)
        return fail(CSMPN_ERR_INVALID, "edge model in_features %d != %d + %d", blocks[0].in_features, channels, attr_channels);
    memset(&io, 0, sizeof(io));
    io.rows = E; io.nseg = attr_channels > 0 ? 2 : 1;
    io.seg[0].a = h; io.seg[0].ia = dst_sorted; io.seg[0].b = h; io.seg[0].ib = src_sorted; io.seg[0].ch = channels;
    io.seg[1].a = edge_attr; io.seg[1].ia = perm; io.seg[1].ch = attr_channels; io.seg[1].off = channels;
    io.dst = dst_sorted; io.src = src_sorted; io.perm = perm;
    // deterministic: the forward's agg is the [E, O, D] message table, the backward's gh the [E, C, D] per-edge gradient table
    io.row_store = (flags & CSMPN_FLAG_DETERMINISTIC) ? 1 : 0;
    io.save_state = (flags & CSMPN_FLAG_SAVE_STATE) ? 1 : 0;
    return CSMPN_OK;
}

int csmpn_egcl_edge_forward(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* h,
                            int32_t channels, const float* edge_attr, int32_t attr_channels, const int32_t* perm,
                            const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N, float* agg,
                            float* save_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    RowIO io;
    int rc = edge_io(blocks, h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, flags, io);
    if (rc) return rc;
    Plan plan;
    if ((rc = make_plan(id, blocks, nullptr, n_blocks, workspace, workspace_bytes, false, blocks[n_blocks - 1].out_features << n, false,
                        E, plan, (flags & CSMPN_FLAG_DETERMINISTIC) != 0))) return rc;
    const bool need_pack = !(flags & CSMPN_FLAG_WEIGHTS_PACKED);   // packed fragments are a matter of the general kernels: run_rows
    io.agg = agg; io.save = save_inputs;
    io.gather_rows = N;
    return run_rows(plan, MODE_EDGE, false, io, (hipStream_t)stream, need_pack);
}

// deferred: run_rows (plan.hpp)
static int edge_backward(const float* metric, int n, const csmpn_block_params* blocks,
                         const csmpn_block_grads* grads, int n_blocks, const float* h, int32_t channels,
                         const float* edge_attr, int32_t attr_channels, const int32_t* perm,
                         const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N,
                         const float* g_agg, float* gh, float* g_edge_attr, const float* saved_inputs, void* workspace,
                         size_t workspace_bytes, uint32_t flags, void* stream, SliceSet* deferred) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    RowIO io;
    int rc = edge_io(blocks, h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, flags, io);
    if (rc) return rc;
    Plan plan;
    if ((rc = make_plan(id, blocks, grads, n_blocks, workspace, workspace_bytes, true, 0, saved_inputs != nullptr, E, plan,
                        (flags & CSMPN_FLAG_DETERMINISTIC) != 0))) return rc;
    // fragments packed by the forward are only valid for the forward's own layout choice (a forward
    // with LDS-staged raw weights packs nothing): the backward packs for itself; no-op for VAR_WAVE
    const bool need_pack = true;
    io.gy = g_agg; io.gx[0] = gh; io.gx[1] = g_edge_attr; io.saved = saved_inputs;
    io.gather_rows = N;
    return run_rows(plan, MODE_EDGE, true, io, (hipStream_t)stream, need_pack, (flags & CSMPN_FLAG_WEIGHTS_PACKED) != 0, deferred);
}

int csmpn_egcl_edge_backward(const float* metric, int n, const csmpn_block_params* blocks,
                             const csmpn_block_grads* grads, int n_blocks, const float* h, int32_t channels,
                             const float* edge_attr, int32_t attr_channels, const int32_t* perm,
                             const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N,
                             const float* g_agg, float* gh, float* g_edge_attr, const float* saved_inputs, void* workspace,
                             size_t workspace_bytes, uint32_t flags, void* stream) {
    return edge_backward(metric, n, blocks, grads, n_blocks, h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, N,
                         g_agg, gh, g_edge_attr, saved_inputs, workspace, workspace_bytes, flags, stream, nullptr);
}

static int node_io(const csmpn_block_params* blocks, int n_blocks, const float* h, int channels, const float* agg,
                   int agg_channels, const float* node_attr, int attr_channels, const int32_t* in_degree,
                   int mean_aggr, int residual, int64_t N, RowIO& io) {
    if (attr_channels > 0 && !node_attr) return fail(CSMPN_ERR_INVALID, "node_attr is null");
    if (channels + agg_channels + attr_channels != blocks[0].in_features)
        return fail(CSMPN_ERR_INVALID, "node model in_features %d != %d + %d + %d", blocks[0].in_features, channels,
                    agg_channels, attr_channels);
    if (residual && blocks[n_blocks - 1].out_features != channels)
        return fail(CSMPN_ERR_INVALID, "residual needs out_features == channels");
    if (mean_aggr && !in_degree) return fail(CSMPN_ERR_INVALID, "in_degree is null");
    memset(&io, 0, sizeof(io));
    io.rows = N; io.nseg = attr_channels > 0 ? 3 : 2;
    io.seg[0].a = h; io.seg[0].ch = channels; io.seg[0].off = 0;
    io.seg[1].a = agg; io.seg[1].ch = agg_channels; io.seg[1].off = channels;
    io.seg[1].deg = mean_aggr ? in_degree : nullptr;
    io.seg[2].a = node_attr; io.seg[2].ch = attr_channels; io.seg[2].off = channels + agg_channels;
    return CSMPN_OK;
}

int csmpn_egcl_node_forward(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* h,
                            int32_t channels, const float* agg, int32_t agg_channels, const float* node_attr,
                            int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr, int32_t residual,
                            int64_t N, float* out, float* save_inputs, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    RowIO io;
    int rc = node_io(blocks, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr,
                     residual, N, io);
    if (rc) return rc;
    Plan plan;
    if ((rc = make_plan(id, blocks, nullptr, n_blocks, workspace, workspace_bytes, false, 0, false, N, plan,
                        (flags & CSMPN_FLAG_DETERMINISTIC) != 0))) return rc;
    const bool need_pack = !(flags & CSMPN_FLAG_WEIGHTS_PACKED);   // packed fragments are a matter of the general kernels: run_rows
    io.y = out; io.resid = residual ? h : nullptr; io.save = save_inputs;
    io.row_store = (flags & CSMPN_FLAG_DETERMINISTIC) ? 1 : 0;   // node stage: no row table, only atomic-free kernels qualify
    io.save_state = (flags & CSMPN_FLAG_SAVE_STATE) ? 1 : 0;
    return run_rows(plan, MODE_NODE, false, io, (hipStream_t)stream, need_pack);
}

static int node_backward(const float* metric, int n, const csmpn_block_params* blocks,
                         const csmpn_block_grads* grads, int n_blocks, const float* h, int32_t channels,
                         const float* agg, int32_t agg_channels, const float* node_attr, int32_t attr_channels,
                         const int32_t* in_degree, int32_t mean_aggr, int32_t residual, int64_t N,
                         const float* g_out, float* gh, float* g_agg, float* g_node_attr, const float* saved_inputs, void* workspace,
                         size_t workspace_bytes, uint32_t flags, void* stream, SliceSet* deferred) {
    const AlgId id = alg_id(metric, n);
    if (id == ALG_NONE) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    RowIO io;
    int rc = node_io(blocks, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr,
                     residual, N, io);
    if (rc) return rc;
    Plan plan;
    if ((rc = make_plan(id, blocks, grads, n_blocks, workspace, workspace_bytes, true, 0, saved_inputs != nullptr, N, plan,
                        (flags & CSMPN_FLAG_DETERMINISTIC) != 0))) return rc;
    // fragments packed by the forward are only valid for the forward's own layout choice (a forward
    // with LDS-staged raw weights packs nothing): the backward packs for itself; no-op for VAR_WAVE
    const bool need_pack = true;
    io.gy = g_out; io.gx[0] = gh; io.gx[1] = g_agg; io.gx[2] = g_node_attr;
    io.resid_bwd = residual ? 1 : 0; io.saved = saved_inputs;
    io.row_store = (flags & CSMPN_FLAG_DETERMINISTIC) ? 1 : 0;
    io.save_state = (flags & CSMPN_FLAG_SAVE_STATE) ? 1 : 0;
    return run_rows(plan, MODE_NODE, true, io, (hipStream_t)stream, need_pack, (flags & CSMPN_FLAG_WEIGHTS_PACKED) != 0, deferred);
}

int csmpn_egcl_node_backward(const float* metric, int n, const csmpn_block_params* blocks,
                             const csmpn_block_grads* grads, int n_blocks, const float* h, int32_t channels,
                             const float* agg, int32_t agg_channels, const float* node_attr, int32_t attr_channels,
                             const int32_t* in_degree, int32_t mean_aggr, int32_t residual, int64_t N,
                             const float* g_out, float* gh, float* g_agg, float* g_node_attr, const float* saved_inputs, void* workspace,
                             size_t workspace_bytes, uint32_t flags, void* stream) {
    return node_backward(metric, n, blocks, grads, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr,
                         residual, N, g_out, gh, g_agg, g_node_attr, saved_inputs, workspace, workspace_bytes, flags, stream, nullptr);
}

// Both backwards of one layer. Where both stages end in a slice sum their unit can defer (LaneUnit::sum_slices: the
// (row, channel)-per-lane family), the node program's sum does not run in front of the edge backward, which needs only g_agg
// and gh: one launch behind the edge backward sums both programs' slices. The node workspace holds the node slices until
// then: nothing between the two stages touches it. Every other pair of families, and the deterministic mode: the two
// stages exactly as the separate entry points run them.
int csmpn_egcl_backward(const float* metric, int n, const csmpn_block_params* edge_blocks, const csmpn_block_grads* edge_grads,
                        int n_edge_blocks, const csmpn_block_params* node_blocks, const csmpn_block_grads* node_grads,
                        int n_node_blocks, const float* h, int32_t channels, const float* agg, int32_t agg_channels,
                        const float* edge_attr, int32_t edge_attr_channels, const float* node_attr, int32_t node_attr_channels,
                        const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* in_degree,
                        int32_t mean_aggr, int32_t residual, int64_t E, int64_t N, const float* g_out, float* gh, float* g_agg,
                        float* g_edge_attr, float* g_node_attr, float* g_edge_rows, const float* edge_saved, void* edge_workspace,
                        size_t edge_workspace_bytes, uint32_t edge_flags, const float* node_saved, void* node_workspace,
                        size_t node_workspace_bytes, uint32_t node_flags, void* stream) {
    const bool det = ((edge_flags | node_flags) & CSMPN_FLAG_DETERMINISTIC) != 0;
    if ((edge_flags & CSMPN_FLAG_DETERMINISTIC) && !g_edge_rows)
        return fail(CSMPN_ERR_INVALID, "CSMPN_FLAG_DETERMINISTIC: g_edge_rows ([E, C, D], csmpn_egcl_edge_backward's gh) is null");
    // the node slices wait in the node workspace while the edge backward runs: only if that one works elsewhere
    const char *we = static_cast<const char*>(edge_workspace), *wn = static_cast<const char*>(node_workspace);
    const bool apart = we && wn && (we + edge_workspace_bytes <= wn || wn + node_workspace_bytes <= we);
    SliceSet node_set, edge_set;
    node_set.unit = edge_set.unit = nullptr;
    const bool defer = !det && apart;
    int rc = node_backward(metric, n, node_blocks, node_grads, n_node_blocks, h, channels, agg, agg_channels, node_attr,
                           node_attr_channels, in_degree, mean_aggr, residual, N, g_out, gh, g_agg, g_node_attr, node_saved,
                           node_workspace, node_workspace_bytes, node_flags, stream, defer ? &node_set : nullptr);
    if (rc) return rc;
    // (a node stage that deferred nothing: the edge stage sums for itself as ever)
    rc = edge_backward(metric, n, edge_blocks, edge_grads, n_edge_blocks, h, channels, edge_attr, edge_attr_channels, perm, src_sorted,
                       dst_sorted, E, N, g_agg, (edge_flags & CSMPN_FLAG_DETERMINISTIC) ? g_edge_rows : gh, g_edge_attr, edge_saved,
                       edge_workspace, edge_workspace_bytes, edge_flags, stream, node_set.unit ? &edge_set : nullptr);
    if (node_set.unit) {
        // owed whatever became of the edge stage: the node gradients are complete when this entry returns without a HIP error
        const SliceSet* const other = (!rc && edge_set.unit == node_set.unit) ? &edge_set : nullptr;
        HIP_TRY(node_set.unit->sum_slices(node_set, other, (hipStream_t)stream));
        if (!rc && edge_set.unit && !other) HIP_TRY(edge_set.unit->sum_slices(edge_set, nullptr, (hipStream_t)stream));
    }
    return rc;
}

}  // extern "C"

