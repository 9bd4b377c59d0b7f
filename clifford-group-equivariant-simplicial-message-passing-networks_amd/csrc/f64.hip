// C-ABI of the float64 kernel family (include/csmpn_hip.h, "float64"): argument checks, the tile / workspace plan, the
// launches of cemlp_f64.hpp's kernels (one unit per algebra: k_f64_<tag>.hip) - or, for a signature that is none of the six
// compiled algebras, of cemlp_sig.hpp's double kernel on the same plan - and the two fixed-order sums. A rejected call
// launches nothing and writes nothing: every check stands in front of the first HIP call.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/csmpn_hip.h"
#include "capi_common.hpp"
#include "cemlp_f64.hpp"
#include "cemlp_sig.hpp"

#define fail csmpn_fail

namespace csmpn {
void note_kernel(const char* fmt, ...);   // capi.hip
namespace f64 {
#define CSMPN_F64_LAUNCHER(tag) hipError_t launch_##tag(bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args& a);
CSMPN_F64_LAUNCHER(n2) CSMPN_F64_LAUNCHER(n3) CSMPN_F64_LAUNCHER(n4) CSMPN_F64_LAUNCHER(n4m) CSMPN_F64_LAUNCHER(n5) CSMPN_F64_LAUNCHER(n5m)
#undef CSMPN_F64_LAUNCHER

// grads[t][e] += slice of workgroup 0, 1, .. grid - 1, in that order
struct SumArgs {
    double* dst[kMaxBlocks * kTensors];
    long off[kMaxBlocks * kTensors + 1];
    int n, grid;
    const double* ws;
    long wg_doubles;
};
__global__ __launch_bounds__(kThreads) void slices_sum_kernel(const SumArgs s) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= s.off[s.n]) return;
    int t = 0;
    while (e >= s.off[t + 1]) ++t;
    if (!s.dst[t]) return;
    double acc = s.dst[t][e - s.off[t]];
    for (int w = 0; w < s.grid; ++w) acc += s.ws[(long)w * s.wg_doubles + e];
    s.dst[t][e - s.off[t]] = acc;
}

__global__ __launch_bounds__(kThreads) void segment_reduce_f64_kernel(const double* __restrict__ rows, long row_doubles, long n_nodes,
                                                                      const int* __restrict__ add_ptr, const int* __restrict__ add_order,
                                                                      const int* __restrict__ sub_ptr, const int* __restrict__ sub_order,
                                                                      double* __restrict__ out, int accumulate) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_nodes * row_doubles) return;
    const long v = e / row_doubles, f = e - v * row_doubles;
    double acc = accumulate ? out[e] : 0.0;
    if (add_ptr)
        for (int k = add_ptr[v]; k < add_ptr[v + 1]; ++k) acc += rows[(long)(add_order ? add_order[k] : k) * row_doubles + f];
    if (sub_ptr)
        for (int k = sub_ptr[v]; k < sub_ptr[v + 1]; ++k) acc -= rows[(long)(sub_order ? sub_order[k] : k) * row_doubles + f];
    out[e] = acc;
}


namespace {
enum { MODE_PLAIN = 0, MODE_EDGE = 1, MODE_NODE = 2 };
typedef hipError_t (*Launcher)(bool, unsigned, size_t, hipStream_t, const Args&);

struct AlgInfo { Launcher launch; int P; const char* name; };

// the compiled algebras: the check of csmpn_metric_supported
bool find_alg(const float* metric, int n, AlgInfo& a) {
    if (!metric || n < 2 || n > 5) return false;
    unsigned neg = 0;
    for (int i = 0; i < n; ++i) {
        if (metric[i] == 1.0f) continue;
        if (metric[i] == -1.0f) { neg |= 1u << i; continue; }
        return false;
    }
    if (n == 2 && neg == 0) a = {launch_n2, Alg<2, 0u>::P, "Cl(2,0)"};
    else if (n == 3 && neg == 0) a = {launch_n3, Alg<3, 0u>::P, "Cl(3,0)"};
    else if (n == 4 && neg == 0) a = {launch_n4, Alg<4, 0u>::P, "Cl(4,0)"};
    else if (n == 4 && neg == 0x8u) a = {launch_n4m, Alg<4, 0x8u>::P, "Cl(3,1)"};
    else if (n == 5 && neg == 0) a = {launch_n5, Alg<5, 0u>::P, "Cl(5,0)"};
    else if (n == 5 && neg == 0x10u) a = {launch_n5m, Alg<5, 0x10u>::P, "Cl(4,1)"};
    else return false;
    return true;
}

int paths_of(int n) {   // the path count depends on n alone (the metric has no zero entry)
    return n == 2 ? Alg<2, 0u>::P : n == 3 ? Alg<3, 0u>::P : n == 4 ? Alg<4, 0u>::P : Alg<5, 0u>::P;
}

// Tile and workspace plan of one CEMLP for a launch of `rows` rows (include/csmpn_hip.h states the formula)
struct Plan {
    int R, maxO, maxW;
    unsigned grid;
    long tiles, slice, act, g, wg;
    long slice_off[kMaxBlocks], act_off[kMaxBlocks];
    size_t lds, bytes;
};

// shape checks shared by the query and the entry points; 0 or the error code (message set)
int make_plan(int n, const csmpn_block_params_f64* b, int nb, int64_t rows, Plan& p) {
    if (!b) return fail(CSMPN_ERR_INVALID, "float64: blocks is null");
    if (n < 2 || n > 5) return fail(CSMPN_ERR_UNSUPPORTED, "float64: n=%d not in 2..5", n);
    if (nb < 1 || nb > CSMPN_MAX_BLOCKS) return fail(CSMPN_ERR_INVALID, "float64: %d blocks not in 1..%d", nb, CSMPN_MAX_BLOCKS);
    if (rows < 0) return fail(CSMPN_ERR_INVALID, "float64: negative row count %lld", (long long)rows);
    const int D = 1 << n, G = n + 1, P = paths_of(n);
    p.maxO = p.maxW = 0; p.slice = p.act = 0;
    for (int k = 0; k < nb; ++k) {
        const int I = b[k].in_features, O = b[k].out_features;
        if (I < 1 || O < 1) return fail(CSMPN_ERR_INVALID, "float64: block %d has in_features %d, out_features %d", k, I, O);
        if (O > kMaxWidth)
            return fail(CSMPN_ERR_UNSUPPORTED, "float64: out_features %d of block %d is above the limit of %d channels", O, k, kMaxWidth);
        if (k > 0 && I != b[k - 1].out_features)
            return fail(CSMPN_ERR_INVALID, "float64: in_features %d of block %d != out_features %d of block %d", I, k, b[k - 1].out_features, k - 1);
        p.maxO = O > p.maxO ? O : p.maxO;
        p.maxW = (I > p.maxW ? I : p.maxW); p.maxW = (O > p.maxW ? O : p.maxW);
        p.slice_off[k] = p.slice;
        p.slice += (long)O * I * (b[k].lin_subspaces ? G : 1) + 3L * O + 3L * O * G + (long)O * P + 2L * O * O * G;
    }
    const size_t row_bytes = sizeof(double) * (size_t)lds_row_doubles(p.maxO, D, G);
    p.R = (int)(kLdsSmall / row_bytes);
    if (p.R > kMaxTileRows) p.R = kMaxTileRows;
    if (p.R < 1) p.R = (int)(kLdsMax / row_bytes);
    if (p.R < 1) return fail(CSMPN_ERR_UNSUPPORTED, "float64: one row of %d channels does not fit the LDS", p.maxO);
    p.lds = row_bytes * p.R;
    for (int k = 0; k < nb; ++k) { p.act_off[k] = p.act; p.act += (long)p.R * b[k].in_features * D; }
    p.g = (long)p.R * p.maxW * D;
    p.wg = p.slice + p.act + 2 * p.g;
    p.tiles = (long)((rows + p.R - 1) / p.R);
    const long cap = p.lds <= kLdsSmall ? 2L * kGridCap : kGridCap;   // two workgroups per CU where the LDS allows it
    p.grid = (unsigned)(p.tiles < cap ? p.tiles : cap);
    p.bytes = sizeof(double) * (size_t)p.wg * p.grid;
    return CSMPN_OK;
}

bool debug_on() {
    static const bool on = getenv("CSMPN_DEBUG") != nullptr;
    return on;
}

int fill_blocks(const csmpn_block_params_f64* b, int nb, const Plan& p, Args& a) {
    for (int k = 0; k < nb; ++k) {
        if (!b[k].lin_w || !b[k].silu_a || !b[k].silu_b || !b[k].gp_w || !b[k].norm_a || !b[k].right_w || !b[k].left_w || !b[k].left_b ||
            !b[k].ln_a)
            return fail(CSMPN_ERR_INVALID, "float64: block %d has a null parameter pointer", k);
        a.blk[k] = Blk{b[k].in_features, b[k].out_features, b[k].lin_subspaces ? 1 : 0, b[k].lin_w, b[k].lin_b, b[k].silu_a, b[k].silu_b,
                       b[k].gp_w, b[k].norm_a, b[k].right_w, b[k].left_w, b[k].left_b, b[k].ln_a, p.slice_off[k], p.act_off[k]};
    }
    a.nblk = nb; a.R = p.R; a.maxO = p.maxO; a.tiles = p.tiles;
    a.wg_doubles = p.wg; a.slice_doubles = p.slice; a.act_doubles = p.act; a.g_doubles = p.g;
    return CSMPN_OK;
}

// One stage: the checks every entry point shares, then the row kernel and (backward) the slice sum. `a` arrives with its
// segments and row pointers set.
int run(const float* metric, int n, const csmpn_block_params_f64* blocks, const csmpn_block_grads_f64* grads, int nb, int mode, bool bwd,
        int64_t rows, Args& a, void* ws, size_t ws_bytes, hipStream_t st) {
    AlgInfo alg = {nullptr, 0, ""};
    unsigned neg = 0;
    if (!metric) return fail(CSMPN_ERR_INVALID, "float64: metric is null");
    if (!sig::parse_signature(metric, n, neg)) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    // the six compiled algebras keep their kernel; every other signature (and all of them under CSMPN_FORCE_SIG=1) runs the
    // run-time-signature kernel (cemlp_sig.hpp) on the same plan
    const bool use_sig = !find_alg(metric, n, alg) || sig::force_sig();
    Plan p;
    int rc = make_plan(n, blocks, nb, rows, p);
    if (rc) return rc;
    if (bwd && !grads) return fail(CSMPN_ERR_INVALID, "float64: grads is null");
    if ((rc = fill_blocks(blocks, nb, p, a))) return rc;
    int in = 0;
    for (int s = 0; s < a.nseg; ++s) { a.seg[s].off = in; in += a.seg[s].ch; }
    if (in != blocks[0].in_features) return fail(CSMPN_ERR_INVALID, "float64: in_features %d != %d input channels", blocks[0].in_features, in);
    if (ws_bytes < p.bytes || (p.bytes && !ws))
        return fail(CSMPN_ERR_INVALID, "float64: workspace of %zu bytes, %zu needed (csmpn_cemlp_f64_workspace_bytes)", ws_bytes, p.bytes);
    a.rows = rows; a.ws = static_cast<double*>(ws);
    if (use_sig)
        note_kernel("csmpn::sig::cemlp_sig_kernel<%d, double, %s> (signature 0x%x, mode %d, %d blocks, %d channels)", n, bwd ? "bwd" : "fwd",
                    neg, mode, nb, p.maxO);
    else
        note_kernel("csmpn::f64::cemlp_f64_kernel<%s, %s> (mode %d, %d blocks, %d channels)", alg.name, bwd ? "bwd" : "fwd", mode, nb, p.maxO);
    if (debug_on() && use_sig)
        fprintf(stderr, "[csmpn] sig dtype=f64 n=%d neg=0x%x mode=%d bwd=%d channels=%d i0=%d grid=%u tile_rows=%d tiles=%ld lds=%zu rows=%ld\n",
                n, neg, mode, (int)bwd, p.maxO, blocks[0].in_features, p.grid, p.R, p.tiles, p.lds + sig::table_bytes(1 << n), (long)rows);
    else if (debug_on())
        fprintf(stderr, "[csmpn] f64 mode=%d bwd=%d channels=%d i0=%d grid=%u tile_rows=%d tiles=%ld lds=%zu rows=%ld\n", mode, (int)bwd, p.maxO,
                blocks[0].in_features, p.grid, p.R, p.tiles, p.lds, (long)rows);
    if (p.grid == 0) return CSMPN_OK;
    hipError_t e = use_sig ? sig::launch_f64(n, neg, bwd, p.grid, p.lds, st, a) : alg.launch(bwd, p.grid, p.lds, st, a);
    if (e != hipSuccess) return fail(CSMPN_ERR_HIP, "float64 row kernel: %s", hipGetErrorString(e));
    if (bwd) {
        SumArgs s;
        memset(&s, 0, sizeof(s));
        const int G = n + 1;
        long off = 0;
        for (int k = 0; k < nb; ++k) {
            const long O = blocks[k].out_features, I = blocks[k].in_features;
            double* const dst[kTensors] = {grads[k].lin_w, grads[k].lin_b, grads[k].silu_a, grads[k].silu_b, grads[k].gp_w,
                                           grads[k].norm_a, grads[k].right_w, grads[k].left_w, grads[k].left_b, grads[k].ln_a};
            const long size[kTensors] = {O * I * (blocks[k].lin_subspaces ? G : 1), O, O * G, O * G, O * (long)paths_of(n), O * G, O * O * G, O * O * G, O, O};
            for (int t = 0; t < kTensors; ++t) { s.dst[s.n] = dst[t]; s.off[s.n] = off; off += size[t]; ++s.n; }
        }
        s.off[s.n] = off;
        s.grid = (int)p.grid; s.ws = a.ws; s.wg_doubles = p.wg;
        hipLaunchKernelGGL(slices_sum_kernel, dim3((unsigned)((off + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, s);
        if ((e = hipGetLastError()) != hipSuccess) return fail(CSMPN_ERR_HIP, "float64 slice sum: %s", hipGetErrorString(e));
    }
    return CSMPN_OK;
}
}  // namespace
}  // namespace f64
}  // namespace csmpn

using namespace csmpn::f64;

extern "C" {

size_t csmpn_cemlp_f64_workspace_bytes(int n, const csmpn_block_params_f64* blocks, int n_blocks, int64_t rows) {
    Plan p;
    return make_plan(n, blocks, n_blocks, rows, p) ? 0 : p.bytes;
}

int csmpn_cemlp_forward_f64(const float* metric, int n, const csmpn_block_params_f64* blocks, int n_blocks, const double* x, int64_t rows,
                            double* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows > 0 && (!x || !y)) return fail(CSMPN_ERR_INVALID, "float64: x or y is null");
    Args a;
    memset(&a, 0, sizeof(a));
    a.nseg = 1;
    a.seg[0].a = x; a.seg[0].ch = blocks ? blocks[0].in_features : 0; a.seg[0].a_rows = rows;
    a.y = y;
    return run(metric, n, blocks, nullptr, n_blocks, MODE_PLAIN, false, rows, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_cemlp_backward_f64(const float* metric, int n, const csmpn_block_params_f64* blocks, const csmpn_block_grads_f64* grads,
                             int n_blocks, const double* x, const double* gy, int64_t rows, double* gx, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (rows > 0 && (!x || !gy)) return fail(CSMPN_ERR_INVALID, "float64: x or gy is null");
    Args a;
    memset(&a, 0, sizeof(a));
    a.nseg = 1;
    a.seg[0].a = x; a.seg[0].ch = blocks ? blocks[0].in_features : 0; a.seg[0].a_rows = rows; a.seg[0].g = gx;
    a.gy = gy; a.gy_rows = rows;
    return run(metric, n, blocks, grads, n_blocks, MODE_PLAIN, true, rows, a, workspace, workspace_bytes, (hipStream_t)stream);
}

static int edge_args(const double* h, int32_t channels, const double* edge_attr, int32_t attr_channels, const int32_t* perm,
                     const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N, Args& a) {
    if (N < 0) return fail(CSMPN_ERR_INVALID, "float64: negative node count %lld", (long long)N);
    if (channels < 1 || attr_channels < 0) return fail(CSMPN_ERR_INVALID, "float64: %d channels, %d attribute channels", channels, attr_channels);
    if (E > 0 && (!h || !perm || !src_sorted || !dst_sorted || N < 1)) return fail(CSMPN_ERR_INVALID, "float64: h or an index table is null");
    if (E > 0 && attr_channels > 0 && !edge_attr) return fail(CSMPN_ERR_INVALID, "edge_attr is null");
    memset(&a, 0, sizeof(a));
    a.nseg = attr_channels > 0 ? 2 : 1;
    a.seg[0].a = h; a.seg[0].ia = dst_sorted; a.seg[0].b = h; a.seg[0].ib = src_sorted; a.seg[0].ch = channels; a.seg[0].a_rows = N;
    a.seg[1].a = edge_attr; a.seg[1].ia = perm; a.seg[1].ch = attr_channels; a.seg[1].a_rows = E;
    return CSMPN_OK;
}

int csmpn_egcl_edge_forward_f64(const float* metric, int n, const csmpn_block_params_f64* blocks, int n_blocks, const double* h,
                                int32_t channels, const double* edge_attr, int32_t attr_channels, const int32_t* perm,
                                const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N, double* msg_rows,
                                void* workspace, size_t workspace_bytes, void* stream) {
    Args a;
    int rc = edge_args(h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, N, a);
    if (rc) return rc;
    if (E > 0 && !msg_rows) return fail(CSMPN_ERR_INVALID, "float64: msg_rows is null");
    a.y = msg_rows;
    return run(metric, n, blocks, nullptr, n_blocks, MODE_EDGE, false, E, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_egcl_edge_backward_f64(const float* metric, int n, const csmpn_block_params_f64* blocks, const csmpn_block_grads_f64* grads,
                                 int n_blocks, const double* h, int32_t channels, const double* edge_attr, int32_t attr_channels,
                                 const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N,
                                 const double* g_agg, double* g_edge_rows, double* g_edge_attr, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    Args a;
    int rc = edge_args(h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, N, a);
    if (rc) return rc;
    if (E > 0 && (!g_agg || !g_edge_rows)) return fail(CSMPN_ERR_INVALID, "float64: g_agg or g_edge_rows is null");
    a.gy = g_agg; a.gy_idx = dst_sorted; a.gy_rows = N;
    a.seg[0].g = g_edge_rows;
    a.seg[1].g = g_edge_attr; a.seg[1].gi = perm;
    return run(metric, n, blocks, grads, n_blocks, MODE_EDGE, true, E, a, workspace, workspace_bytes, (hipStream_t)stream);
}

static int node_args(const csmpn_block_params_f64* blocks, int n_blocks, const double* h, int32_t channels, const double* agg,
                     int32_t agg_channels, const double* node_attr, int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr,
                     int32_t residual, int64_t N, Args& a) {
    if (channels < 1 || agg_channels < 1 || attr_channels < 0)
        return fail(CSMPN_ERR_INVALID, "float64: %d channels, %d aggregate channels, %d attribute channels", channels, agg_channels, attr_channels);
    if (N > 0 && (!h || !agg)) return fail(CSMPN_ERR_INVALID, "float64: h or agg is null");
    if (N > 0 && attr_channels > 0 && !node_attr) return fail(CSMPN_ERR_INVALID, "node_attr is null");
    if (N > 0 && mean_aggr && !in_degree) return fail(CSMPN_ERR_INVALID, "in_degree is null");
    if (residual && blocks && n_blocks >= 1 && n_blocks <= CSMPN_MAX_BLOCKS && blocks[n_blocks - 1].out_features != channels)
        return fail(CSMPN_ERR_INVALID, "residual needs out_features == channels");
    memset(&a, 0, sizeof(a));
    a.nseg = attr_channels > 0 ? 3 : 2;
    a.seg[0].a = h; a.seg[0].ch = channels; a.seg[0].a_rows = N;
    a.seg[1].a = agg; a.seg[1].ch = agg_channels; a.seg[1].a_rows = N; a.seg[1].deg = mean_aggr ? in_degree : nullptr;
    a.seg[2].a = node_attr; a.seg[2].ch = attr_channels; a.seg[2].a_rows = N;
    return CSMPN_OK;
}

int csmpn_egcl_node_forward_f64(const float* metric, int n, const csmpn_block_params_f64* blocks, int n_blocks, const double* h,
                                int32_t channels, const double* agg, int32_t agg_channels, const double* node_attr, int32_t attr_channels,
                                const int32_t* in_degree, int32_t mean_aggr, int32_t residual, int64_t N, double* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    Args a;
    int rc = node_args(blocks, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr, residual, N, a);
    if (rc) return rc;
    if (N > 0 && !out) return fail(CSMPN_ERR_INVALID, "float64: out is null");
    a.y = out; a.resid = residual ? h : nullptr;
    return run(metric, n, blocks, nullptr, n_blocks, MODE_NODE, false, N, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_egcl_node_backward_f64(const float* metric, int n, const csmpn_block_params_f64* blocks, const csmpn_block_grads_f64* grads,
                                 int n_blocks, const double* h, int32_t channels, const double* agg, int32_t agg_channels,
                                 const double* node_attr, int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr,
                                 int32_t residual, int64_t N, const double* g_out, double* gh, double* g_agg, double* g_node_attr,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    Args a;
    int rc = node_args(blocks, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr, residual, N, a);
    if (rc) return rc;
    if (N > 0 && (!g_out || !gh || !g_agg)) return fail(CSMPN_ERR_INVALID, "float64: g_out, gh or g_agg is null");
    a.gy = g_out; a.gy_rows = N; a.resid_bwd = residual ? 1 : 0;
    a.seg[0].g = gh; a.seg[1].g = g_agg; a.seg[2].g = g_node_attr;
    return run(metric, n, blocks, grads, n_blocks, MODE_NODE, true, N, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_segment_reduce_f64(const double* rows, int64_t row_doubles, int64_t n_nodes, const int32_t* add_ptr, const int32_t* add_order,
                             const int32_t* sub_ptr, const int32_t* sub_order, double* out, int32_t accumulate, void* stream) {
    if (n_nodes < 0 || row_doubles < 1) return fail(CSMPN_ERR_INVALID, "float64 segment sum: %lld nodes of %lld doubles", (long long)n_nodes, (long long)row_doubles);
    if (n_nodes == 0) return CSMPN_OK;
    if (!out || ((add_ptr || sub_ptr) && !rows)) return fail(CSMPN_ERR_INVALID, "float64 segment sum: rows or out is null");
    const long total = (long)n_nodes * row_doubles;
    hipLaunchKernelGGL(segment_reduce_f64_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       rows, (long)row_doubles, (long)n_nodes, add_ptr, add_order, sub_ptr, sub_order, out, (int)accumulate);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CSMPN_ERR_HIP, "float64 segment sum: %s", hipGetErrorString(e));
    return CSMPN_OK;
}

}  // extern "C"
