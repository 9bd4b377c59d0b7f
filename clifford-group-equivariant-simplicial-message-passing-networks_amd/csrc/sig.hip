// C-ABI of the run-time-signature kernel family (include/csmpn_hip.h, "run-time signature"): csmpn_signature_supported, the
// seven float32 *_sig entry points (argument checks, the float tile / workspace plan, the launches of cemlp_sig.hpp's
// kernels - one unit per n: k_sig_n<n>.hip - and the fixed-order slice sum) and the double launch that f64.hip uses for
// the signatures it has no compiled algebra for. A rejected call launches nothing and writes nothing: every check stands
// in front of the first HIP call.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/csmpn_hip.h"
#include "capi_common.hpp"
#include "cemlp_sig.hpp"

#define fail csmpn_fail

namespace csmpn {
void note_kernel(const char* fmt, ...);   // capi.hip
namespace sig {
#define CSMPN_SIG_LAUNCHER(tag)                                                                              \
    hipError_t launch_##tag(bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args<float>& a);      \
    hipError_t launch_##tag(bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args<double>& a);
CSMPN_SIG_LAUNCHER(n2) CSMPN_SIG_LAUNCHER(n3) CSMPN_SIG_LAUNCHER(n4) CSMPN_SIG_LAUNCHER(n5)
#undef CSMPN_SIG_LAUNCHER

bool parse_signature(const float* metric, int n, unsigned& neg) {
    if (!metric || n < 2 || n > 5) return false;
    neg = 0;
    for (int i = 0; i < n; ++i) {
        if (metric[i] == 1.0f) continue;
        if (metric[i] == -1.0f) { neg |= 1u << i; continue; }
        return false;
    }
    return true;
}

bool force_sig() {
    static const bool on = [] { const char* v = getenv("CSMPN_FORCE_SIG"); return v && v[0] == '1' && !v[1]; }();
    return on;
}

template <class Real>
static hipError_t launch(int n, bool bwd, unsigned grid, size_t lds, hipStream_t st, const Args<Real>& a) {
    switch (n) {
        case 2: return launch_n2(bwd, grid, lds, st, a);
        case 3: return launch_n3(bwd, grid, lds, st, a);
        case 4: return launch_n4(bwd, grid, lds, st, a);
        case 5: return launch_n5(bwd, grid, lds, st, a);
    }
    return hipErrorInvalidValue;
}

// the float64 stage `a` of f64.hip (checked, planned and filled there) on the sig kernel of signature `neg`;
// lds_rows = the plan's LDS bytes for the tile state, the sign table goes behind it
hipError_t launch_f64(int n, unsigned neg, bool bwd, unsigned grid, size_t lds_rows, hipStream_t st, const f64::Args& a) {
    Args<double> s;
    memset(&s, 0, sizeof(s));
    for (int k = 0; k < a.nblk; ++k) {
        const f64::Blk& b = a.blk[k];
        s.blk[k] = Blk<double>{b.I, b.O, b.sub, b.W1, b.b1, b.sa, b.sb, b.w, b.an, b.WR, b.WL, b.bL, b.la, b.slice_off, b.act_off};
    }
    for (int k = 0; k < 3; ++k) {
        const f64::Seg& g = a.seg[k];
        s.seg[k] = Seg<double>{g.a, g.b, g.ia, g.ib, g.deg, g.gi, g.g, g.ch, g.off, g.a_rows};
    }
    s.nblk = a.nblk; s.nseg = a.nseg; s.R = a.R; s.maxO = a.maxO; s.resid_bwd = a.resid_bwd; s.neg = neg;
    s.rows = a.rows; s.tiles = a.tiles; s.gy_rows = a.gy_rows;
    s.y = a.y; s.resid = a.resid; s.gy = a.gy; s.gy_idx = a.gy_idx; s.ws = a.ws;
    s.wg_elems = a.wg_doubles; s.slice_elems = a.slice_doubles; s.act_elems = a.act_doubles; s.g_elems = a.g_doubles;
    return launch<double>(n, bwd, grid, lds_rows + table_bytes(1 << n), st, s);
}

namespace {
// grads[t][e] += slice of workgroup 0, 1, .. grid - 1, in that order (f64.hip's slices_sum_kernel on floats)
struct SumArgs {
    float* dst[kMaxBlocks * kTensors];
    long off[kMaxBlocks * kTensors + 1];
    int n, grid;
    const float* ws;
    long wg_elems;
};
__global__ __launch_bounds__(kThreads) void slices_sum_f32_kernel(const SumArgs s) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= s.off[s.n]) return;
    int t = 0;
    while (e >= s.off[t + 1]) ++t;
    if (!s.dst[t]) return;
    float acc = s.dst[t][e - s.off[t]];
    for (int w = 0; w < s.grid; ++w) acc += s.ws[(long)w * s.wg_elems + e];
    s.dst[t][e - s.off[t]] = acc;
}

enum { MODE_PLAIN = 0, MODE_EDGE = 1, MODE_NODE = 2 };
typedef Args<float> ArgsF;

int paths_of(int n) {   // the path count depends on n alone (the metric has no zero entry)
    return n == 2 ? Alg<2, 0u>::P : n == 3 ? Alg<3, 0u>::P : n == 4 ? Alg<4, 0u>::P : Alg<5, 0u>::P;
}

// Tile and workspace plan of one float CEMLP for a launch of `rows` rows (include/csmpn_hip.h states the formula)
struct Plan {
    int R, maxO, maxW;
    unsigned grid;
    long tiles, slice, act, g, wg;
    long slice_off[kMaxBlocks], act_off[kMaxBlocks];
    size_t lds, bytes;
};

// shape checks shared by the query and the entry points; 0 or the error code (message set)
int make_plan(int n, const csmpn_block_params* b, int nb, int64_t rows, Plan& p) {
    if (!b) return fail(CSMPN_ERR_INVALID, "sig: blocks is null");
    if (n < 2 || n > 5) return fail(CSMPN_ERR_UNSUPPORTED, "sig: n=%d not in 2..5", n);
    if (nb < 1 || nb > CSMPN_MAX_BLOCKS) return fail(CSMPN_ERR_INVALID, "sig: %d blocks not in 1..%d", nb, CSMPN_MAX_BLOCKS);
    if (rows < 0) return fail(CSMPN_ERR_INVALID, "sig: negative row count %lld", (long long)rows);
    const int D = 1 << n, G = n + 1, P = paths_of(n);
    p.maxO = p.maxW = 0; p.slice = p.act = 0;
    for (int k = 0; k < nb; ++k) {
        const int I = b[k].in_features, O = b[k].out_features;
        if (I < 1 || O < 1) return fail(CSMPN_ERR_INVALID, "sig: block %d has in_features %d, out_features %d", k, I, O);
        if (O > kMaxWidth)
            return fail(CSMPN_ERR_UNSUPPORTED, "sig: out_features %d of block %d is above the limit of %d channels", O, k, kMaxWidth);
        if (k > 0 && I != b[k - 1].out_features)
            return fail(CSMPN_ERR_INVALID, "sig: in_features %d of block %d != out_features %d of block %d", I, k, b[k - 1].out_features, k - 1);
        p.maxO = O > p.maxO ? O : p.maxO;
        p.maxW = (I > p.maxW ? I : p.maxW); p.maxW = (O > p.maxW ? O : p.maxW);
        p.slice_off[k] = p.slice;
        p.slice += (long)O * I * (b[k].lin_subspaces ? G : 1) + 3L * O + 3L * O * G + (long)O * P + 2L * O * O * G;
    }
    const size_t row_bytes = sizeof(float) * (size_t)lds_row_elems(p.maxO, D, G), tb = table_bytes(D);
    p.R = (int)((kLdsSmall - tb) / row_bytes);
    if (p.R > kMaxTileRows) p.R = kMaxTileRows;
    if (p.R < 1) p.R = (int)((kLdsMax - tb) / row_bytes);
    if (p.R < 1) return fail(CSMPN_ERR_UNSUPPORTED, "sig: one row of %d channels does not fit the LDS", p.maxO);
    p.lds = row_bytes * p.R + tb;
    for (int k = 0; k < nb; ++k) { p.act_off[k] = p.act; p.act += (long)p.R * b[k].in_features * D; }
    p.g = (long)p.R * p.maxW * D;
    p.wg = p.slice + p.act + 2 * p.g;
    p.tiles = (long)((rows + p.R - 1) / p.R);
    const long cap = p.lds <= kLdsSmall ? 2L * kGridCap : kGridCap;   // two workgroups per CU where the LDS allows it
    p.grid = (unsigned)(p.tiles < cap ? p.tiles : cap);
    p.bytes = sizeof(float) * (size_t)p.wg * p.grid;
    return CSMPN_OK;
}

bool debug_on() {
    static const bool on = getenv("CSMPN_DEBUG") != nullptr;
    return on;
}

int fill_blocks(const csmpn_block_params* b, int nb, const Plan& p, ArgsF& a) {
    for (int k = 0; k < nb; ++k) {
        if (!b[k].lin_w || !b[k].silu_a || !b[k].silu_b || !b[k].gp_w || !b[k].norm_a || !b[k].right_w || !b[k].left_w || !b[k].left_b ||
            !b[k].ln_a)
            return fail(CSMPN_ERR_INVALID, "sig: block %d has a null parameter pointer", k);
        a.blk[k] = Blk<float>{b[k].in_features, b[k].out_features, b[k].lin_subspaces ? 1 : 0, b[k].lin_w, b[k].lin_b, b[k].silu_a,
                              b[k].silu_b, b[k].gp_w, b[k].norm_a, b[k].right_w, b[k].left_w, b[k].left_b, b[k].ln_a, p.slice_off[k],
                              p.act_off[k]};
    }
    a.nblk = nb; a.R = p.R; a.maxO = p.maxO; a.tiles = p.tiles;
    a.wg_elems = p.wg; a.slice_elems = p.slice; a.act_elems = p.act; a.g_elems = p.g;
    return CSMPN_OK;
}

// One float stage: the checks every entry point shares, then the row kernel and (backward) the slice sum. `a` arrives
// with its segments and row pointers set.
int run(const float* metric, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads, int nb, int mode, bool bwd,
        int64_t rows, ArgsF& a, void* ws, size_t ws_bytes, hipStream_t st) {
    unsigned neg = 0;
    if (!metric) return fail(CSMPN_ERR_INVALID, "sig: metric is null");
    if (!parse_signature(metric, n, neg)) return fail(CSMPN_ERR_UNSUPPORTED, "metric not supported by the HIP path");
    Plan p;
    int rc = make_plan(n, blocks, nb, rows, p);
    if (rc) return rc;
    if (bwd && !grads) return fail(CSMPN_ERR_INVALID, "sig: grads is null");
    if ((rc = fill_blocks(blocks, nb, p, a))) return rc;
    int in = 0;
    for (int s = 0; s < a.nseg; ++s) { a.seg[s].off = in; in += a.seg[s].ch; }
    if (in != blocks[0].in_features) return fail(CSMPN_ERR_INVALID, "sig: in_features %d != %d input channels", blocks[0].in_features, in);
    if (ws_bytes < p.bytes || (p.bytes && !ws))
        return fail(CSMPN_ERR_INVALID, "sig: workspace of %zu bytes, %zu needed (csmpn_cemlp_sig_workspace_bytes)", ws_bytes, p.bytes);
    a.rows = rows; a.ws = static_cast<float*>(ws); a.neg = neg;
    note_kernel("csmpn::sig::cemlp_sig_kernel<%d, float, %s> (signature 0x%x, mode %d, %d blocks, %d channels)", n, bwd ? "bwd" : "fwd", neg,
                mode, nb, p.maxO);
    if (debug_on())
        fprintf(stderr, "[csmpn] sig dtype=f32 n=%d neg=0x%x mode=%d bwd=%d channels=%d i0=%d grid=%u tile_rows=%d tiles=%ld lds=%zu rows=%ld\n",
                n, neg, mode, (int)bwd, p.maxO, blocks[0].in_features, p.grid, p.R, p.tiles, p.lds, (long)rows);
    if (p.grid == 0) return CSMPN_OK;
    hipError_t e = launch<float>(n, bwd, p.grid, p.lds, st, a);
    if (e != hipSuccess) return fail(CSMPN_ERR_HIP, "sig row kernel: %s", hipGetErrorString(e));
    if (bwd) {
        SumArgs s;
        memset(&s, 0, sizeof(s));
        const int G = n + 1, P = paths_of(n);
        long off = 0;
        for (int k = 0; k < nb; ++k) {
            const long O = blocks[k].out_features, I = blocks[k].in_features;
            float* const dst[kTensors] = {grads[k].lin_w, grads[k].lin_b, grads[k].silu_a, grads[k].silu_b, grads[k].gp_w,
                                          grads[k].norm_a, grads[k].right_w, grads[k].left_w, grads[k].left_b, grads[k].ln_a};
            const long size[kTensors] = {O * I * (blocks[k].lin_subspaces ? G : 1), O, O * G, O * G, O * P, O * G, O * O * G, O * O * G, O, O};
            for (int t = 0; t < kTensors; ++t) { s.dst[s.n] = dst[t]; s.off[s.n] = off; off += size[t]; ++s.n; }
        }
        s.off[s.n] = off;
        s.grid = (int)p.grid; s.ws = a.ws; s.wg_elems = p.wg;
        hipLaunchKernelGGL(slices_sum_f32_kernel, dim3((unsigned)((off + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, s);
        if ((e = hipGetLastError()) != hipSuccess) return fail(CSMPN_ERR_HIP, "sig slice sum: %s", hipGetErrorString(e));
    }
    return CSMPN_OK;
}

int edge_args(const float* h, int32_t channels, const float* edge_attr, int32_t attr_channels, const int32_t* perm,
              const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N, ArgsF& a) {
    if (N < 0) return fail(CSMPN_ERR_INVALID, "sig: negative node count %lld", (long long)N);
    if (channels < 1 || attr_channels < 0) return fail(CSMPN_ERR_INVALID, "sig: %d channels, %d attribute channels", channels, attr_channels);
    if (E > 0 && (!h || !perm || !src_sorted || !dst_sorted || N < 1)) return fail(CSMPN_ERR_INVALID, "sig: h or an index table is null");
    if (E > 0 && attr_channels > 0 && !edge_attr) return fail(CSMPN_ERR_INVALID, "edge_attr is null");
    memset(&a, 0, sizeof(a));
    a.nseg = attr_channels > 0 ? 2 : 1;
    a.seg[0].a = h; a.seg[0].ia = dst_sorted; a.seg[0].b = h; a.seg[0].ib = src_sorted; a.seg[0].ch = channels; a.seg[0].a_rows = N;
    a.seg[1].a = edge_attr; a.seg[1].ia = perm; a.seg[1].ch = attr_channels; a.seg[1].a_rows = E;
    return CSMPN_OK;
}

int node_args(const csmpn_block_params* blocks, int n_blocks, const float* h, int32_t channels, const float* agg, int32_t agg_channels,
              const float* node_attr, int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr, int32_t residual, int64_t N,
              ArgsF& a) {
    if (channels < 1 || agg_channels < 1 || attr_channels < 0)
        return fail(CSMPN_ERR_INVALID, "sig: %d channels, %d aggregate channels, %d attribute channels", channels, agg_channels, attr_channels);
    if (N > 0 && (!h || !agg)) return fail(CSMPN_ERR_INVALID, "sig: h or agg is null");
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
}  // namespace
}  // namespace sig
}  // namespace csmpn

using namespace csmpn::sig;

extern "C" {

int csmpn_signature_supported(const float* metric_host, int n) {
    unsigned neg;
    return parse_signature(metric_host, n, neg) ? 1 : 0;
}

size_t csmpn_cemlp_sig_workspace_bytes(int n, const csmpn_block_params* blocks, int n_blocks, int64_t rows) {
    Plan p;
    return make_plan(n, blocks, n_blocks, rows, p) ? 0 : p.bytes;
}

int csmpn_cemlp_forward_sig(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* x, int64_t rows,
                            float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows > 0 && (!x || !y)) return fail(CSMPN_ERR_INVALID, "sig: x or y is null");
    ArgsF a;
    memset(&a, 0, sizeof(a));
    a.nseg = 1;
    a.seg[0].a = x; a.seg[0].ch = blocks ? blocks[0].in_features : 0; a.seg[0].a_rows = rows;
    a.y = y;
    return run(metric, n, blocks, nullptr, n_blocks, MODE_PLAIN, false, rows, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_cemlp_backward_sig(const float* metric, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads, int n_blocks,
                             const float* x, const float* gy, int64_t rows, float* gx, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (rows > 0 && (!x || !gy)) return fail(CSMPN_ERR_INVALID, "sig: x or gy is null");
    ArgsF a;
    memset(&a, 0, sizeof(a));
    a.nseg = 1;
    a.seg[0].a = x; a.seg[0].ch = blocks ? blocks[0].in_features : 0; a.seg[0].a_rows = rows; a.seg[0].g = gx;
    a.gy = gy; a.gy_rows = rows;
    return run(metric, n, blocks, grads, n_blocks, MODE_PLAIN, true, rows, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_egcl_edge_forward_sig(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* h,
                                int32_t channels, const float* edge_attr, int32_t attr_channels, const int32_t* perm,
                                const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N, float* msg_rows,
                                void* workspace, size_t workspace_bytes, void* stream) {
    ArgsF a;
    int rc = edge_args(h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, N, a);
    if (rc) return rc;
    if (E > 0 && !msg_rows) return fail(CSMPN_ERR_INVALID, "sig: msg_rows is null");
    a.y = msg_rows;
    return run(metric, n, blocks, nullptr, n_blocks, MODE_EDGE, false, E, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_egcl_edge_backward_sig(const float* metric, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                                 int n_blocks, const float* h, int32_t channels, const float* edge_attr, int32_t attr_channels,
                                 const int32_t* perm, const int32_t* src_sorted, const int32_t* dst_sorted, int64_t E, int64_t N,
                                 const float* g_agg, float* g_edge_rows, float* g_edge_attr, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    ArgsF a;
    int rc = edge_args(h, channels, edge_attr, attr_channels, perm, src_sorted, dst_sorted, E, N, a);
    if (rc) return rc;
    if (E > 0 && (!g_agg || !g_edge_rows)) return fail(CSMPN_ERR_INVALID, "sig: g_agg or g_edge_rows is null");
    a.gy = g_agg; a.gy_idx = dst_sorted; a.gy_rows = N;
    a.seg[0].g = g_edge_rows;
    a.seg[1].g = g_edge_attr; a.seg[1].gi = perm;
    return run(metric, n, blocks, grads, n_blocks, MODE_EDGE, true, E, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_egcl_node_forward_sig(const float* metric, int n, const csmpn_block_params* blocks, int n_blocks, const float* h,
                                int32_t channels, const float* agg, int32_t agg_channels, const float* node_attr, int32_t attr_channels,
                                const int32_t* in_degree, int32_t mean_aggr, int32_t residual, int64_t N, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    ArgsF a;
    int rc = node_args(blocks, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr, residual, N, a);
    if (rc) return rc;
    if (N > 0 && !out) return fail(CSMPN_ERR_INVALID, "sig: out is null");
    a.y = out; a.resid = residual ? h : nullptr;
    return run(metric, n, blocks, nullptr, n_blocks, MODE_NODE, false, N, a, workspace, workspace_bytes, (hipStream_t)stream);
}

int csmpn_egcl_node_backward_sig(const float* metric, int n, const csmpn_block_params* blocks, const csmpn_block_grads* grads,
                                 int n_blocks, const float* h, int32_t channels, const float* agg, int32_t agg_channels,
                                 const float* node_attr, int32_t attr_channels, const int32_t* in_degree, int32_t mean_aggr,
                                 int32_t residual, int64_t N, const float* g_out, float* gh, float* g_agg, float* g_node_attr,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    ArgsF a;
    int rc = node_args(blocks, n_blocks, h, channels, agg, agg_channels, node_attr, attr_channels, in_degree, mean_aggr, residual, N, a);
    if (rc) return rc;
    if (N > 0 && (!g_out || !gh || !g_agg)) return fail(CSMPN_ERR_INVALID, "sig: g_out, gh or g_agg is null");
    a.gy = g_out; a.gy_rows = N; a.resid_bwd = residual ? 1 : 0;
    a.seg[0].g = gh; a.seg[1].g = g_agg; a.seg[2].g = g_node_attr;
    return run(metric, n, blocks, grads, n_blocks, MODE_NODE, true, N, a, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
