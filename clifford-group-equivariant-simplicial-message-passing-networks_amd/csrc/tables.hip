// Per-batch index tables of the embedding stage on the device (C-ABI: csmpn_simplex_tables, include/csmpn_hip.h):
// what SimplicialBatch.plan() builds on the host with nonzero / advanced indexing / bincount - the ascending rows of every
// simplex dimension, their vertices in all (d+1)! orders as batch rows, the graph of every vertex, the vertex count of
// every graph and the int32 copy of the types - rebuilt in place for a batch of new topology and the same row counts,
// without an allocation or a host round trip, so that a captured training step can be replayed on it.
//
// Stable compaction by type as a two-level scan:
//   count    every workgroup of 256 rows counts its rows of each type                      -> counts[block][4]
//   offsets  ONE workgroup scans the counts block by block (hipCUB BlockScan, 256 blocks per pass) -> first position of
//            every (block, type); compares the totals with the expected counts             -> status word
//   scatter  every row finds its rank among the rows of its type in its workgroup (wave ballots + the wave totals in LDS),
//            adds the workgroup's offset and writes its entries - only at positions below the expected count
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "../../include/csmpn_hip.h"
#include "capi_common.hpp"

namespace {

constexpr int kBlock = 256;      // rows per workgroup (4 waves of 64)
constexpr int kWaves = kBlock / 64;
constexpr int kTypes = 4;        // dimensions 0..3
constexpr int kOrders = 1 + 2 + 6 + 24;

struct Orders {                  // the vertex orders of every dimension, itertools.permutations order (lexicographic)
    unsigned char p[kOrders][4];
};
struct Expected {
    long long n[kTypes];
};
struct Outputs {
    int64_t* rows[kTypes];
    int64_t* verts[kTypes];
    int32_t* verts_i32[kTypes];
};

__device__ __forceinline__ int order_base(int d) { return d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 3 : 9; }
__device__ __forceinline__ int order_count(int d) { return d == 0 ? 1 : d == 1 ? 2 : d == 2 ? 6 : 24; }

// a[i] of a four-entry private array without a dynamic index (which would put the array into scratch memory)
template <class T>
__device__ __forceinline__ T pick4(const T* a, int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }

// rank of this lane among the lanes of its wave that hold type d, for d = 0..max_dim, and the wave's totals
__device__ __forceinline__ void wave_ranks(int type, int max_dim, int lane, int* rank, int* total) {
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int d = 0; d < kTypes; ++d) {
        const unsigned long long m = d <= max_dim ? __ballot(type == d) : 0ull;
        rank[d] = __popcll(m & below);
        total[d] = __popcll(m);
    }
}

__device__ __forceinline__ int row_type(const int64_t* node_types, long r, long S, int max_dim) {
    if (r >= S) return -1;
    const int64_t t = node_types[r];
    return (t < 0 || t > max_dim) ? -1 : (int)t;
}

__global__ __launch_bounds__(kBlock) void tables_count_kernel(const int64_t* node_types, long S, int max_dim, int* counts) {
    __shared__ int wave_total[kWaves][kTypes];
    const long r = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank[kTypes], total[kTypes];
    wave_ranks(row_type(node_types, r, S, max_dim), max_dim, lane, rank, total);
    if (lane == 0)
        for (int d = 0; d < kTypes; ++d) wave_total[wave][d] = total[d];
    __syncthreads();
    if (threadIdx.x < kTypes) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += wave_total[w][threadIdx.x];
        counts[(long)blockIdx.x * kTypes + threadIdx.x] = s;
    }
}

// one workgroup: offsets[b][d] = sum of counts[b'][d] over b' < b; status |= 1 << d where the total differs from expected[d]
__global__ __launch_bounds__(kBlock) void tables_offsets_kernel(const int* counts, long n_blocks, int max_dim, Expected expected,
                                                                 int* offsets, unsigned* status) {
    using Scan = hipcub::BlockScan<int, kBlock>;
    __shared__ typename Scan::TempStorage temp;
    unsigned bad = 0;
    for (int d = 0; d <= max_dim; ++d) {
        long long carry = 0;
        for (long base = 0; base < n_blocks; base += kBlock) {
            const long b = base + threadIdx.x;
            const int c = b < n_blocks ? counts[b * kTypes + d] : 0;
            int excl, sum;
            Scan(temp).ExclusiveSum(c, excl, sum);
            __syncthreads();
            if (b < n_blocks) offsets[b * kTypes + d] = (int)(carry + excl);
            carry += sum;
        }
        if (carry != expected.n[d]) bad |= 1u << d;
    }
    if (threadIdx.x == 0 && bad && status) atomicOr(status, bad);
}

__global__ __launch_bounds__(kBlock) void tables_scatter_kernel(const int64_t* x_ind, int M, const int64_t* node_types,
                                                                 const int64_t* x_ind_batch, const int64_t* x_ind_ptr, long S,
                                                                 long B, int max_dim, Expected expected, Orders orders,
                                                                 const int* offsets, Outputs out, int64_t* graph_of_vertex,
                                                                 unsigned long long* vertices_per_graph, int32_t* types_i32,
                                                                 unsigned* status) {
    __shared__ int wave_total[kWaves][kTypes];
    const long r = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int type = row_type(node_types, r, S, max_dim);
    int rank[kTypes], total[kTypes];
    wave_ranks(type, max_dim, lane, rank, total);
    if (lane == 0)
        for (int d = 0; d < kTypes; ++d) wave_total[wave][d] = total[d];
    __syncthreads();
    if (r >= S) return;
    if (types_i32) types_i32[r] = (int32_t)node_types[r];
    unsigned bad = 0;
    if (type < 0) {
        bad = 16u;                                   // a type outside [0, max_dim]: the row is in no table
    } else {
        long pos = offsets[(long)blockIdx.x * kTypes + type] + pick4(rank, type);
        for (int w = 0; w < wave; ++w) pos += wave_total[w][type];
        if (pos < expected.n[type]) {                // a count above the expected one never writes past the buffers
            int64_t g = x_ind_batch[r];
            if (g < 0 || g >= B) { bad |= 32u; g = g < 0 ? 0 : B - 1; }
            const int64_t start = x_ind_ptr[g];
            out.rows[type][pos] = r;
            if (type == 0) {
                graph_of_vertex[pos] = g;
                atomicAdd(&vertices_per_graph[g], 1ull);
            }
            int64_t v[kTypes];
#pragma unroll
            for (int j = 0; j < kTypes; ++j) {
                int64_t x = j <= type ? x_ind[r * M + j] + start : 0;
                if (x < 0 || x >= S) { bad |= 32u; x = x < 0 ? 0 : S - 1; }
                v[j] = x;
            }
            const int n_orders = order_count(type), first = order_base(type), width = type + 1;
            int64_t* vt = out.verts[type] + pos * n_orders * width;
            int32_t* vi = out.verts_i32[type] ? out.verts_i32[type] + pos * n_orders * width : nullptr;
            for (int k = 0; k < n_orders; ++k)
                for (int j = 0; j < width; ++j) {
                    const int64_t x = pick4(v, orders.p[first + k][j]);
                    vt[k * width + j] = x;
                    if (vi) vi[k * width + j] = (int32_t)x;
                }
        }
    }
    if (bad && status) atomicOr(status, bad);
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline long blocks_for(int64_t S) { return (long)((S + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

size_t csmpn_simplex_tables_workspace_bytes(int64_t n_rows, int32_t max_dim) {
    if (n_rows <= 0 || n_rows >= (1ll << 31) || max_dim < 0 || max_dim >= kTypes) return 0;
    return 256 + 2 * align256(sizeof(int) * kTypes * (size_t)blocks_for(n_rows));
}

int csmpn_simplex_tables(const int64_t* x_ind, int32_t x_ind_cols, const int64_t* node_types, const int64_t* x_ind_batch,
                         const int64_t* x_ind_ptr, int64_t n_rows, int64_t n_graphs, int32_t max_dim,
                         const int64_t* n_expected_host, int64_t* const* rows_host, int64_t* const* verts_host,
                         int32_t* const* verts_i32_host, int64_t* graph_of_vertex, int64_t* vertices_per_graph,
                         int32_t* types_i32, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (max_dim < 0) return csmpn_fail(CSMPN_ERR_INVALID, "max_dim %d is negative", (int)max_dim);
    if (max_dim >= kTypes) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "simplex tables: max_dim %d > 3 (24 vertex orders)", (int)max_dim);
    if (n_rows <= 0 || n_rows >= (1ll << 31) || n_graphs <= 0 || n_graphs >= (1ll << 31))
        return csmpn_fail(CSMPN_ERR_INVALID, "bad sizes n_rows=%lld n_graphs=%lld", (long long)n_rows, (long long)n_graphs);
    if (x_ind_cols <= max_dim) return csmpn_fail(CSMPN_ERR_INVALID, "x_ind has %d columns, max_dim %d needs %d", (int)x_ind_cols, (int)max_dim, (int)max_dim + 1);
    if (!x_ind || !node_types || !x_ind_batch || !x_ind_ptr || !n_expected_host || !rows_host || !verts_host || !graph_of_vertex ||
        !vertices_per_graph)
        return csmpn_fail(CSMPN_ERR_INVALID, "null pointer");
    Expected expected{};
    Outputs out{};
    for (int d = 0; d <= max_dim; ++d) {
        expected.n[d] = n_expected_host[d];
        if (expected.n[d] < 0 || expected.n[d] > n_rows) return csmpn_fail(CSMPN_ERR_INVALID, "expected count %lld of dimension %d", (long long)expected.n[d], d);
        out.rows[d] = rows_host[d];
        out.verts[d] = verts_host[d];
        out.verts_i32[d] = verts_i32_host ? verts_i32_host[d] : nullptr;
        if (expected.n[d] > 0 && (!out.rows[d] || !out.verts[d])) return csmpn_fail(CSMPN_ERR_INVALID, "null table of dimension %d", d);
    }
    const size_t need = csmpn_simplex_tables_workspace_bytes(n_rows, max_dim);
    if (!workspace || workspace_bytes < need) return csmpn_fail(CSMPN_ERR_INVALID, "simplex tables workspace too small: %zu < %zu", workspace_bytes, need);
    Orders orders{};
    for (int d = 0, k = 0; d < kTypes; ++d) {
        unsigned char p[4] = {0, 1, 2, 3};
        do {
            for (int j = 0; j < 4; ++j) orders.p[k][j] = p[j];
            ++k;
        } while (std::next_permutation(p, p + d + 1));
    }
    const long n_blocks = blocks_for(n_rows);
    char* ws = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(workspace)));
    // the alignment may cost up to 255 of the 256 spare bytes
    int* counts = reinterpret_cast<int*>(ws);
    int* offsets = reinterpret_cast<int*>(ws + align256(sizeof(int) * kTypes * (size_t)n_blocks));
    hipError_t e = hipMemsetAsync(vertices_per_graph, 0, sizeof(int64_t) * (size_t)n_graphs, st);
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(tables_count_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, node_types, (long)n_rows, (int)max_dim, counts);
    hipLaunchKernelGGL(tables_offsets_kernel, dim3(1), dim3(kBlock), 0, st, (const int*)counts, n_blocks, (int)max_dim, expected,
                       offsets, (unsigned*)status);
    hipLaunchKernelGGL(tables_scatter_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, x_ind, (int)x_ind_cols, node_types,
                       x_ind_batch, x_ind_ptr, (long)n_rows, (long)n_graphs, (int)max_dim, expected, orders, (const int*)offsets, out,
                       graph_of_vertex, reinterpret_cast<unsigned long long*>(vertices_per_graph), types_i32, (unsigned*)status);
    e = hipGetLastError();
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "simplex tables kernels: %s", hipGetErrorString(e));
    return CSMPN_OK;
}

}  // extern "C"
