// Vietoris-Rips lift of a batch on the device at a fixed capacity (C-ABI: csmpn_rips_lift, include/csmpn_hip.h): the
// structure tensors that the host builds with rips_complex -> lift -> to_complex -> collate -> pad_batch
// (csmpn/data/complexes.py) - x_ind, node_types, batch / x_ind_batch, ptr / x_ind_ptr, edge_index, edge_types, the fillers
// behind the real part included - from the vertex positions, without an allocation, a host round trip or an atomic on an
// output: every position of every entry is computed, never claimed.
//
// csmpn_knn_lift is the same lift of the clique complex of the k-nearest-neighbour graph (knn_clique_complex): another
// kernel produces the neighbour masks, and the adjacencies have no 0_0 block over the non-edges (kVertexBlock = false).
//
// csmpn_hull_lift is the same lift of the convex-hull complex (hull_complex(method="exact")) with the hull's volume: its
// kernel finds the facets among the subsets of point_dim vertices and writes, beside the masks, a table T[a][b] of the w with
// {a, b, w} in a facet - the triangles and cofaces of an edge come from T, not from the masks (kFacetTable = true).
//
// csmpn_clique_lift is the thresholded clique lift of any graph G (clique_complex): G's masks come from a caller's edge list
// (lift_list_kernel: 64-bit atomic ORs into zeroed masks) or from lift_knn_kernel; lift_filter_kernel keeps the edges of G
// with s <= edge_th^2 and the triangles of G with Gram determinant <= 4 tri_th^2, brings back the pairs of every kept
// triangle, and writes the final masks and a 64-wide table T - three surviving edges need not bound a surviving triangle,
// so the scatter reads T as the hull's does (kFacetTable = true, kTableStride = 64, no vertex block).
//
// csmpn_cloud_lift is the Rips lift of graphs of up to 4096 vertices, with or without the vertex block: several mask words per
// vertex, one wave per vertex and kernels of its own - the section "the Rips lift of point clouds" below;
// csmpn_cloud_knn_lift is the kNN clique lift of the same graphs: two kernels of its own make the mask words, the rest of that
// section follows unchanged. Everything up to there is the four lifts of small graphs:
//
// A graph has at most 64 vertices, so ONE 64-bit neighbour mask per vertex (a wave ballot over the other vertices) carries
// it, and every index is a popcount of masks plus a scan: with upper[a] = mask[a] restricted to b > a,
//   index of the edge (a, b), a < b      = sum_{a' < a} popc(upper[a']) + popc(upper[a] & below(b))
//   triangles in front of the edge (a,b) = the scan over the edges of popc(upper[a] & upper[b])   (triangles (a, b, c), c ascending)
//   cofaces in front of the edge (a, b)  = the scan over the edges of popc(mask[a] & mask[b])     (the 1_1 block)
// Both scans are kept per vertex a (64 entries in LDS); the part inside a's row of edges is a wave scan over the lanes b.
//
//   count    one workgroup per graph: the masks -> workspace, the graph's numbers of 1- and 2-simplices
//            (lift_count_kernel: pairs within dis; lift_knn_kernel: the symmetrised k nearest neighbours;
//            lift_hull_kernel<N>: the pairs and triples inside a facet, and the volume)
//   offsets  ONE workgroup: the totals against the capacity -> fit flag, status word; where the batch fits, the scan of the
//            graphs' row and adjacency counts (256 graphs per pass) -> ptr / x_ind_ptr, counts, the offsets of every graph
//   scatter  one workgroup per graph + workgroups for the fillers; all of them return at once when the fit flag is clear,
//            so a batch that does not fit leaves every output as it was
//
// Order of a graph's real part (= lift + to_complex): rows = the V vertices, the close pairs (a < b) and the triples
// (a < b < c) with all pairs close, both lexicographic; adjacencies = seven blocks, see scatter_graph below.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "../../include/csmpn_hip.h"
#include "capi_common.hpp"

namespace {

using u64 = unsigned long long;

constexpr int kBlock = 256;      // 4 waves of 64
constexpr int kWaves = kBlock / 64;
constexpr int kMaxVerts = 64;    // one mask bit per vertex
constexpr int kMaxFillBlocks = 1024;

struct Capacity {
    long long rows[3];           // rows per dimension (rows[2] = 0 for max_dim = 1)
    long long edges;
};

struct Header {                  // first 256 bytes of the workspace, written by the offsets kernel
    int fit;                     // 1: the batch fits its capacity, the scatter kernel writes
    long long n[3];              // real rows per dimension
    long long adj;               // real adjacencies
    int bad_list;                // csmpn_clique_lift: zeroed on the stream, set by lift_list_kernel for an end it refuses
};

struct Outputs {
    int64_t* x_ind;
    int64_t* node_types;
    int64_t* batch;
    int64_t* x_ind_batch;
    int64_t* edge_index;         // [2, cap_edges]
    int64_t* edge_types;         // [cap_edges, 2] or nullptr
    int cols;                    // columns of x_ind
    long long cap_edges;
};

__device__ __forceinline__ u64 below(int b) { return (1ull << b) - 1ull; }                       // bits < b, b in 0..63
__device__ __forceinline__ u64 above(int a) { return a >= 63 ? 0ull : ~0ull << (a + 1); }         // bits > a
__device__ __forceinline__ int first_bit(u64 m) { return __ffsll((long long)m) - 1; }

// exclusive prefix sum of v over the 64 lanes of a wave (every lane calls it)
__device__ __forceinline__ int wave_scan(int v, int lane, int* total) {
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (total) *total = __shfl(x, 63, 64);
    return x - v;
}

__device__ __forceinline__ void put_row(const Outputs& o, long long row, int type, long long graph, int v0, int v1, int v2) {
    for (int j = 0; j < o.cols; ++j) o.x_ind[row * o.cols + j] = j == 0 ? v0 : j == 1 ? v1 : j == 2 ? v2 : 0;
    o.node_types[row] = type;
    o.batch[row] = graph;
    o.x_ind_batch[row] = graph;
}

__device__ __forceinline__ void put_adj(const Outputs& o, long long pos, long long src, long long dst, int ts, int tt) {
    o.edge_index[pos] = src;
    o.edge_index[o.cap_edges + pos] = dst;
    if (o.edge_types) {
        o.edge_types[2 * pos] = ts;
        o.edge_types[2 * pos + 1] = tt;
    }
}

// The end of both mask kernels, run by wave 0 once m[0 .. V) is complete in LDS: the masks -> workspace, the graph's numbers
// of 1-simplices (bits above the diagonal) and 2-simplices (common upper neighbours of the two ends of every edge).
__device__ __forceinline__ void count_tail(const u64* m, long g, int V, int max_dim, int lane, u64* masks, int* n1, int* n2) {
    int c1 = 0, c2 = 0;
    if (lane < V) {
        const u64 ma = m[lane], up = ma & above(lane);
        masks[g * V + lane] = ma;
        c1 = __popcll(up);
        if (max_dim >= 2)
            for (u64 r = up; r; r &= r - 1) {
                const int b = first_bit(r);
                c2 += __popcll(up & m[b] & above(b));
            }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c1 += __shfl_down(c1, d, 64);
        c2 += __shfl_down(c2, d, 64);
    }
    if (lane == 0) {
        n1[g] = c1;
        n2[g] = c2;
    }
}

// one workgroup per graph: mask[a] bit b = (a != b and |p_a - p_b|^2 <= dis^2, summed in double over k ascending)
__global__ __launch_bounds__(kBlock) void lift_count_kernel(const float* points, int P, int V, double dis2, int max_dim,
                                                             u64* masks, int* n1, int* n2) {
    __shared__ u64 m[kMaxVerts];
    const long g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* pg = points + g * V * (long)P;
    for (int a = wave; a < V; a += kWaves) {
        bool close = false;
        if (lane < V && lane != a) {
            double s = 0.0;
            for (int k = 0; k < P; ++k) {
                const double d = (double)pg[a * P + k] - (double)pg[lane * P + k];
                s = __dadd_rn(s, __dmul_rn(d, d));            // no contraction: the sum the host takes
            }
            close = s <= dis2;                                // false for a NaN
        }
        const u64 mk = __ballot(close);
        if (lane == 0) m[a] = mk;
    }
    __syncthreads();
    if (wave == 0) count_tail(m, g, V, max_dim, lane, masks, n1, n2);
}

// one workgroup per graph: mask[a] bit b = (b is one of the k nearest neighbours of a, or a one of b's). With s(a, b) the
// sum of lift_count_kernel (a NaN counts as +infinity), the rank of b for a is the number of c outside {a, b} with
// s(a, c) < s(a, b), or s(a, c) == s(a, b) and c < b; b is a neighbour of a iff that rank is below k. The wave of a holds
// the row s(a, .) one value per lane and reads it across the lanes: no LDS for the row, no scratch.
__global__ __launch_bounds__(kBlock) void lift_knn_kernel(const float* points, int P, int V, int k, int max_dim, u64* masks,
                                                           int* n1, int* n2) {
    __shared__ u64 dir[kMaxVerts], m[kMaxVerts];
    const long g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* pg = points + g * V * (long)P;
    for (int a = wave; a < V; a += kWaves) {
        const bool in = lane < V && lane != a;
        double s = __longlong_as_double(0x7ff0000000000000ll);
        if (in) {
            double t = 0.0;
            for (int j = 0; j < P; ++j) {
                const double d = (double)pg[a * P + j] - (double)pg[lane * P + j];
                t = __dadd_rn(t, __dmul_rn(d, d));            // no contraction: the sum the host takes
            }
            if (t == t) s = t;                                // a NaN stays +infinity
        }
        int rank = 0;
        for (int c = 0; c < V; ++c) {                         // c is wave-uniform
            const double sc = __shfl(s, c, 64);
            rank += c != a && c != lane && (sc < s || (sc == s && c < lane)) ? 1 : 0;
        }
        const u64 d = __ballot(in && rank < k);
        if (lane == 0) dir[a] = d;
    }
    __syncthreads();
    if (wave == 0) {                                          // the undirected graph: bit b of dir[a] | bit a of dir[b]
        u64 sym = 0ull;
        if (lane < V) {
            sym = dir[lane];
            for (int b = 0; b < V; ++b) sym |= ((dir[b] >> lane) & 1ull) << b;
        }
        m[lane] = sym;
    }
    __syncthreads();
    if (wave == 0) count_tail(m, g, V, max_dim, lane, masks, n1, n2);
}

// ------------------------------------------------------------------------------------------------ the convex-hull lift
//
// A graph has V <= 16 points in R^N, N = 2..5. A candidate is an N-subset F = (f_0 < ... < f_{N-1}); with the rows
// M_i = p_{f_{i+1}} - p_{f_0} (i = 0..N-2), its normal is nrm_j = (-1)^(N-1+j) det(M without column j), and
// side(F, q) = sum_j nrm_j (q_j - p_{f_0, j}). F is a facet iff side(F, q) > 0 for every vertex q outside F, or < 0 for
// every one (a zero or a NaN: no facet). Everything in double, every product, sum and difference rounded once; the order of
// operations below is the one csmpn.data.complexes.hull_facets states on the host:
//   det of one entry = the entry; det of k rows = the Laplace expansion along the first of them over the columns c_0 < c_1 < ..:
//     ((M[c_0] det_0 - M[c_1] det_1) + M[c_2] det_2) - ...   (left to right, each product rounded before it is added);
//   side = ((nrm_0 d_0 + nrm_1 d_1) + nrm_2 d_2) + ..., d_j = q_j - p_{f_0, j}.
// Volume = (sum over the facets of |side(F, p_0)|) / N!: a thread sums the candidates rank = tid, tid + 256, ... ascending
// (rank = the lexicographic index of F), a wave adds lane + 32, + 16, ... + 1 into lane 0, wave 0's sum takes those of waves
// 1, 2, 3 in that order.

constexpr int kHullMaxVerts = 16;                             // C(16, 5) = 4368 candidates; the T table is 16 x 16 masks

// Rounded once, never contracted into an fma. The unit is built with -ffp-contract=fast, under which the backend fuses any
// product into the sum that takes it, whatever a pragma or __dmul_rn says; so the product is an instruction of its own that
// the optimiser cannot look into (pure: equal products are still computed once), and with it no sum has a product to fuse.
__device__ __forceinline__ double mul_rn(double x, double y) {
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
__device__ __forceinline__ double add_rn(double x, double y) { return x + y; }
__device__ __forceinline__ double sub_rn(double x, double y) { return x - y; }

constexpr int low_bit(unsigned m) { return (m & 1u) ? 0 : 1 + low_bit(m >> 1); }
constexpr int bits_of(unsigned m) { return m ? 1 + bits_of(m & (m - 1)) : 0; }

template <int N, int Row, unsigned Cols>
__device__ __forceinline__ double minor_det(const double (&M)[N - 1][N]);

// the terms of the expansion along row Row that are still to come (the columns in Rest), K of them taken
template <int N, int Row, unsigned Cols, unsigned Rest, int K>
__device__ __forceinline__ double laplace(const double (&M)[N - 1][N], double acc) {
    if constexpr (Rest == 0u) {
        return acc;
    } else {
        constexpr int c = low_bit(Rest);
        const double term = mul_rn(M[Row][c], minor_det<N, Row + 1, (Cols & ~(1u << c))>(M));
        const double next = K == 0 ? term : (K & 1) ? sub_rn(acc, term) : add_rn(acc, term);
        return laplace<N, Row, Cols, (Rest & (Rest - 1u)), K + 1>(M, next);
    }
}

// determinant of the rows Row .. N-2 and the columns in Cols (as many as rows)
template <int N, int Row, unsigned Cols>
__device__ __forceinline__ double minor_det(const double (&M)[N - 1][N]) {
    static_assert(bits_of(Cols) == N - 1 - Row, "as many columns as rows");
    if constexpr (bits_of(Cols) == 1)
        return M[Row][low_bit(Cols)];
    else
        return laplace<N, Row, Cols, Cols, 0>(M, 0.0);
}

template <int N, int J>
__device__ __forceinline__ void normal_of(const double (&M)[N - 1][N], double (&nrm)[N]) {
    if constexpr (J < N) {
        const double d = minor_det<N, 0, (((1u << N) - 1u) & ~(1u << J))>(M);
        nrm[J] = ((N - 1 + J) & 1) ? -d : d;
        normal_of<N, J + 1>(M, nrm);
    }
}

template <int N>
__device__ __forceinline__ double side_of(const double (&nrm)[N], const double* q, const double* origin) {
    double s = mul_rn(nrm[0], sub_rn(q[0], origin[0]));
#pragma unroll
    for (int j = 1; j < N; ++j) s = add_rn(s, mul_rn(nrm[j], sub_rn(q[j], origin[j])));
    return s;
}

// C(m, K) for 0 <= m <= 16 (0 for m < K); every intermediate is an integer
template <int K>
__device__ __forceinline__ int choose(int m) {
    int r = 1;
#pragma unroll
    for (int t = 0; t < K; ++t) r = r * (m - t) / (t + 1);
    return r;
}

// f = the rank-th N-subset of 0 .. V-1 in lexicographic order, rank < C(V, N)
template <int N, int I>
__device__ __forceinline__ void unrank(int V, int r, int x, int (&f)[N]) {
    if constexpr (I < N) {
        for (; x < V - (N - I); ++x) {                        // at the bound x is the only choice left
            const int c = choose<N - 1 - I>(V - 1 - x);       // subsets whose I-th element is x
            if (r < c) break;
            r -= c;
        }
        f[I] = x;
        unrank<N, I + 1>(V, r, x + 1, f);
    }
}

// one workgroup per graph: the facets among the C(V, N) candidates -> mask[a] bit b = {a, b} lies in a facet, T[a][b] bit w =
// {a, b, w} lies in a facet (both ORed together in LDS: the result does not depend on the order), the counts n1 and n2 and
// the volume -> workspace. No output is touched: the scatter kernel copies the volume once the batch is known to fit.
template <int N>
__global__ __launch_bounds__(kBlock) void lift_hull_kernel(const float* points, int V, int n_cand, int max_dim, u64* masks, u64* tables,
                                                            int* n1, int* n2, float* vols) {
    __shared__ double p[kHullMaxVerts * N];
    __shared__ u64 m[kHullMaxVerts], T[kHullMaxVerts * kHullMaxVerts];
    __shared__ double part[kWaves];
    const long g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pg = points + g * V * (long)N;
    if (tid < V * N) p[tid] = (double)pg[tid];                // V N <= 80
    if (tid < kHullMaxVerts) m[tid] = 0ull;
    T[tid] = 0ull;                                            // kBlock == 16 x 16
    __syncthreads();
    double vol = 0.0;
    for (int rank = tid; rank < n_cand; rank += kBlock) {
        int f[N];
        unrank<N, 0>(V, rank, 0, f);
        const double* origin = p + f[0] * N;
        double M[N - 1][N], nrm[N];
        u64 fb = 1ull << f[0];
#pragma unroll
        for (int i = 1; i < N; ++i) {
            fb |= 1ull << f[i];
#pragma unroll
            for (int j = 0; j < N; ++j) M[i - 1][j] = sub_rn(p[f[i] * N + j], origin[j]);
        }
        normal_of<N, 0>(M, nrm);
        bool pos = true, neg = true;
        for (int q = 0; q < V; ++q) {
            if ((fb >> q) & 1ull) continue;
            const double s = side_of<N>(nrm, p + q * N, origin);
            pos = pos && s > 0.0;
            neg = neg && s < 0.0;
        }
        if (!(pos || neg)) continue;
        vol = add_rn(vol, fabs(side_of<N>(nrm, p, origin)));
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const u64 others = fb & ~(1ull << f[i]);
            atomicOr(&m[f[i]], others);
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (j != i) atomicOr(&T[f[i] * kHullMaxVerts + f[j]], others & ~(1ull << f[j]));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) vol = add_rn(vol, __shfl_down(vol, d, 64));
    if (lane == 0) part[wave] = vol;
    __syncthreads();
    if (wave != 0) return;
    int c1 = 0, c2 = 0;
    if (lane < V) {
        const u64 ma = m[lane], up = ma & above(lane);
        masks[g * V + lane] = ma;
        c1 = __popcll(up);
        if (max_dim >= 2)
            for (u64 r = up; r; r &= r - 1) {
                const int b = first_bit(r);
                c2 += __popcll(T[lane * kHullMaxVerts + b] & above(b));
            }
    }
    for (int i = lane; i < V * V; i += 64) tables[g * V * V + i] = T[(i / V) * kHullMaxVerts + i % V];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c1 += __shfl_down(c1, d, 64);
        c2 += __shfl_down(c2, d, 64);
    }
    if (lane == 0) {
        n1[g] = c1;
        n2[g] = c2;
        double fact = 1.0;
        for (int i = 2; i <= N; ++i) fact *= i;
        vols[g] = (float)(add_rn(add_rn(add_rn(part[0], part[1]), part[2]), part[3]) / fact);
    }
}

// -------------------------------------------------------------------------------------- the thresholded clique lift
//
// G is any graph on the V vertices of a graph of the batch, as masks gm[a] bit b. With s(a, b) the sum of lift_count_kernel
// and, for a < b < c, g(a, b, c) = uu vv - uv uv (u = p_b - p_a, v = p_c - p_a, uu / vv / uv summed over j ascending; a NaN s
// or g counts as +infinity), all in double, every product, sum and difference rounded once (mul_rn above):
//   E_keep = the edges of G with s <= edge_th^2;   T_keep = the triples whose pairs are edges of G with g <= 4 tri_th^2;
//   1-simplices = E_keep and the three pairs of every triple of T_keep;   2-simplices = T_keep.

constexpr int kCliqueStride = kMaxVerts;                      // the T table of a graph in LDS: 64 x 64 masks, 32 KB

// G from a caller's list [2, n_list] of global vertex ids (graph g holds g V .. g V + V - 1): both directions ORed into
// the zeroed masks - an OR does not depend on the order. (-1, -1) is padding, a self-loop is skipped; an end outside the
// batch or two ends in different graphs set *bad_list and write nothing.
__global__ __launch_bounds__(kBlock) void lift_list_kernel(const int64_t* list, long long n_list, long long n_verts, int V, u64* gmasks,
                                                            int* bad_list) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_list) return;
    const long long a = list[i], b = list[n_list + i];
    if (a == -1 && b == -1) return;
    if (a < 0 || a >= n_verts || b < 0 || b >= n_verts || a / V != b / V) {
        atomicOr(bad_list, 1);
        return;
    }
    if (a == b) return;
    atomicOr(&gmasks[a], 1ull << (int)(b % V));
    atomicOr(&gmasks[b], 1ull << (int)(a % V));
}

__device__ __forceinline__ double not_nan(double x) { return x == x ? x : __longlong_as_double(0x7ff0000000000000ll); }

// one workgroup per graph: G's masks -> the final masks, the table T[a][b] (bit c = {a, b, c} in T_keep; [V, V] per graph in
// the workspace) and the counts. G's masks and the final ones live side by side in LDS; the pairs a kept triangle brings back
// and the table entries are ORed there (the result does not depend on the order). A thread takes the pairs (a, b) of G,
// a < b, and walks their common neighbours c > b: every triple is tried once.
__global__ __launch_bounds__(kBlock) void lift_filter_kernel(const float* points, int P, int V, double edge_th2, double tri_th4,
                                                              int max_dim, const u64* gmasks, u64* masks, u64* tables, int* n1, int* n2) {
    __shared__ u64 gm[kMaxVerts], fm[kMaxVerts], T[kCliqueStride * kCliqueStride];
    const long g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pg = points + g * V * (long)P;
    if (tid < kMaxVerts) gm[tid] = tid < V ? gmasks[g * V + tid] : 0ull;        // neither source sets a bit at or above V
    for (int i = tid; i < kCliqueStride * kCliqueStride; i += kBlock) T[i] = 0ull;
    __syncthreads();
    for (int a = wave; a < V; a += kWaves) {                  // E_keep
        bool keep = false;
        if (lane < V && lane != a && ((gm[a] >> lane) & 1ull)) {
            double s = 0.0;
            for (int j = 0; j < P; ++j) {
                const double d = sub_rn((double)pg[a * P + j], (double)pg[lane * P + j]);
                s = add_rn(s, mul_rn(d, d));
            }
            keep = not_nan(s) <= edge_th2;
        }
        const u64 mk = __ballot(keep);
        if (lane == 0) fm[a] = mk;
    }
    __syncthreads();
    for (int i = tid; i < V * V; i += kBlock) {               // T_keep
        const int a = i / V, b = i % V;
        if (a >= b || !((gm[a] >> b) & 1ull)) continue;
        u64 kept = 0ull;
        for (u64 r = gm[a] & gm[b] & above(b); r; r &= r - 1) {
            const int c = first_bit(r);
            double uu = 0.0, vv = 0.0, uv = 0.0;
            for (int j = 0; j < P; ++j) {
                const double pa = (double)pg[a * P + j];
                const double u = sub_rn((double)pg[b * P + j], pa), v = sub_rn((double)pg[c * P + j], pa);
                uu = add_rn(uu, mul_rn(u, u));
                vv = add_rn(vv, mul_rn(v, v));
                uv = add_rn(uv, mul_rn(u, v));
            }
            const double gram = sub_rn(mul_rn(uu, vv), mul_rn(uv, uv));
            if (!(not_nan(gram) <= tri_th4)) continue;
            kept |= 1ull << c;
            atomicOr(&T[a * kCliqueStride + c], 1ull << b);
            atomicOr(&T[c * kCliqueStride + a], 1ull << b);
            atomicOr(&T[b * kCliqueStride + c], 1ull << a);
            atomicOr(&T[c * kCliqueStride + b], 1ull << a);
            atomicOr(&fm[c], (1ull << a) | (1ull << b));
        }
        if (!kept) continue;
        atomicOr(&T[a * kCliqueStride + b], kept);
        atomicOr(&T[b * kCliqueStride + a], kept);
        atomicOr(&fm[a], kept | (1ull << b));
        atomicOr(&fm[b], kept | (1ull << a));
    }
    __syncthreads();
    for (int i = tid; i < V * V; i += kBlock) tables[g * V * V + i] = T[(i / V) * kCliqueStride + i % V];
    if (wave != 0) return;
    int c1 = 0, c2 = 0;
    if (lane < V) {
        const u64 ma = fm[lane], up = ma & above(lane);
        masks[g * V + lane] = ma;
        c1 = __popcll(up);
        if (max_dim >= 2)
            for (u64 r = up; r; r &= r - 1) {
                const int b = first_bit(r);
                c2 += __popcll(T[lane * kCliqueStride + b] & above(b));
            }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c1 += __shfl_down(c1, d, 64);
        c2 += __shfl_down(c2, d, 64);
    }
    if (lane == 0) {
        n1[g] = c1;
        n2[g] = c2;
    }
}

// one workgroup: totals against the capacity; if the batch fits, the offsets of every graph and ptr / x_ind_ptr / counts.
// kVertexBlock:a graph's adjacencies hold the 0_0 block over the non-edges (Rips), V (V - 1) + 5 n1 + 12 n2 of them; without
// it (kNN cliques) 6 n1 + 12 n2. A template parameter, here and in the scatter kernel: the Rips instantiations are the
// kernels without the switch, and the kNN instantiation of the scatter carries neither the block-2 store nor its index
// arithmetic - no wave-uniform branch in the pair loop and no register for it.
// kListFlag (csmpn_clique_lift): a list that lift_list_kernel has refused (hdr->bad_list) makes the batch invalid - bit 5 of
// the status word alone, whatever the counts of the rest of the list are, and no output is written. The instantiations without
// it never read the field.
template <bool kVertexBlock, bool kListFlag = false>
__global__ __launch_bounds__(kBlock) void lift_offsets_kernel(const int* n1, const int* n2, long B, int V, int max_dim, Capacity cap,
                                                               Header* hdr, long long* row_off, long long* adj_off, int64_t* ptr,
                                                               int64_t* x_ind_ptr, int64_t* counts, unsigned* status) {
    using Scan = hipcub::BlockScan<long long, kBlock>;
    __shared__ typename Scan::TempStorage temp;
    if constexpr (kListFlag) {
        if (hdr->bad_list) {                                  // uniform
            if (threadIdx.x == 0) {
                hdr->fit = 0;
                if (status) atomicOr(status, 1u << 5);
            }
            return;
        }
    }
    const long long VV = kVertexBlock ? (long long)V * (V - 1) : 0ll;     // adjacencies of a graph = VV + per_edge n1 + 12 n2
    const long long per_edge = kVertexBlock ? 5 : 6;
    long long N1 = 0, N2 = 0;
    for (long base = 0; base < B; base += kBlock) {
        const long g = base + threadIdx.x;
        long long excl, sum;
        Scan(temp).ExclusiveSum(g < B ? (long long)n1[g] : 0ll, excl, sum);
        __syncthreads();
        N1 += sum;
        Scan(temp).ExclusiveSum(g < B ? (long long)n2[g] : 0ll, excl, sum);
        __syncthreads();
        N2 += sum;
    }
    const long long E = B * VV + per_edge * N1 + 12 * N2;
    unsigned bad = 0;
    if (N1 > cap.rows[1]) bad |= 1u << 1;
    if (max_dim >= 2 && N2 > cap.rows[2]) bad |= 1u << 2;
    if (E > cap.edges) bad |= 1u << 3;
    if (!bad && E < cap.edges && cap.rows[1] - N1 + (max_dim >= 2 ? cap.rows[2] - N2 : 0) == 0) bad |= 1u << 4;
    if (bad) {                                               // uniform: every thread holds the same totals
        if (threadIdx.x == 0) {
            hdr->fit = 0;
            if (status) atomicOr(status, bad);
        }
        return;
    }
    long long rows = 0, adjs = 0;
    for (long base = 0; base < B; base += kBlock) {
        const long g = base + threadIdx.x;
        const long long a1 = g < B ? n1[g] : 0, a2 = g < B ? n2[g] : 0;
        long long excl, sum;
        Scan(temp).ExclusiveSum(g < B ? V + a1 + a2 : 0ll, excl, sum);
        __syncthreads();
        if (g < B) {
            row_off[g] = rows + excl;
            ptr[g] = rows + excl;
            x_ind_ptr[g] = rows + excl;
        }
        rows += sum;
        Scan(temp).ExclusiveSum(g < B ? VV + per_edge * a1 + 12 * a2 : 0ll, excl, sum);
        __syncthreads();
        if (g < B) adj_off[g] = adjs + excl;
        adjs += sum;
    }
    if (threadIdx.x == 0) {
        ptr[B] = rows;
        x_ind_ptr[B] = rows;
        hdr->n[0] = B * V;
        hdr->n[1] = N1;
        hdr->n[2] = N2;
        hdr->adj = E;
        hdr->fit = 1;
        if (counts) {
            counts[0] = B * V;
            counts[1] = N1;
            if (max_dim >= 2) counts[2] = N2;
            counts[max_dim + 1] = E;
        }
    }
}

// The real part of graph g. Adjacency blocks, each at its closed-form offset behind adj_off[g] (rows offset by row_off[g]):
//   1  0_0  for s, for the neighbours u of s ascending: (u, s)                                              2 n1
//   2  0_0  for i, for j: (i, j) for every ordered pair i != j except the pairs i < j that are an edge      V (V - 1) - n1
//           (kVertexBlock only: without it block 3 follows block 1)
//   3  0_1  for every edge e = (a, b): (a, e), (b, e)                                                       2 n1
//   4  1_0  the flips of block 3                                                                            2 n1
//   5  1_1  for every edge s = (a, b), for the common neighbours w ascending: ({a, w}, s), ({b, w}, s)       6 n2
//   6  1_2  for every triangle t = (a, b, c): ((a, b), t), ((a, c), t), ((b, c), t)                         3 n2
//   7  2_1  the flips of block 6                                                                            3 n2
// A wave takes the vertices a = wave, wave + 4, ...; its lane b holds the pair (a, b).
// kFacetTable (the hull lift, V <= 16): a triple is a 2-simplex iff it lies in a facet, not iff its pairs are edges, so the
// triangles of the edge (a, b) are T[a][b] & above(b) and its cofaces T[a][b], T = `tables` [V, V] of graph g loaded into
// LDS, instead of the intersections of the neighbour masks. A template parameter for the reason kVertexBlock is one: the
// Rips and kNN instantiations carry neither the table nor a branch on it. kTableStride: the row length of T in LDS - 16 for
// the hull lift, 64 for the thresholded clique lift (32 KB, loaded by a loop); a template parameter again, so that the hull
// instantiation keeps its one-statement load and its index arithmetic.
template <bool kVertexBlock, bool kFacetTable, int kTableStride = kHullMaxVerts>
__device__ void scatter_graph(long g, int V, int max_dim, const u64* masks, const u64* tables, const int* n1s, const int* n2s,
                              const long long* row_off, const long long* adj_off, const Outputs& o) {
    __shared__ u64 m[kMaxVerts];
    const u64* T = nullptr;
    if constexpr (kFacetTable) {
        __shared__ u64 table_s[kTableStride * kTableStride];
        if constexpr (kTableStride == kHullMaxVerts) {
            if ((int)threadIdx.x < V * V) table_s[(threadIdx.x / V) * kHullMaxVerts + threadIdx.x % V] = tables[g * V * V + threadIdx.x];
        } else {
            for (int i = threadIdx.x; i < V * V; i += kBlock) table_s[(i / V) * kTableStride + i % V] = tables[g * V * V + i];
        }
        T = table_s;
    }
    __shared__ int deg_s[kMaxVerts], up_s[kMaxVerts], tri_s[kMaxVerts], cof_s[kMaxVerts];   // sums over the vertices in front
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kMaxVerts) m[tid] = tid < V ? masks[g * V + tid] : 0ull;
    __syncthreads();
    if (wave == 0) {
        const u64 ma = m[lane], up = ma & above(lane);
        int t = 0, c = 0;
        if (max_dim >= 2)
            for (u64 r = up; r; r &= r - 1) {
                const int b = first_bit(r);
                const u64 mb = m[b];
                const u64 cof = kFacetTable ? T[lane * kTableStride + b] : ma & mb;
                t += __popcll(kFacetTable ? cof & above(b) : up & mb & above(b));
                c += __popcll(cof);
            }
        deg_s[lane] = wave_scan(__popcll(ma), lane, nullptr);
        up_s[lane] = wave_scan(__popcll(up), lane, nullptr);
        tri_s[lane] = wave_scan(t, lane, nullptr);
        cof_s[lane] = wave_scan(c, lane, nullptr);
    }
    __syncthreads();
    const long long n1 = n1s[g], n2 = n2s[g], row0 = row_off[g], adj0 = adj_off[g];
    const long long VV = kVertexBlock ? (long long)V * (V - 1) : 0ll;
    const long long o1 = adj0, o2 = o1 + 2 * n1, o3 = kVertexBlock ? adj0 + VV + n1 : o2, o4 = o3 + 2 * n1, o5 = o4 + 2 * n1, o6 = o5 + 6 * n2,
                    o7 = o6 + 3 * n2;
    const long long e0 = row0 + V, t0 = e0 + n1;              // first edge row, first triangle row
    if (tid < V) put_row(o, row0 + tid, 0, g, tid, 0, 0);
    for (int a = wave; a < V; a += kWaves) {
        const u64 ma = m[a], up = ma & above(a), mb = m[lane];
        if ((ma >> lane) & 1ull) put_adj(o, o1 + deg_s[a] + __popcll(ma & below(lane)), row0 + lane, row0 + a, 0, 0);
        if (kVertexBlock && lane < V && lane != a && !(lane > a && ((ma >> lane) & 1ull)))
            put_adj(o, o2 + (long long)a * (V - 1) - up_s[a] + lane - (lane > a ? 1 : 0) - __popcll(up & below(lane)), row0 + a,
                    row0 + lane, 0, 0);
        const bool edge = (up >> lane) & 1ull;                // the pair (a, lane), a < lane, is an edge
        const u64 both = kFacetTable ? (edge ? T[a * kTableStride + lane] : 0ull) : ma & mb;
        const u64 tri = edge && max_dim >= 2 ? (kFacetTable ? both : up & mb) & above(lane) : 0ull;   // its triangles (a, lane, c)
        const u64 cof = edge && max_dim >= 2 ? both : 0ull;                      // its cofaces {a, lane, w}
        const long long tb = tri_s[a] + wave_scan(__popcll(tri), lane, nullptr);
        const long long cb = cof_s[a] + wave_scan(__popcll(cof), lane, nullptr);
        if (!edge) continue;
        const long long e = up_s[a] + __popcll(up & below(lane)), erow = e0 + e;
        put_row(o, erow, 1, g, a, lane, 0);
        put_adj(o, o3 + 2 * e, row0 + a, erow, 0, 1);
        put_adj(o, o3 + 2 * e + 1, row0 + lane, erow, 0, 1);
        put_adj(o, o4 + 2 * e, erow, row0 + a, 1, 0);
        put_adj(o, o4 + 2 * e + 1, erow, row0 + lane, 1, 0);
        const u64 upb = mb & above(lane);
        int k = 0;
        for (u64 r = tri; r; r &= r - 1, ++k) {
            const int c = first_bit(r);
            const long long t = tb + k, trow = t0 + t;
            const long long eac = e0 + up_s[a] + __popcll(up & below(c)), ebc = e0 + up_s[lane] + __popcll(upb & below(c));
            put_row(o, trow, 2, g, a, lane, c);
            put_adj(o, o6 + 3 * t, erow, trow, 1, 2);
            put_adj(o, o6 + 3 * t + 1, eac, trow, 1, 2);
            put_adj(o, o6 + 3 * t + 2, ebc, trow, 1, 2);
            put_adj(o, o7 + 3 * t, trow, erow, 2, 1);
            put_adj(o, o7 + 3 * t + 1, trow, eac, 2, 1);
            put_adj(o, o7 + 3 * t + 2, trow, ebc, 2, 1);
        }
        k = 0;
        for (u64 r = cof; r; r &= r - 1, ++k) {
            const int w = first_bit(r);
            // in the sorted triple of {a, lane, w} the edge {a, w} always comes before {lane, w}
            const int la = a < w ? a : w, ha = a < w ? w : a, lb = lane < w ? lane : w, hb = lane < w ? w : lane;
            const long long eaw = e0 + up_s[la] + __popcll(m[la] & above(la) & below(ha));
            const long long ebw = e0 + up_s[lb] + __popcll(m[lb] & above(lb) & below(hb));
            put_adj(o, o5 + 2 * (cb + k), eaw, erow, 1, 1);
            put_adj(o, o5 + 2 * (cb + k) + 1, ebw, erow, 1, 1);
        }
    }
}

// The fillers behind the real part (pad_batch): filler d-simplices, dimension by dimension, x_ind = 0..d, graph B - 1;
// filler adjacencies = self-loops on the filler rows, round-robin, edge_types (d, d).
__device__ void scatter_fillers(long block, long n_blocks, long B, int max_dim, Capacity cap, const Header* hdr, const Outputs& o) {
    const long long S = hdr->n[0] + hdr->n[1] + hdr->n[2], E = hdr->adj;
    const long long fill1 = cap.rows[1] - hdr->n[1], fill2 = max_dim >= 2 ? cap.rows[2] - hdr->n[2] : 0;
    const long long n_fill = fill1 + fill2, e_fill = cap.edges - E;
    const long long first = block * kBlock + threadIdx.x, stride = n_blocks * kBlock;
    for (long long i = first; i < n_fill; i += stride) {
        const int d = i < fill1 ? 1 : 2;
        put_row(o, S + i, d, B - 1, 0, 1, d == 2 ? 2 : 0);
    }
    if (n_fill <= 0) return;                                  // (the offsets kernel has refused e_fill > 0 without a filler row)
    for (long long j = first; j < e_fill; j += stride) {
        const long long i = j % n_fill;
        const int d = i < fill1 ? 1 : 2;
        put_adj(o, E + j, S + i, S + i, d, d);
    }
}

template <bool kVertexBlock>
__global__ __launch_bounds__(kBlock) void lift_scatter_kernel(long B, int V, int max_dim, Capacity cap, const Header* hdr,
                                                               const u64* masks, const int* n1, const int* n2, const long long* row_off,
                                                               const long long* adj_off, Outputs o) {
    if (!hdr->fit) return;
    if ((long)blockIdx.x < B)
        scatter_graph<kVertexBlock, false>((long)blockIdx.x, V, max_dim, masks, nullptr, n1, n2, row_off, adj_off, o);
    else
        scatter_fillers((long)blockIdx.x - B, (long)gridDim.x - B, B, max_dim, cap, hdr, o);
}

// the scatter of the hull lift: the vertex block, the facet table, and the volumes from the workspace to their output
__global__ __launch_bounds__(kBlock) void lift_hull_scatter_kernel(long B, int V, int max_dim, Capacity cap, const Header* hdr,
                                                                    const u64* masks, const u64* tables, const int* n1, const int* n2,
                                                                    const long long* row_off, const long long* adj_off,
                                                                    const float* vols, float* volume, Outputs o) {
    if (!hdr->fit) return;
    if ((long)blockIdx.x < B) {
        if (volume && threadIdx.x == 0) volume[blockIdx.x] = vols[blockIdx.x];
        scatter_graph<true, true>((long)blockIdx.x, V, max_dim, masks, tables, n1, n2, row_off, adj_off, o);
    } else {
        scatter_fillers((long)blockIdx.x - B, (long)gridDim.x - B, B, max_dim, cap, hdr, o);
    }
}

// the scatter of the thresholded clique lift: no vertex block, the 64-wide table of lift_filter_kernel
__global__ __launch_bounds__(kBlock) void lift_clique_scatter_kernel(long B, int V, int max_dim, Capacity cap, const Header* hdr,
                                                                      const u64* masks, const u64* tables, const int* n1, const int* n2,
                                                                      const long long* row_off, const long long* adj_off, Outputs o) {
    if (!hdr->fit) return;
    if ((long)blockIdx.x < B)
        scatter_graph<false, true, kCliqueStride>((long)blockIdx.x, V, max_dim, masks, tables, n1, n2, row_off, adj_off, o);
    else
        scatter_fillers((long)blockIdx.x - B, (long)gridDim.x - B, B, max_dim, cap, hdr, o);
}

// ------------------------------------------------------------------------------- the Rips lift of point clouds, V > 64
//
// csmpn_cloud_lift: the Rips rule of lift_count_kernel on graphs of up to kCloudMaxVerts vertices. A vertex has
// W = ceil(V / 64) mask words, masks[g][a][w] bit i = vertex 64 w + i is close to a (bits at or above V are never set), and
// the closed forms above hold with sums over the words. One workgroup per graph no longer fills the chip (B = 1 is the case
// the entry is for) and a graph's masks no longer fit LDS, so the grid is (graph, tile of kWaves vertices), one wave per
// vertex, and the per-vertex prefix sums are read from the workspace:
//   mask     a wave per vertex a: for every word, lane = the vertex inside it, a ballot = the word; beside it
//            rank[g][a][w] = the upper neighbours of a in the words in front of w (the index of the edge (a, c) is then
//            up_s[a] + rank[a][c / 64] + one popcount), and the vertex's degree deg[a] and upper degree up[a]
//   count    (max_dim = 2) a wave per vertex a, lane = a WORD: for every upper neighbour b ascending the lanes load the row of
//            b and add popc(up_a & m_b & above b) and popc(m_a & m_b) -> tri[a], cof[a] (triangles / cofaces of a's edges)
//   scan     a workgroup per graph: deg / up / tri / cof -> their exclusive prefixes over the vertices, in place; n1, n2
//   offsets  lift_offsets_kernel, unchanged
//   scatter  a wave per vertex a + the filler workgroups: the rows and adjacencies of scatter_graph at the same positions;
//            the prefix of tri / cof inside a's edges is a wave scan per word plus a carry over the words
// No atomic, no LDS array sized by V. A graph's triangles can pass 2^31 long before the capacity is read (C(4096, 3)): the
// scan sums in 64 bits and n2 saturates at INT_MAX, which no capacity admits, so such a batch is refused (bit 2) and the
// truncated prefixes are never read.

constexpr int kCloudMaxVerts = 4096;                          // W <= 64: a lane per word in the count kernel

constexpr int cloud_words(int V) { return (V + 63) / 64; }

// the bits of word `word` that belong to vertices above v
__device__ __forceinline__ u64 above_in(int word, int v) {
    const int wv = v >> 6;
    return word < wv ? 0ull : word == wv ? above(v & 63) : ~0ull;
}

// one wave per vertex a of graph g = blockIdx.x / tiles: its mask words, ranks, degree and upper degree -> workspace
__global__ __launch_bounds__(kBlock) void cloud_mask_kernel(const float* points, int P, int V, int W, int tiles, double dis2, u64* masks,
                                                             int* rank, int* deg, int* up) {
    const long g = blockIdx.x / (unsigned)tiles;
    const int lane = threadIdx.x & 63, a = (int)(blockIdx.x % (unsigned)tiles) * kWaves + (threadIdx.x >> 6);
    if (a >= V) return;                                       // the whole wave
    const float* pg = points + g * V * (long)P;
    const long long va = (long long)g * V + a;
    u64* ma = masks + va * W;
    int* ra = rank + va * W;
    int nd = 0, nu = 0;
    for (int w = 0; w < W; ++w) {
        const int b = w * 64 + lane;
        bool close = false;
        if (b < V && b != a) {                                // a lane past V reads no point and sets no bit
            double s = 0.0;
            for (int k = 0; k < P; ++k) {
                const double d = sub_rn((double)pg[a * P + k], (double)pg[b * P + k]);
                s = add_rn(s, mul_rn(d, d));                  // no contraction: the sum the host takes
            }
            close = s <= dis2;                                // false for a NaN
        }
        const u64 word = __ballot(close);
        if (lane == 0) {
            ma[w] = word;
            ra[w] = nu;
        }
        nd += __popcll(word);
        nu += __popcll(word & above_in(w, a));
    }
    if (lane == 0) {
        deg[va] = nd;
        up[va] = nu;
    }
}

// csmpn_cloud_knn_lift: the kNN rule of lift_knn_kernel on the same graphs. Two kernels stand where cloud_mask_kernel
// stands, both a wave per vertex, and the count, scan, offsets and scatter kernels follow unchanged (no vertex block):
//   select   dir[g][a][w] bit i = vertex 64 w + i is one of the k nearest neighbours of a. Counting ranks costs V^2 comparisons
//            per vertex; instead the wave finds T, the k-th smallest s(a, .), by bisection on its bits - a non-negative double
//            and +infinity order as the 64-bit integers their bits spell - two bits in a pass: with c_j = T | j << bit
//            (j = 1, 2, 3) and n_j = #{b : s(a, b) < c_j} (a ballot and a popcount per word), T becomes the largest c_j with
//            n_j < k. 32 passes, bit = 62, 60 .. 0, bit 63 never taken: both candidates that carry it lie above every s and
//            count V - 1 > k. Behind them #{s < T} < k <= #{s <= T}, so T is the k-th smallest, and a last pass takes every b
//            with s < T and, of the b with s == T, the first k - #{s < T} in ascending index (a popcount prefix carried over
//            the words): rank(a, b) < k exactly. A candidate with n_j == k ends the bisection at once - the k sums below it
//            are the neighbours and no tie is left to take - which, where the k-th and (k + 1)-th sums differ, happens at
//            the first bit that parts them: 8 passes or so instead of 32. The row s(a, .) stays in registers, one 64-bit
//            value per word and lane: the kernel is a template over the row's length (1, 2, 4, 16 or 64 words, the
//            smallest that holds W) with every loop over it unrolled - no LDS, no index taken at run time, no scratch; the
//            passes are compares, ballots and popcounts alone. k >= V - 1: every other vertex, no pass.
//   mask     m[a] = dir[a] | (bit a of dir[b], every b): for word w, lane i reads the one word of dir[64 w + i] that holds
//            bit a, and a ballot gives the word; beside it the rank, deg and up of cloud_mask_kernel.

// one wave per vertex a of graph g = blockIdx.x / tiles: the words of its k nearest neighbours -> dir. kWords >= W is the
// length of the row in registers: every loop over it is unrolled, so no index is taken at run time (no scratch).
template <int kWords>
__global__ __launch_bounds__(kBlock) void cloud_knn_select_kernel(const float* points, int P, int V, int W, int tiles, int k, u64* dir) {
    const long g = blockIdx.x / (unsigned)tiles;
    const int lane = threadIdx.x & 63, a = (int)(blockIdx.x % (unsigned)tiles) * kWaves + (threadIdx.x >> 6);
    if (a >= V) return;                                       // the whole wave
    const float* pg = points + g * V * (long)P;
    u64* da = dir + ((long long)g * V + a) * W;
    if (k >= V - 1) {                                         // every other vertex
        for (int w = lane; w < W; w += 64) {
            const int left = V - w * 64;                      // >= 1
            u64 word = left >= 64 ? ~0ull : below(left);
            if (w == (a >> 6)) word &= ~(1ull << (a & 63));
            da[w] = word;
        }
        return;
    }
    // the row: s[w] = s(a, 64 w + lane) of lift_knn_kernel as the integer its bits spell, a NaN as +infinity; a lane at or
    // past V, and the lane of a itself, reads no point and holds ~0, which lies above every candidate and equals no T: it
    // never counts and never sets a bit. j is the outer loop, so the loads of one coordinate are all in flight together.
    double acc[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) acc[w] = 0.0;
    for (int j = 0; j < P; ++j) {
        const double pa = (double)pg[a * P + j];
#pragma unroll
        for (int w = 0; w < kWords; ++w) {
            const int b = w * 64 + lane;
            if (b < V) {
                const double d = sub_rn(pa, (double)pg[b * P + j]);
                acc[w] = add_rn(acc[w], mul_rn(d, d));        // no contraction: the sum the host takes
            }
        }
    }
    u64 s[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
        const int b = w * 64 + lane;
        s[w] = b >= V || b == a ? ~0ull : acc[w] == acc[w] ? (u64)__double_as_longlong(acc[w]) : 0x7ff0000000000000ull;
    }
    u64 T = 0ull;
    int less = 0;                                             // #{b : s(a, b) < T}, below k until a candidate counts k
    for (int bit = 62; bit >= 0; bit -= 2) {
        const u64 c1 = T | 1ull << bit, c2 = T | 2ull << bit, c3 = T | 3ull << bit;
        int n1 = 0, n2 = 0, n3 = 0;
#pragma unroll
        for (int w = 0; w < kWords; ++w) {
            n1 += __popcll(__ballot(s[w] < c1));
            n2 += __popcll(__ballot(s[w] < c2));
            n3 += __popcll(__ballot(s[w] < c3));
        }
        if (n1 == k || n2 == k || n3 == k) {                  // exactly k sums lie below this candidate: they are the neighbours
            T = n1 == k ? c1 : n2 == k ? c2 : c3;
            less = k;
            break;
        }
        if (n3 < k) {
            T = c3;
            less = n3;
        } else if (n2 < k) {
            T = c2;
            less = n2;
        } else if (n1 < k) {
            T = c1;
            less = n1;
        }
    }
    int ties = k - less;                                      // the b with s == T still to take, smallest index first
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
        const u64 eq = __ballot(s[w] == T);
        const u64 word = __ballot(s[w] < T || (s[w] == T && __popcll(eq & below(lane)) < ties));
        ties -= min(ties, __popcll(eq));
        if (lane == 0 && w < W) da[w] = word;
    }
}

// one wave per vertex a: the words of the undirected graph, and what cloud_mask_kernel writes beside them -> workspace
__global__ __launch_bounds__(kBlock) void cloud_knn_mask_kernel(int V, int W, int tiles, const u64* dir, u64* masks, int* rank, int* deg,
                                                                 int* up) {
    const long g = blockIdx.x / (unsigned)tiles;
    const int lane = threadIdx.x & 63, a = (int)(blockIdx.x % (unsigned)tiles) * kWaves + (threadIdx.x >> 6);
    if (a >= V) return;                                       // the whole wave
    const long long va = (long long)g * V + a;
    const u64* dg = dir + (long long)g * V * W;
    u64* ma = masks + va * W;
    int* ra = rank + va * W;
    int nd = 0, nu = 0;
    for (int w = 0; w < W; ++w) {
        const int b = w * 64 + lane;
        const bool named = b < V && ((dg[(long long)b * W + (a >> 6)] >> (a & 63)) & 1ull);   // b names a; dir[a] never holds bit a
        const u64 word = dg[(long long)a * W + w] | __ballot(named);
        if (lane == 0) {
            ma[w] = word;
            ra[w] = nu;
        }
        nd += __popcll(word);
        nu += __popcll(word & above_in(w, a));
    }
    if (lane == 0) {
        deg[va] = nd;
        up[va] = nu;
    }
}

// one wave per vertex a; lane = word: tri[a] = the triangles (a, b, c), a < b < c, cof[a] = the cofaces of the edges (a, b), a < b
__global__ __launch_bounds__(kBlock) void cloud_count_kernel(int V, int W, int tiles, const u64* masks, int* tri, int* cof) {
    const long g = blockIdx.x / (unsigned)tiles;
    const int lane = threadIdx.x & 63, a = (int)(blockIdx.x % (unsigned)tiles) * kWaves + (threadIdx.x >> 6);
    if (a >= V) return;
    const u64* mg = masks + (long long)g * V * W;
    const u64 ma = lane < W ? mg[(long long)a * W + lane] : 0ull;
    const u64 ua = ma & above_in(lane, a);
    int t = 0, c = 0;
    for (int w = a >> 6; w < W; ++w)
        for (u64 r = __shfl(ua, w, 64); r; r &= r - 1) {      // wave-uniform: the upper neighbours b of a, ascending
            const int b = w * 64 + first_bit(r);
            const u64 mb = lane < W ? mg[(long long)b * W + lane] : 0ull;
            t += __popcll(ua & mb & above_in(lane, b));
            c += __popcll(ma & mb);
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        t += __shfl_down(t, d, 64);
        c += __shfl_down(c, d, 64);
    }
    if (lane == 0) {
        tri[(long long)g * V + a] = t;
        cof[(long long)g * V + a] = c;
    }
}

using CloudScan = hipcub::BlockScan<long long, kBlock>;

// x[0 .. V) -> its exclusive prefix sums, in place (kBlock vertices per pass); returns the total
__device__ __forceinline__ long long cloud_scan_in_place(int* x, int V, typename CloudScan::TempStorage& temp) {
    long long carry = 0;
    for (int v0 = 0; v0 < V; v0 += kBlock) {
        const int v = v0 + threadIdx.x;
        long long excl, sum;
        CloudScan(temp).ExclusiveSum(v < V ? (long long)x[v] : 0ll, excl, sum);
        __syncthreads();
        if (v < V) x[v] = (int)(carry + excl);
        carry += sum;
    }
    return carry;
}

// one workgroup per graph
__global__ __launch_bounds__(kBlock) void cloud_scan_kernel(int V, int max_dim, int* deg, int* up, int* tri, int* cof, int* n1, int* n2) {
    __shared__ typename CloudScan::TempStorage temp;
    const long long v0 = (long long)blockIdx.x * V;
    cloud_scan_in_place(deg + v0, V, temp);
    const long long e = cloud_scan_in_place(up + v0, V, temp);    // <= V (V - 1) / 2
    long long t = 0;
    if (max_dim >= 2) {
        t = cloud_scan_in_place(tri + v0, V, temp);
        cloud_scan_in_place(cof + v0, V, temp);
    }
    if (threadIdx.x == 0) {
        n1[blockIdx.x] = (int)e;
        n2[blockIdx.x] = t > 0x7fffffffll ? 0x7fffffff : (int)t;
    }
}

// index, among its graph's edges, of the edge (lo, hi), lo < hi; mg / rg / up_s are the graph's masks, ranks and scanned `up`
__device__ __forceinline__ long long cloud_edge(const u64* mg, const int* rg, const int* up_s, int W, int lo, int hi) {
    const int w = hi >> 6;
    const long long i = (long long)lo * W + w;
    return (long long)up_s[lo] + rg[i] + __popcll(mg[i] & above_in(w, lo) & below(hi & 63));
}

// The part of vertex a in the real part of graph g, run by one wave: scatter_graph's rows and adjacencies at scatter_graph's
// positions. The wave walks a's words; in word w its lane holds the pair (a, b = 64 w + lane).
template <bool kVertexBlock>
__device__ void cloud_scatter_vertex(long g, int a, int lane, int V, int W, int max_dim, const u64* masks, const int* rank, const int* deg,
                                     const int* up, const int* tri, const int* cof, const int* n1s, const int* n2s,
                                     const long long* row_off, const long long* adj_off, const Outputs& o) {
    const long long v0 = (long long)g * V;
    const u64* mg = masks + v0 * W;
    const int* rg = rank + v0 * W;
    const int *deg_s = deg + v0, *up_s = up + v0;
    const long long n1 = n1s[g], n2 = n2s[g], row0 = row_off[g], adj0 = adj_off[g];
    const long long VV = kVertexBlock ? (long long)V * (V - 1) : 0ll;
    const long long o1 = adj0, o2 = o1 + 2 * n1, o3 = kVertexBlock ? adj0 + VV + n1 : o2, o4 = o3 + 2 * n1, o5 = o4 + 2 * n1, o6 = o5 + 6 * n2,
                    o7 = o6 + 3 * n2;
    const long long e0 = row0 + V, t0 = e0 + n1;              // first edge row, first triangle row
    const u64* ma = mg + (long long)a * W;
    if (lane == 0) put_row(o, row0 + a, 0, g, a, 0, 0);
    // in front of word w: the block-1 entries of a and of the vertices before it, the edges, the triangles and the cofaces
    long long nd = deg_s[a], nu = up_s[a], tb = max_dim >= 2 ? tri[v0 + a] : 0, cb = max_dim >= 2 ? cof[v0 + a] : 0;
    for (int w = 0; w < W; ++w) {
        const int b = w * 64 + lane;
        const u64 maw = ma[w], uaw = maw & above_in(w, a);
        if ((maw >> lane) & 1ull) put_adj(o, o1 + nd + __popcll(maw & below(lane)), row0 + b, row0 + a, 0, 0);
        if (kVertexBlock && b < V && b != a && !((uaw >> lane) & 1ull))
            put_adj(o, o2 + (long long)a * (V - 1) + b - (b > a ? 1 : 0) - nu - __popcll(uaw & below(lane)), row0 + a, row0 + b, 0, 0);
        nd += __popcll(maw);
        if (uaw == 0ull) continue;                            // the whole wave: no edge (a, b) in this word
        const bool edge = (uaw >> lane) & 1ull;               // the pair (a, b), a < b, is an edge
        const u64* mb = mg + (long long)b * W;                // read by the edge lanes alone (b < V there)
        int nt = 0, nc = 0;                                   // its triangles (a, b, c) and its cofaces {a, b, x}
        if (edge && max_dim >= 2)
            for (int x = 0; x < W; ++x) {
                const u64 both = ma[x] & mb[x];
                nc += __popcll(both);
                nt += __popcll(both & above_in(x, b));
            }
        int sum_t, sum_c;
        long long t = tb + wave_scan(nt, lane, &sum_t), k = cb + wave_scan(nc, lane, &sum_c);
        tb += sum_t;
        cb += sum_c;
        const long long e = nu + __popcll(uaw & below(lane)), erow = e0 + e;
        nu += __popcll(uaw);
        if (!edge) continue;
        put_row(o, erow, 1, g, a, b, 0);
        put_adj(o, o3 + 2 * e, row0 + a, erow, 0, 1);
        put_adj(o, o3 + 2 * e + 1, row0 + b, erow, 0, 1);
        put_adj(o, o4 + 2 * e, erow, row0 + a, 1, 0);
        put_adj(o, o4 + 2 * e + 1, erow, row0 + b, 1, 0);
        if (max_dim < 2) continue;
        for (int x = w; x < W; ++x) {                         // c > b: from b's word on
            const u64 ubx = mb[x] & above_in(x, b);
            for (u64 r = ma[x] & ubx; r; r &= r - 1, ++t) {
                const int ci = first_bit(r), c = x * 64 + ci;
                const long long trow = t0 + t;
                const long long eac = e0 + cloud_edge(mg, rg, up_s, W, a, c);
                const long long ebc = e0 + up_s[b] + rg[(long long)b * W + x] + __popcll(ubx & below(ci));
                put_row(o, trow, 2, g, a, b, c);
                put_adj(o, o6 + 3 * t, erow, trow, 1, 2);
                put_adj(o, o6 + 3 * t + 1, eac, trow, 1, 2);
                put_adj(o, o6 + 3 * t + 2, ebc, trow, 1, 2);
                put_adj(o, o7 + 3 * t, trow, erow, 2, 1);
                put_adj(o, o7 + 3 * t + 1, trow, eac, 2, 1);
                put_adj(o, o7 + 3 * t + 2, trow, ebc, 2, 1);
            }
        }
        for (int x = 0; x < W; ++x)
            for (u64 r = ma[x] & mb[x]; r; r &= r - 1, ++k) {
                const int y = x * 64 + first_bit(r);
                // in the sorted triple of {a, b, y} the edge {a, y} always comes before {b, y}
                const long long eay = e0 + cloud_edge(mg, rg, up_s, W, a < y ? a : y, a < y ? y : a);
                const long long eby = e0 + cloud_edge(mg, rg, up_s, W, b < y ? b : y, b < y ? y : b);
                put_adj(o, o5 + 2 * k, eay, erow, 1, 1);
                put_adj(o, o5 + 2 * k + 1, eby, erow, 1, 1);
            }
    }
}

template <bool kVertexBlock>
__global__ __launch_bounds__(kBlock) void cloud_scatter_kernel(long B, int V, int W, int tiles, int max_dim, Capacity cap, const Header* hdr,
                                                                const u64* masks, const int* rank, const int* deg, const int* up,
                                                                const int* tri, const int* cof, const int* n1, const int* n2,
                                                                const long long* row_off, const long long* adj_off, Outputs o) {
    if (!hdr->fit) return;
    const long n_real = B * tiles;                            // workgroups of the real part
    if ((long)blockIdx.x < n_real) {
        const int a = (int)(blockIdx.x % (unsigned)tiles) * kWaves + (threadIdx.x >> 6);
        if (a < V)
            cloud_scatter_vertex<kVertexBlock>((long)(blockIdx.x / (unsigned)tiles), a, threadIdx.x & 63, V, W, max_dim, masks, rank, deg, up,
                                               tri, cof, n1, n2, row_off, adj_off, o);
    } else {
        scatter_fillers((long)blockIdx.x - n_real, (long)gridDim.x - n_real, B, max_dim, cap, hdr, o);
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline bool sizes_ok(int64_t n_graphs, int32_t V, int32_t max_dim, int32_t max_verts = kMaxVerts) {
    return (max_dim == 1 || max_dim == 2) && V > max_dim && V <= max_verts && n_graphs > 0 && n_graphs < (1ll << 31) / V;
}

enum class Lift { rips, knn, hull, clique, cloud, cloud_knn };

// csmpn_cloud_lift: alignment slack + header | masks [B, V, W] | rank [B, V, W] | deg, up, tri, cof [B, V] | n1 | n2 |
// row offsets | adjacency offsets, W = ceil(V / 64) - V^2 / 8 bytes of masks and V^2 / 16 of ranks per graph
inline size_t cloud_workspace_bytes_of(int64_t n_graphs, int32_t V, int32_t max_dim) {
    if (!sizes_ok(n_graphs, V, max_dim, kCloudMaxVerts)) return 0;
    const size_t B = (size_t)n_graphs, BV = B * (size_t)V, BVW = BV * (size_t)cloud_words(V);
    return 256 + 256 + align256(sizeof(u64) * BVW) + align256(sizeof(int) * BVW) + 4 * align256(sizeof(int) * BV) +
           2 * align256(sizeof(int) * B) + 2 * align256(sizeof(long long) * B);
}

// csmpn_cloud_knn_lift: the same, then | dir [B, V, W], the masks before they are made symmetric
inline size_t cloud_knn_workspace_bytes_of(int64_t n_graphs, int32_t V, int32_t max_dim) {
    const size_t cloud = cloud_workspace_bytes_of(n_graphs, V, max_dim);
    return cloud ? cloud + align256(sizeof(u64) * (size_t)n_graphs * (size_t)V * (size_t)cloud_words(V)) : 0;
}

inline size_t workspace_bytes_of(int64_t n_graphs, int32_t V, int32_t max_dim, Lift kind = Lift::rips) {
    if (kind == Lift::cloud) return cloud_workspace_bytes_of(n_graphs, V, max_dim);
    if (kind == Lift::cloud_knn) return cloud_knn_workspace_bytes_of(n_graphs, V, max_dim);
    if (!sizes_ok(n_graphs, V, max_dim) || (kind == Lift::hull && V > kHullMaxVerts)) return 0;
    const size_t B = (size_t)n_graphs;
    // alignment slack + header | masks | n1 | n2 | row offsets | adjacency offsets; the hull lift: | T tables | volumes;
    // the thresholded clique lift: | T tables | the masks of G
    const size_t hull = kind == Lift::hull ? align256(sizeof(u64) * B * (size_t)V * (size_t)V) + align256(sizeof(float) * B) : 0;
    const size_t clique = kind == Lift::clique ? align256(sizeof(u64) * B * (size_t)V * (size_t)V) + align256(sizeof(u64) * B * (size_t)V) : 0;
    return 256 + 256 + align256(sizeof(u64) * B * (size_t)V) + 2 * align256(sizeof(int) * B) + 2 * align256(sizeof(long long) * B) + hull + clique;
}

struct LiftArgs {                // what csmpn_rips_lift and csmpn_knn_lift share
    const float* points;
    int32_t point_dim;
    int64_t n_graphs;
    int32_t verts_per_graph, max_dim;
    const int64_t* capacity_rows;
    int64_t capacity_edges;
    int64_t* x_ind;
    int32_t x_ind_cols;
    int64_t *node_types, *batch, *x_ind_batch, *ptr, *x_ind_ptr, *edge_index, *edge_types, *counts;
    uint32_t* status;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
};

struct CliqueSource {            // what csmpn_clique_lift adds: the graph (a list, or k >= 1 in the knn_k of the others) and the thresholds
    const int64_t* edge_list;
    int64_t n_list;
    double edge_th, tri_th;
};

// the checks the entries share, before the first HIP call; `what` names the entry in the messages. dis >= 0: the Rips
// threshold, knn_k: the k of the kNN entry (0 for the others) - each checked where csmpn_rips_lift has always checked dis; the
// hull entry checks its point dimension there, and its 16 vertices where the others check their 64; the clique entry checks
// its graph source and its thresholds there; the cloud entry checks its kCloudMaxVerts vertices where the others check their
// 64, and its vertex_block behind dis; the kNN cloud entry checks its vertices with the cloud entry and its k with the kNN entry.
int check_lift_args(const char* what, const LiftArgs& a, double dis, int knn_k, Lift kind, Capacity* cap, const CliqueSource* src = nullptr,
                    int vertex_block = 0) {
    const int V = a.verts_per_graph, max_dim = a.max_dim;
    const bool knn = kind == Lift::knn || kind == Lift::cloud_knn, hull = kind == Lift::hull;
    const bool cloud = kind == Lift::cloud || kind == Lift::cloud_knn;
    if (max_dim < 0) return csmpn_fail(CSMPN_ERR_INVALID, "max_dim %d is negative", max_dim);
    if (max_dim != 1 && max_dim != 2) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "%s: max_dim %d (1 or 2)", what, max_dim);
    if (hull && V > kHullMaxVerts) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "%s: %d vertices per graph > %d (every subset of point_dim vertices is tried)", what, V, kHullMaxVerts);
    if (cloud && V > kCloudMaxVerts)
        return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "%s: %d vertices per graph > kCloudMaxVerts = %d (V^2 / 8 bytes of masks and V^2 pair tests per graph)", what, V, kCloudMaxVerts);
    if (!cloud && V > kMaxVerts) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "%s: %d vertices per graph > %d (one 64-bit mask per vertex)", what, V, kMaxVerts);
    if (V <= max_dim) return csmpn_fail(CSMPN_ERR_INVALID, "%s: %d vertices per graph, max_dim %d needs %d", what, V, max_dim, max_dim + 1);
    if (a.n_graphs <= 0 || a.n_graphs >= (1ll << 31) / V) return csmpn_fail(CSMPN_ERR_INVALID, "bad sizes n_graphs=%lld verts_per_graph=%d", (long long)a.n_graphs, V);
    if (a.point_dim <= 0) return csmpn_fail(CSMPN_ERR_INVALID, "point_dim %d", (int)a.point_dim);
    if (hull && (a.point_dim < 2 || a.point_dim > 5)) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "%s: points in R^%d (2 .. 5)", what, (int)a.point_dim);
    if (hull && V <= a.point_dim) return csmpn_fail(CSMPN_ERR_INVALID, "%s: %d vertices per graph in R^%d (a hull needs %d)", what, V, (int)a.point_dim, (int)a.point_dim + 1);
    if (!knn && !hull && !(dis >= 0.0)) return csmpn_fail(CSMPN_ERR_INVALID, "dis %g is negative or not a number", dis);
    if (kind == Lift::cloud && vertex_block != 0 && vertex_block != 1) return csmpn_fail(CSMPN_ERR_INVALID, "%s: vertex_block %d (0 or 1)", what, vertex_block);
    if (knn && knn_k < 1) return csmpn_fail(CSMPN_ERR_INVALID, "%s: k = %d (at least 1)", what, knn_k);
    if (kind == Lift::clique) {
        if ((src->edge_list != nullptr) == (knn_k >= 1))
            return csmpn_fail(CSMPN_ERR_INVALID, "%s: exactly one of an edge list and k >= 1 names the graph (edge_list %s, k = %d)", what, src->edge_list ? "given" : "NULL", knn_k);
        if (src->edge_list && (src->n_list < 0 || src->n_list >= (1ll << 31))) return csmpn_fail(CSMPN_ERR_INVALID, "%s: n_list = %lld", what, (long long)src->n_list);
        if (!(src->edge_th >= 0.0)) return csmpn_fail(CSMPN_ERR_INVALID, "%s: edge_th %g is negative or not a number", what, src->edge_th);
        if (!(src->tri_th >= 0.0)) return csmpn_fail(CSMPN_ERR_INVALID, "%s: tri_th %g is negative or not a number", what, src->tri_th);
    }
    if (a.x_ind_cols <= max_dim) return csmpn_fail(CSMPN_ERR_INVALID, "x_ind has %d columns, max_dim %d needs %d", (int)a.x_ind_cols, max_dim, max_dim + 1);
    if (!a.points || !a.capacity_rows || !a.x_ind || !a.node_types || !a.batch || !a.x_ind_batch || !a.ptr || !a.x_ind_ptr || !a.edge_index)
        return csmpn_fail(CSMPN_ERR_INVALID, "null pointer");
    long long total = 0;
    for (int d = 0; d <= max_dim; ++d) {
        cap->rows[d] = a.capacity_rows[d];
        if (cap->rows[d] < 0 || cap->rows[d] >= (1ll << 31)) return csmpn_fail(CSMPN_ERR_INVALID, "capacity %lld of dimension %d", cap->rows[d], d);
        total += cap->rows[d];
    }
    cap->edges = a.capacity_edges;
    if (cap->rows[0] != a.n_graphs * V)
        return csmpn_fail(CSMPN_ERR_INVALID, "capacity_rows[0] = %lld, the batch has %lld vertices (vertex rows are never padded)", cap->rows[0], (long long)(a.n_graphs * V));
    if (total >= (1ll << 31) || cap->edges < 0 || cap->edges >= (1ll << 31))
        return csmpn_fail(CSMPN_ERR_INVALID, "bad capacity: %lld rows, %lld adjacencies", total, cap->edges);
    const size_t need = workspace_bytes_of(a.n_graphs, V, max_dim, kind);
    if (!a.workspace || a.workspace_bytes < need) return csmpn_fail(CSMPN_ERR_INVALID, "%s workspace too small: %zu < %zu", what, a.workspace_bytes, need);
    return CSMPN_OK;
}

// Behind the argument checks: the workspace carved up, then the three launches. knn_k = 0: the masks of the pairs within
// `dis` and the adjacencies with the vertex block (Rips); knn_k >= 1: the masks of the k nearest neighbours, no vertex block;
// kind == Lift::hull: the masks and the T tables of the facets, the vertex block, the volumes -> `volume` (may be null);
// kind == Lift::clique: the masks of G from src's list (zeroed on the stream first) or from the knn_k nearest neighbours, the
// filter, no vertex block - two memsets at the most and four launches.
int launch_lift(const char* what, const LiftArgs& a, const Capacity& cap, double dis, int knn_k, Lift kind = Lift::rips,
                float* volume = nullptr, const CliqueSource* src = nullptr) {
    hipStream_t st = (hipStream_t)a.stream;
    const int V = a.verts_per_graph, max_dim = a.max_dim, P = a.point_dim;
    const size_t B = (size_t)a.n_graphs;
    char* ws = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(a.workspace)));   // may cost up to 255 of the spare bytes
    Header* hdr = reinterpret_cast<Header*>(ws);
    ws += 256;
    u64* masks = reinterpret_cast<u64*>(ws);
    ws += align256(sizeof(u64) * B * (size_t)V);
    int* n1 = reinterpret_cast<int*>(ws);
    ws += align256(sizeof(int) * B);
    int* n2 = reinterpret_cast<int*>(ws);
    ws += align256(sizeof(int) * B);
    long long* row_off = reinterpret_cast<long long*>(ws);
    ws += align256(sizeof(long long) * B);
    long long* adj_off = reinterpret_cast<long long*>(ws);
    ws += align256(sizeof(long long) * B);
    const bool hull = kind == Lift::hull, clique = kind == Lift::clique;                   // their workspaces alone have these bytes
    u64* tables = hull || clique ? reinterpret_cast<u64*>(ws) : nullptr;
    u64* gmasks = clique ? reinterpret_cast<u64*>(ws + align256(sizeof(u64) * B * (size_t)V * (size_t)V)) : nullptr;
    float* vols = hull ? reinterpret_cast<float*>(ws + align256(sizeof(u64) * B * (size_t)V * (size_t)V)) : nullptr;
    Outputs out{a.x_ind, a.node_types, a.batch, a.x_ind_batch, a.edge_index, a.edge_types, (int)a.x_ind_cols, cap.edges};
    const long long fill_items = std::max(cap.rows[1] + cap.rows[2], cap.edges);
    const long fill_blocks = (long)std::min<long long>(std::max<long long>((fill_items + kBlock - 1) / kBlock, 1), kMaxFillBlocks);
    const dim3 per_graph((unsigned)B), one(1), scatter((unsigned)(B + fill_blocks)), block(kBlock);
    if (hull) {
        int n_cand = 1;                                                                    // C(V, P) <= C(16, 5)
        for (int t = 0; t < P; ++t) n_cand = n_cand * (V - t) / (t + 1);
#define CSMPN_HULL_COUNT(N)                                                                                                       \
    hipLaunchKernelGGL(lift_hull_kernel<N>, per_graph, block, 0, st, a.points, V, n_cand, max_dim, masks, tables, n1, n2, vols)
        switch (P) {
            case 2: CSMPN_HULL_COUNT(2); break;
            case 3: CSMPN_HULL_COUNT(3); break;
            case 4: CSMPN_HULL_COUNT(4); break;
            default: CSMPN_HULL_COUNT(5); break;
        }
#undef CSMPN_HULL_COUNT
        hipLaunchKernelGGL(lift_offsets_kernel<true>, one, block, 0, st, (const int*)n1, (const int*)n2, (long)B, V, max_dim, cap, hdr,
                           row_off, adj_off, a.ptr, a.x_ind_ptr, a.counts, (unsigned*)a.status);
        hipLaunchKernelGGL(lift_hull_scatter_kernel, scatter, block, 0, st, (long)B, V, max_dim, cap, (const Header*)hdr, (const u64*)masks,
                           (const u64*)tables, (const int*)n1, (const int*)n2, (const long long*)row_off, (const long long*)adj_off,
                           (const float*)vols, volume, out);
    } else if (clique) {
        hipError_t e = hipMemsetAsync(hdr, 0, 256, st);                                    // bad_list = 0
        if (e == hipSuccess && src->edge_list) e = hipMemsetAsync(gmasks, 0, sizeof(u64) * B * (size_t)V, st);
        if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "%s memset: %s", what, hipGetErrorString(e));
        if (!src->edge_list)                                                               // its counts are overwritten by the filter
            hipLaunchKernelGGL(lift_knn_kernel, per_graph, block, 0, st, a.points, P, V, knn_k, max_dim, gmasks, n1, n2);
        else if (src->n_list > 0)
            hipLaunchKernelGGL(lift_list_kernel, dim3((unsigned)((src->n_list + kBlock - 1) / kBlock)), block, 0, st, src->edge_list,
                               (long long)src->n_list, (long long)(B * (size_t)V), V, gmasks, &hdr->bad_list);
        hipLaunchKernelGGL(lift_filter_kernel, per_graph, block, 0, st, a.points, P, V, src->edge_th * src->edge_th,
                           4.0 * src->tri_th * src->tri_th, max_dim, (const u64*)gmasks, masks, tables, n1, n2);
        hipLaunchKernelGGL((lift_offsets_kernel<false, true>), one, block, 0, st, (const int*)n1, (const int*)n2, (long)B, V, max_dim, cap,
                           hdr, row_off, adj_off, a.ptr, a.x_ind_ptr, a.counts, (unsigned*)a.status);
        hipLaunchKernelGGL(lift_clique_scatter_kernel, scatter, block, 0, st, (long)B, V, max_dim, cap, (const Header*)hdr, (const u64*)masks,
                           (const u64*)tables, (const int*)n1, (const int*)n2, (const long long*)row_off, (const long long*)adj_off, out);
    } else if (knn_k > 0) {
        hipLaunchKernelGGL(lift_knn_kernel, per_graph, block, 0, st, a.points, P, V, knn_k, max_dim, masks, n1, n2);
        hipLaunchKernelGGL(lift_offsets_kernel<false>, one, block, 0, st, (const int*)n1, (const int*)n2, (long)B, V, max_dim, cap, hdr,
                           row_off, adj_off, a.ptr, a.x_ind_ptr, a.counts, (unsigned*)a.status);
        hipLaunchKernelGGL(lift_scatter_kernel<false>, scatter, block, 0, st, (long)B, V, max_dim, cap, (const Header*)hdr,
                           (const u64*)masks, (const int*)n1, (const int*)n2, (const long long*)row_off, (const long long*)adj_off, out);
    } else {
        hipLaunchKernelGGL(lift_count_kernel, per_graph, block, 0, st, a.points, P, V, dis * dis, max_dim, masks, n1, n2);
        hipLaunchKernelGGL(lift_offsets_kernel<true>, one, block, 0, st, (const int*)n1, (const int*)n2, (long)B, V, max_dim, cap, hdr,
                           row_off, adj_off, a.ptr, a.x_ind_ptr, a.counts, (unsigned*)a.status);
        hipLaunchKernelGGL(lift_scatter_kernel<true>, scatter, block, 0, st, (long)B, V, max_dim, cap, (const Header*)hdr,
                           (const u64*)masks, (const int*)n1, (const int*)n2, (const long long*)row_off, (const long long*)adj_off, out);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "%s kernels: %s", what, hipGetErrorString(e));
    return CSMPN_OK;
}

// csmpn_cloud_lift behind the argument checks: the workspace carved up (cloud_workspace_bytes_of), then five launches - four
// for max_dim = 1, which has no triangle to count. knn_k >= 1: csmpn_cloud_knn_lift - the select and mask kernels in the place
// of cloud_mask_kernel (one launch more), dir behind the cloud entry's parts, no vertex block.
int launch_cloud_lift(const char* what, const LiftArgs& a, const Capacity& cap, double dis, bool vertex_block, int knn_k = 0) {
    hipStream_t st = (hipStream_t)a.stream;
    const int V = a.verts_per_graph, W = cloud_words(V), max_dim = a.max_dim, tiles = (V + kWaves - 1) / kWaves;
    const size_t B = (size_t)a.n_graphs, BV = B * (size_t)V, BVW = BV * (size_t)W;
    char* ws = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(a.workspace)));
    const auto carve = [&ws](size_t bytes) {
        char* p = ws;
        ws += align256(bytes);
        return p;
    };
    Header* hdr = reinterpret_cast<Header*>(carve(256));
    u64* masks = reinterpret_cast<u64*>(carve(sizeof(u64) * BVW));
    int* rank = reinterpret_cast<int*>(carve(sizeof(int) * BVW));
    int* deg = reinterpret_cast<int*>(carve(sizeof(int) * BV));
    int* up = reinterpret_cast<int*>(carve(sizeof(int) * BV));
    int* tri = reinterpret_cast<int*>(carve(sizeof(int) * BV));
    int* cof = reinterpret_cast<int*>(carve(sizeof(int) * BV));
    int* n1 = reinterpret_cast<int*>(carve(sizeof(int) * B));
    int* n2 = reinterpret_cast<int*>(carve(sizeof(int) * B));
    long long* row_off = reinterpret_cast<long long*>(carve(sizeof(long long) * B));
    long long* adj_off = reinterpret_cast<long long*>(carve(sizeof(long long) * B));
    u64* dir = knn_k > 0 ? reinterpret_cast<u64*>(carve(sizeof(u64) * BVW)) : nullptr;   // the kNN workspace alone has these bytes
    Outputs out{a.x_ind, a.node_types, a.batch, a.x_ind_batch, a.edge_index, a.edge_types, (int)a.x_ind_cols, cap.edges};
    const long long fill_items = std::max(cap.rows[1] + cap.rows[2], cap.edges);
    const long fill_blocks = (long)std::min<long long>(std::max<long long>((fill_items + kBlock - 1) / kBlock, 1), kMaxFillBlocks);
    const dim3 per_vertex((unsigned)(B * (size_t)tiles)), per_graph((unsigned)B), one(1), scatter((unsigned)(B * (size_t)tiles + fill_blocks)),
        block(kBlock);
    if (knn_k > 0) {
#define CSMPN_CLOUD_SELECT(WORDS) \
    hipLaunchKernelGGL(cloud_knn_select_kernel<WORDS>, per_vertex, block, 0, st, a.points, (int)a.point_dim, V, W, tiles, knn_k, dir)
        if (W <= 1) CSMPN_CLOUD_SELECT(1);
        else if (W <= 2) CSMPN_CLOUD_SELECT(2);
        else if (W <= 4) CSMPN_CLOUD_SELECT(4);
        else if (W <= 16) CSMPN_CLOUD_SELECT(16);
        else CSMPN_CLOUD_SELECT(64);
#undef CSMPN_CLOUD_SELECT
        hipLaunchKernelGGL(cloud_knn_mask_kernel, per_vertex, block, 0, st, V, W, tiles, (const u64*)dir, masks, rank, deg, up);
    } else {
        hipLaunchKernelGGL(cloud_mask_kernel, per_vertex, block, 0, st, a.points, (int)a.point_dim, V, W, tiles, dis * dis, masks, rank, deg, up);
    }
    if (max_dim >= 2) hipLaunchKernelGGL(cloud_count_kernel, per_vertex, block, 0, st, V, W, tiles, (const u64*)masks, tri, cof);
    hipLaunchKernelGGL(cloud_scan_kernel, per_graph, block, 0, st, V, max_dim, deg, up, tri, cof, n1, n2);
#define CSMPN_CLOUD_TAIL(BLOCK)                                                                                                                   \
    hipLaunchKernelGGL(lift_offsets_kernel<BLOCK>, one, block, 0, st, (const int*)n1, (const int*)n2, (long)B, V, max_dim, cap, hdr, row_off,    \
                       adj_off, a.ptr, a.x_ind_ptr, a.counts, (unsigned*)a.status);                                                              \
    hipLaunchKernelGGL(cloud_scatter_kernel<BLOCK>, scatter, block, 0, st, (long)B, V, W, tiles, max_dim, cap, (const Header*)hdr,                \
                       (const u64*)masks, (const int*)rank, (const int*)deg, (const int*)up, (const int*)tri, (const int*)cof, (const int*)n1,   \
                       (const int*)n2, (const long long*)row_off, (const long long*)adj_off, out)
    if (vertex_block) {
        CSMPN_CLOUD_TAIL(true);
    } else {
        CSMPN_CLOUD_TAIL(false);
    }
#undef CSMPN_CLOUD_TAIL
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "%s kernels: %s", what, hipGetErrorString(e));
    return CSMPN_OK;
}

}  // namespace

extern "C" {

size_t csmpn_cloud_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim) {
    return workspace_bytes_of(n_graphs, verts_per_graph, max_dim, Lift::cloud);
}

int csmpn_cloud_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, double dis, int32_t vertex_block,
                     int32_t max_dim, const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols,
                     int64_t* node_types, int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index,
                     int64_t* edge_types, int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const LiftArgs a{points, point_dim, n_graphs, verts_per_graph, max_dim, capacity_rows, capacity_edges, x_ind, x_ind_cols, node_types,
                     batch, x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status, workspace, workspace_bytes, stream};
    Capacity cap{};
    if (const int rc = check_lift_args("cloud lift", a, dis, 0, Lift::cloud, &cap, nullptr, (int)vertex_block)) return rc;
    return launch_cloud_lift("cloud lift", a, cap, dis, vertex_block == 1);
}

size_t csmpn_cloud_knn_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim) {
    return workspace_bytes_of(n_graphs, verts_per_graph, max_dim, Lift::cloud_knn);
}

int csmpn_cloud_knn_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t k, int32_t max_dim,
                         const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                         int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                         int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const LiftArgs a{points, point_dim, n_graphs, verts_per_graph, max_dim, capacity_rows, capacity_edges, x_ind, x_ind_cols, node_types,
                     batch, x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status, workspace, workspace_bytes, stream};
    Capacity cap{};
    if (const int rc = check_lift_args("cloud knn lift", a, 0.0, (int)k, Lift::cloud_knn, &cap)) return rc;
    return launch_cloud_lift("cloud knn lift", a, cap, 0.0, false, (int)k);
}

size_t csmpn_rips_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim) {
    return workspace_bytes_of(n_graphs, verts_per_graph, max_dim);
}

size_t csmpn_knn_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim) {
    return workspace_bytes_of(n_graphs, verts_per_graph, max_dim);
}

int csmpn_rips_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, double dis, int32_t max_dim,
                    const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                    int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                    int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const LiftArgs a{points, point_dim, n_graphs, verts_per_graph, max_dim, capacity_rows, capacity_edges, x_ind, x_ind_cols, node_types,
                     batch, x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status, workspace, workspace_bytes, stream};
    Capacity cap{};
    if (const int rc = check_lift_args("rips lift", a, dis, 0, Lift::rips, &cap)) return rc;
    return launch_lift("rips lift", a, cap, dis, 0);
}

int csmpn_knn_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t k, int32_t max_dim,
                   const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                   int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                   int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const LiftArgs a{points, point_dim, n_graphs, verts_per_graph, max_dim, capacity_rows, capacity_edges, x_ind, x_ind_cols, node_types,
                     batch, x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status, workspace, workspace_bytes, stream};
    Capacity cap{};
    if (const int rc = check_lift_args("knn lift", a, 0.0, (int)k, Lift::knn, &cap)) return rc;
    return launch_lift("knn lift", a, cap, 0.0, (int)k);
}

size_t csmpn_hull_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim) {
    return workspace_bytes_of(n_graphs, verts_per_graph, max_dim, Lift::hull);
}

int csmpn_hull_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim,
                    const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                    int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                    int64_t* counts, uint32_t* status, float* volume, void* workspace, size_t workspace_bytes, void* stream) {
    const LiftArgs a{points, point_dim, n_graphs, verts_per_graph, max_dim, capacity_rows, capacity_edges, x_ind, x_ind_cols, node_types,
                     batch, x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status, workspace, workspace_bytes, stream};
    Capacity cap{};
    if (const int rc = check_lift_args("hull lift", a, 0.0, 0, Lift::hull, &cap)) return rc;
    return launch_lift("hull lift", a, cap, 0.0, 0, Lift::hull, volume);
}

size_t csmpn_clique_lift_workspace_bytes(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim) {
    return workspace_bytes_of(n_graphs, verts_per_graph, max_dim, Lift::clique);
}

int csmpn_clique_lift(const float* points, int32_t point_dim, int64_t n_graphs, int32_t verts_per_graph, int32_t k,
                      const int64_t* edge_list, int64_t n_list, double edge_th, double tri_th, int32_t max_dim,
                      const int64_t* capacity_rows, int64_t capacity_edges, int64_t* x_ind, int32_t x_ind_cols, int64_t* node_types,
                      int64_t* batch, int64_t* x_ind_batch, int64_t* ptr, int64_t* x_ind_ptr, int64_t* edge_index, int64_t* edge_types,
                      int64_t* counts, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const LiftArgs a{points, point_dim, n_graphs, verts_per_graph, max_dim, capacity_rows, capacity_edges, x_ind, x_ind_cols, node_types,
                     batch, x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status, workspace, workspace_bytes, stream};
    const CliqueSource src{edge_list, n_list, edge_th, tri_th};
    Capacity cap{};
    if (const int rc = check_lift_args("clique lift", a, 0.0, (int)k, Lift::clique, &cap, &src)) return rc;
    return launch_lift("clique lift", a, cap, 0.0, (int)k, Lift::clique, nullptr, &src);
}

}  // extern "C"
