// Float64 CEMLP / EGCL kernel family ("f64"): one row-tile kernel in double per compiled algebra and direction, built for
// correctness and a fixed summation order, not for the roofline. The arithmetic is that of oracle/cpu_twin/csmpn_cpu.cpp
// (block_forward / block_backward, phase by phase, every sum in the twin's order) with the reference's float64 constants
// (1e-16 in smooth_abs_sqrt, 1e-6 in the two normalisations). The units are compiled without FMA contraction, as the twin is
// (csrc/Makefile says why): every product is rounded as in the reference's torch ops.
//
// Mapping. A 256-lane workgroup takes a tile of R rows; tile t goes to workgroup t mod grid (grid <= kGridCap). The state
// of ONE block of the tile sits in LDS as doubles: y, z, R, s and, for the backward, ggp, gz (later gy), gr (later gR),
// plus the per-(row, channel, grade) scalars. Lanes loop over (row, channel, blade) with run-time widths; the only
// template parameters are the algebra and forward / backward (12 kernels in the library: the three modes differ in how a
// row is gathered and where its results go, which the IO descriptor states at run time). No per-lane arrays: nothing to spill.
// Block inputs travel through a per-workgroup region of the workspace (input rows are streamed from there, so in_features
// is unbounded); the backward keeps every block's input there, recomputes a block's state from it and walks the blocks
// back to front.
//
// Fixed order everywhere, no atomics. Each parameter-gradient element is owned by one lane, which adds the rows of a tile
// in ascending order into the workgroup's own slice of the workspace; slices_sum_kernel then adds the slices in ascending
// workgroup order INTO the gradient tensors (+=). The edge stage never scatters: it writes row tables in sorted edge order
// and segment_reduce_f64_kernel sums them per node in a fixed order.
//
// Limits: out_features of every block 1..kMaxWidth (64): one row of a block must fit the LDS (7 * 64 * 32 doubles + scalars =
// 118 KB at Cl(5,0) / Cl(4,1)); in_features unbounded; 1..4 blocks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "algebra.hpp"

namespace csmpn {
namespace f64 {

constexpr int kThreads = 256, kMaxBlocks = 4, kMaxWidth = 64, kGridCap = 256, kMaxTileRows = 32, kTensors = 10;
constexpr size_t kLdsSmall = 64 * 1024, kLdsMax = 160 * 1024;   // budget: 64 KB (two workgroups per CU) unless one row needs more

struct Blk {
    int I, O, sub;
    const double *W1, *b1, *sa, *sb, *w, *an, *WR, *WL, *bL, *la;
    long slice_off;   // of this block's gradient slice inside a workgroup's slice region (doubles)
    long act_off;     // of this block's input rows inside a workgroup's activation region (doubles)
};

// one channel segment of the input row: x[c] = a[ia ? ia[row] : row] - (b ? b[ib[row]] : 0), times 1 / max(deg[row], 1)
// with deg; backward: g[gi ? gi[row] : row] = d/dx of the segment (same scale), nullptr: not wanted
struct Seg {
    const double *a, *b;
    const int *ia, *ib, *deg, *gi;
    double* g;
    int ch, off;
    long a_rows;      // rows of a (and b): gathered indices are clamped into [0, a_rows)
};

struct Args {
    Blk blk[kMaxBlocks];
    Seg seg[3];
    int nblk, nseg, R, maxO, resid_bwd;
    long rows, tiles, gy_rows;
    double* y;             // forward: [rows, O, D]
    const double* resid;   // forward: added to y (node stage residual), or nullptr
    const double* gy;      // backward: [*, O, D]
    const int* gy_idx;     // backward: row of gy per row (edge stage: the target node), nullptr = the row itself
    double* ws;
    long wg_doubles, slice_doubles, act_doubles, g_doubles;   // per-workgroup region: slices | block inputs | 2 gradient row buffers
};

// doubles of LDS per tile row: 7 row tensors, 5 per-(channel, grade) scalars, 3 per-channel scalars, invMn and gMn
inline long lds_row_doubles(int maxO, int D, int G) { return 7L * maxO * D + 5L * maxO * G + 3L * maxO + 2; }

template <class A>
struct Tab {
    static constexpr int D = A::D, G = A::G, P = A::P;
    unsigned char out[D * D];     // index of blade_i * blade_k (symmetric in i, k)
    signed char sgn[D * D];       // its sign, metric included
    unsigned char pid[D * D];     // its grade path
    signed char qs[D];
    unsigned char grade[D];
    unsigned char gstart[G + 1];
    unsigned short pstart[P + 1]; // pairs (i, k) of one path, in (i, k) order
    unsigned char pi[D * D], pk[D * D];
};

template <class A>
constexpr Tab<A> make_tab() {
    Tab<A> t{};
    constexpr int D = A::D, G = A::G, P = A::P;
    int cnt[P + 1] = {};
    for (int i = 0; i < D; ++i) {
        t.qs[i] = A::t.qsign[i];
        t.grade[i] = (unsigned char)A::t.bo.grade[i];
        for (int k = 0; k < D; ++k) {
            const int j = A::t.out[i][k];
            t.out[i * D + k] = (unsigned char)j;
            t.sgn[i * D + k] = A::t.sign[i][k];
            const int p = A::t.path_id[A::t.bo.grade[i]][A::t.bo.grade[j]][A::t.bo.grade[k]];
            t.pid[i * D + k] = (unsigned char)p;
            ++cnt[p];
        }
    }
    for (int g = 0; g <= G; ++g) t.gstart[g] = (unsigned char)A::t.bo.gstart[g];
    int pos = 0;
    for (int p = 0; p < P; ++p) { t.pstart[p] = (unsigned short)pos; pos += cnt[p]; cnt[p] = t.pstart[p]; }
    t.pstart[P] = (unsigned short)pos;
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            const int q = cnt[t.pid[i * D + k]]++;
            t.pi[q] = (unsigned char)i; t.pk[q] = (unsigned char)k;
        }
    return t;
}

template <class A>
__constant__ const Tab<A> g_tab = make_tab<A>();

__device__ __forceinline__ double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double smooth_abs_sqrt(double q) { return sqrt(sqrt(q * q + 1e-16)); }
constexpr double kEps = 1e-6, kInvSqrt2 = 0.70710678118654752440;

// LDS of one tile: row tensors indexed [r * O * D + o * D + d], scalars [r * O * G + o * G + g] / [r * O + o] / [r]
struct Lds {
    double *Y, *Z, *RR, *S, *GGP, *GZ, *GR, *gate, *invden, *uu, *gpre, *ganc, *qs, *nl, *dot, *invMn, *gMn;
    __device__ Lds(double* p, int R, int maxO, int D, int G) {
        const long t = (long)R * maxO * D, c = (long)R * maxO * G, o = (long)R * maxO;
        Y = p; Z = Y + t; RR = Z + t; S = RR + t; GGP = S + t; GZ = GGP + t; GR = GZ + t;
        gate = GR + t; invden = gate + c; uu = invden + c; gpre = uu + c; ganc = gpre + c;
        qs = ganc + c; nl = qs + o; dot = nl + o; invMn = dot + o; gMn = invMn + R;
    }
};

// state of block B for the nr rows at x ([nr, I, D], workspace); dst ([nr, O, D]) gets the block's output (+ resid) unless null
template <class A>
__device__ void block_forward(const Blk& B, int nr, const double* __restrict__ x, double* __restrict__ dst,
                              const double* __restrict__ resid, const Lds& l) {
    constexpr int D = A::D, G = A::G, P = A::P;
    const Tab<A>& T = g_tab<A>;
    const int tid = threadIdx.x, I = B.I, O = B.O, OD = O * D, OG = O * G;
    for (int e = tid; e < nr * OD; e += kThreads) {            // MVLinear
        const int r = e / OD, f = e - r * OD, o = f / D, d = f - o * D, g = T.grade[d];
        double acc = (d == 0 && B.b1) ? B.b1[o] : 0.0;
        const double* xr = x + (long)r * I * D + d;
        const double* w = B.sub ? B.W1 + (long)o * I * G + g : B.W1 + (long)o * I;
        const int wst = B.sub ? G : 1;
        for (int i = 0; i < I; ++i) acc += w[(long)i * wst] * xr[(long)i * D];
        l.Y[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // MVSiLU
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const double* y = l.Y + r * OD + o * D;
        double* z = l.Z + r * OD + o * D;
        double u = 0.0;
        if (g == 0) u = y[0];
        else for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) u += double(T.qs[d]) * y[d] * y[d];
        const double gt = sigmoid(B.sa[o * G + g] * u + B.sb[o * G + g]);
        l.gate[e] = gt; l.uu[e] = u;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) z[d] = gt * y[d];
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // linear_right, linear_left (into S)
        const int r = e / OD, f = e - r * OD, o = f / D, d = f - o * D, g = T.grade[d];
        double ar = 0.0, al = (d == 0) ? B.bL[o] : 0.0;
        const double* z = l.Z + r * OD + d;
        const double *wr = B.WR + (long)o * O * G + g, *wl = B.WL + (long)o * O * G + g;
        for (int i = 0; i < O; ++i) { ar += wr[i * G] * z[i * D]; al += wl[i * G] * z[i * D]; }
        l.RR[e] = ar; l.S[e] = al;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // NormalizationLayer
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const double* R = l.RR + r * OD + o * D;
        double qq = 0.0;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) qq += double(T.qs[d]) * R[d] * R[d];
        const double m = sigmoid(B.an[o * G + g]) * (smooth_abs_sqrt(qq) - 1.0) + 1.0;
        l.invden[e] = 1.0 / (m + kEps);
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // geometric product: blade j of the output, left blades ascending
        const int r = e / OD, f = e - r * OD, o = f / D, j = f - o * D;
        const double *z = l.Z + r * OD + o * D, *R = l.RR + r * OD + o * D, *inv = l.invden + r * OG + o * G, *w = B.w + (long)o * P;
        double acc = l.S[e];
        for (int i = 0; i < D; ++i) {
            const int k = T.out[i * D + j], q = i * D + k;
            acc += double(T.sgn[q]) * w[T.pid[q]] * z[i] * (R[k] * inv[T.grade[k]]);
        }
        l.S[e] = acc * kInvSqrt2;
    }
    __syncthreads();
    for (int e = tid; e < nr * O; e += kThreads) {             // MVLayerNorm
        const double* s = l.S + (long)e * D;
        double qs = 0.0;
        for (int d = 0; d < D; ++d) qs += double(T.qs[d]) * s[d] * s[d];
        l.qs[e] = qs; l.nl[e] = smooth_abs_sqrt(qs);
    }
    __syncthreads();
    if (tid < nr) {
        double nsum = 0.0;
        for (int o = 0; o < O; ++o) nsum += l.nl[tid * O + o];
        l.invMn[tid] = 1.0 / (nsum / double(O) + kEps);
    }
    __syncthreads();
    if (dst)
        for (int e = tid; e < nr * OD; e += kThreads) {
            const int r = e / OD, o = (e - r * OD) / D;
            double v = B.la[o] * l.S[e] * l.invMn[r];
            if (resid) v += resid[e];
            dst[e] = v;
        }
    __syncthreads();
}

// backward of block B on the state block_forward left in LDS: gx ([nr, I, D]) from gout ([nr, O, D]); the parameter
// gradients of the nr rows are added to the workgroup's slice, each element by its one owning lane in row order
template <class A>
__device__ void block_backward(const Blk& B, int nr, const double* __restrict__ x, const double* __restrict__ gout,
                               double* __restrict__ gx, double* __restrict__ slice, const Lds& l) {
    constexpr int D = A::D, G = A::G, P = A::P;
    const Tab<A>& T = g_tab<A>;
    const int tid = threadIdx.x, I = B.I, O = B.O, OD = O * D, OG = O * G;
    for (int e = tid; e < nr * O; e += kThreads) {             // MVLayerNorm
        double dt = 0.0;
        for (int d = 0; d < D; ++d) dt += gout[(long)e * D + d] * l.S[(long)e * D + d];
        l.dot[e] = dt;
    }
    __syncthreads();
    if (tid < nr) {
        double gm = 0.0;
        for (int o = 0; o < O; ++o) gm -= B.la[o] * l.dot[tid * O + o];
        l.gMn[tid] = gm * (l.invMn[tid] * l.invMn[tid] / double(O));
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {
        const int r = e / OD, f = e - r * OD, o = f / D, d = f - o * D;
        const double inl = 1.0 / l.nl[r * O + o];
        const double gqs = l.gMn[r] * 0.5 * l.qs[r * O + o] * inl * inl * inl;
        l.GGP[e] = (B.la[o] * gout[e] * l.invMn[r] + gqs * 2.0 * double(T.qs[d]) * l.S[e]) * kInvSqrt2;
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // linear_left and the geometric product: gz, gr
        const int r = e / OD, f = e - r * OD, c = f / D, b = f - c * D, g = T.grade[b];
        const double *ggp = l.GGP + r * OD, *z = l.Z + r * OD + c * D, *R = l.RR + r * OD + c * D, *inv = l.invden + r * OG + c * G;
        const double* w = B.w + (long)c * P;
        double gz = 0.0, gr = 0.0;
        for (int o = 0; o < O; ++o) gz += B.WL[((long)o * O + c) * G + g] * ggp[o * D + b];
        for (int k = 0; k < D; ++k) {                          // b as the left blade i
            const int q = b * D + k, j = T.out[q];
            gz += w[T.pid[q]] * (double(T.sgn[q]) * ggp[c * D + j]) * (R[k] * inv[T.grade[k]]);
        }
        for (int i = 0; i < D; ++i) {                          // b as the right blade k
            const int q = i * D + b, j = T.out[q];
            gr += w[T.pid[q]] * (double(T.sgn[q]) * ggp[c * D + j]) * z[i];
        }
        l.GZ[e] = gz; l.GR[e] = gr;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // NormalizationLayer: gr -> gR in place
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const double* R = l.RR + r * OD + o * D;
        double* gr = l.GR + r * OD + o * D;
        double gden = 0.0, qR = 0.0;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) { gden -= gr[d] * R[d]; qR += double(T.qs[d]) * R[d] * R[d]; }
        const double inv = l.invden[e];
        gden *= inv * inv;
        const double nu = smooth_abs_sqrt(qR), sg = sigmoid(B.an[o * G + g]);
        l.ganc[e] = gden * (nu - 1.0) * sg * (1.0 - sg);
        const double gq = gden * sg * 0.5 * qR / (nu * nu * nu);
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) gr[d] = gr[d] * inv + gq * 2.0 * double(T.qs[d]) * R[d];
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // linear_right
        const int r = e / OD, f = e - r * OD, c = f / D, d = f - c * D, g = T.grade[d];
        double gz = l.GZ[e];
        for (int o = 0; o < O; ++o) gz += B.WR[((long)o * O + c) * G + g] * l.GR[r * OD + o * D + d];
        l.GZ[e] = gz;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // MVSiLU: gz -> gy in place
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const double* y = l.Y + r * OD + o * D;
        double* gz = l.GZ + r * OD + o * D;
        double ggate = 0.0;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) ggate += gz[d] * y[d];
        const double gt = l.gate[e], gpre = ggate * gt * (1.0 - gt), gu = gpre * B.sa[o * G + g];
        l.gpre[e] = gpre;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d)
            gz[d] = gz[d] * gt + (g == 0 ? gu : gu * 2.0 * double(T.qs[d]) * y[d]);
    }
    __syncthreads();
    if (gx)
        for (int e = tid; e < nr * I * D; e += kThreads) {     // MVLinear: d/dx
            const int r = e / (I * D), f = e - r * I * D, i = f / D, d = f - i * D, g = T.grade[d];
            const double* gy = l.GZ + r * OD + d;
            double acc = 0.0;
            for (int o = 0; o < O; ++o) acc += (B.sub ? B.W1[((long)o * I + i) * G + g] : B.W1[(long)o * I + i]) * gy[o * D];
            gx[e] = acc;
        }
    // parameter gradients, slice layout: W1 | b1 | sa | sb | w | an | WR | WL | bL | la
    const long nW1 = (long)O * I * (B.sub ? G : 1), oOG = OG, nw = (long)O * P, nOO = (long)O * O * G;
    const long o_b1 = nW1, o_sa = o_b1 + O, o_sb = o_sa + oOG, o_w = o_sb + oOG, o_an = o_w + nw, o_WR = o_an + oOG, o_WL = o_WR + nOO,
               o_bL = o_WL + nOO, o_la = o_bL + O, total = o_la + O;
    for (long e = tid; e < total; e += kThreads) {
        double acc = slice[e];
        if (e < o_b1) {
            const int g = B.sub ? int(e % G) : 0;
            const long oi = B.sub ? e / G : e;
            const int o = int(oi / I), i = int(oi - (long)o * I);
            const int d0 = B.sub ? T.gstart[g] : 0, d1 = B.sub ? T.gstart[g + 1] : D;
            for (int r = 0; r < nr; ++r)
                for (int d = d0; d < d1; ++d) acc += l.GZ[r * OD + o * D + d] * x[((long)r * I + i) * D + d];
        } else if (e < o_sa) {
            const int o = int(e - o_b1);
            for (int r = 0; r < nr; ++r) acc += l.GZ[r * OD + o * D];
        } else if (e < o_sb) {
            const int f = int(e - o_sa);
            for (int r = 0; r < nr; ++r) acc += l.gpre[r * OG + f] * l.uu[r * OG + f];
        } else if (e < o_w) {
            const int f = int(e - o_sb);
            for (int r = 0; r < nr; ++r) acc += l.gpre[r * OG + f];
        } else if (e < o_an) {
            const int f = int(e - o_w), o = f / P, p = f - o * P;
            for (int r = 0; r < nr; ++r) {
                const double *ggp = l.GGP + r * OD + o * D, *z = l.Z + r * OD + o * D, *R = l.RR + r * OD + o * D,
                             *inv = l.invden + r * OG + o * G;
                for (int q = T.pstart[p]; q < T.pstart[p + 1]; ++q) {
                    const int i = T.pi[q], k = T.pk[q], ik = i * D + k;
                    acc += double(T.sgn[ik]) * ggp[T.out[ik]] * z[i] * (R[k] * inv[T.grade[k]]);
                }
            }
        } else if (e < o_WR) {
            const int f = int(e - o_an);
            for (int r = 0; r < nr; ++r) acc += l.ganc[r * OG + f];
        } else if (e < o_bL) {
            const bool left = e >= o_WL;
            const long f = e - (left ? o_WL : o_WR);
            const int g = int(f % G), o = int(f / G / O), i = int(f / G - (long)o * O);
            const double* gsrc = left ? l.GGP : l.GR;
            for (int r = 0; r < nr; ++r)
                for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) acc += gsrc[r * OD + o * D + d] * l.Z[r * OD + i * D + d];
        } else if (e < o_la) {
            const int o = int(e - o_bL);
            for (int r = 0; r < nr; ++r) acc += l.GGP[r * OD + o * D];
        } else {
            const int o = int(e - o_la);
            for (int r = 0; r < nr; ++r) acc += l.dot[r * O + o] * l.invMn[r];
        }
        slice[e] = acc;
    }
    __syncthreads();
}

__device__ __forceinline__ long clamp_row(long v, long n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

template <class A, bool BWD>
__global__ __launch_bounds__(kThreads) void cemlp_f64_kernel(const Args a) {
    extern __shared__ double f64_lds[];
    constexpr int D = A::D, G = A::G;
    const int tid = threadIdx.x;
    const Lds l(f64_lds, a.R, a.maxO, D, G);
    double* slice = a.ws + (long)blockIdx.x * a.wg_doubles;
    double* act = slice + a.slice_doubles;
    double* gbuf[2] = {act + a.act_doubles, act + a.act_doubles + a.g_doubles};
    if (BWD) {
        for (long e = tid; e < a.slice_doubles; e += kThreads) slice[e] = 0.0;
        __syncthreads();
    }
    const int I0 = a.blk[0].I, OL = a.blk[a.nblk - 1].O;
    for (long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const long r0 = t * a.R;
        const int nr = int(a.rows - r0 < a.R ? a.rows - r0 : a.R);
        for (int e = tid; e < nr * I0 * D; e += kThreads) {    // the input rows of block 0
            const int r = e / (I0 * D), f = e - r * I0 * D, c = f / D, d = f - c * D;
            const int s = (a.nseg > 2 && c >= a.seg[2].off) ? 2 : ((a.nseg > 1 && c >= a.seg[1].off) ? 1 : 0);
            const Seg& sg = a.seg[s];
            const long row = r0 + r, col = (long)(c - sg.off) * D + d, w = (long)sg.ch * D;
            double v = sg.a[clamp_row(sg.ia ? sg.ia[row] : row, sg.a_rows) * w + col];
            if (sg.b) v -= sg.b[clamp_row(sg.ib[row], sg.a_rows) * w + col];
            if (sg.deg) { const int dg = sg.deg[row]; v *= 1.0 / double(dg > 1 ? dg : 1); }
            act[e] = v;
        }
        __syncthreads();
        for (int k = 0; k < a.nblk; ++k) {
            const bool last = k + 1 == a.nblk;
            double* dst = last ? (BWD ? nullptr : a.y + r0 * OL * D) : act + a.blk[k + 1].act_off;
            block_forward<A>(a.blk[k], nr, act + a.blk[k].act_off, dst, (last && !BWD && a.resid) ? a.resid + r0 * OL * D : nullptr, l);
        }
        if (BWD) {
            for (int e = tid; e < nr * OL * D; e += kThreads) {
                const long row = r0 + e / (OL * D);
                gbuf[0][e] = a.gy[clamp_row(a.gy_idx ? a.gy_idx[row] : row, a.gy_rows) * OL * D + e % (OL * D)];
            }
            __syncthreads();
            int cur = 0;
            for (int k = a.nblk - 1; k >= 0; --k) {
                const double* xk = act + a.blk[k].act_off;
                if (k + 1 != a.nblk) block_forward<A>(a.blk[k], nr, xk, nullptr, nullptr, l);   // the last block's state is still there
                block_backward<A>(a.blk[k], nr, xk, gbuf[cur], gbuf[cur ^ 1], slice + a.blk[k].slice_off, l);
                cur ^= 1;
            }
            const double* gx = gbuf[cur];
            for (int e = tid; e < nr * I0 * D; e += kThreads) {
                const int r = e / (I0 * D), f = e - r * I0 * D, c = f / D, d = f - c * D;
                const int s = (a.nseg > 2 && c >= a.seg[2].off) ? 2 : ((a.nseg > 1 && c >= a.seg[1].off) ? 1 : 0);
                const Seg& sg = a.seg[s];
                if (!sg.g) continue;
                const long row = r0 + r, col = (long)(c - sg.off) * D + d, w = (long)sg.ch * D;
                double v = gx[e];
                if (sg.deg) { const int dg = sg.deg[row]; v *= 1.0 / double(dg > 1 ? dg : 1); }
                if (s == 0 && a.resid_bwd) v += a.gy[row * OL * D + col];
                sg.g[(sg.gi ? clamp_row(sg.gi[row], a.rows) : row) * w + col] = v;
            }
            __syncthreads();
        }
    }
}

}  // namespace f64
}  // namespace csmpn
