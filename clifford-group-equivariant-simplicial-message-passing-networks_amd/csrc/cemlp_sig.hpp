// Run-time-signature CEMLP / EGCL kernel family ("sig"): the row-tile kernel of cemlp_f64.hpp with the signature of the
// algebra as a kernel ARGUMENT (`unsigned neg`: bit b set = generator b squares to -1) instead of a template parameter, in
// float or double. One kernel per (n, Real, direction): 16 kernels serve all 60 signatures Cl(p,q), p + q = 2..5.
//
// What depends on the metric. The blade order, the output index of a product, the grade paths and the pair lists of a
// path depend on n alone (layers.hip asserts it); they come from the __constant__ table of Alg<N, 0>. The metric enters
// in two places only:
//   sign(i, k) = structural sign of Alg<N, 0>, flipped when blades i and k share an odd number of negative generators;
//   qsign(d)   = structural qsign, flipped when blade d holds an odd number of negative generators
// (sig_flip below, __host__ __device__: the one statement of the rule). Each workgroup expands the rule ONCE into a
// D x D + D byte table in LDS (1056 bytes at n = 5) behind the tile state: the inner loops then read their sign with one
// ds_read_i8 where cemlp_f64.hpp reads T.sgn through the vector cache - no instruction more per product term. Computing
// the flip per use would add a bitmap load, an AND and a parity fold to every term of the D-long product loops.
//
// Everything else - mapping, phase order, summation order, the IO descriptor of the three modes, no atomics, no saved
// buffers - is cemlp_f64.hpp's, statement by statement: in double the two kernels produce the same bits on the six compiled
// algebras (a sign is an exact factor). In float the constants are the reference's float32 ones (1e-16f, 1e-6f), as in the
// float32 build of the C++ twin.
//
// Limits: those of cemlp_f64.hpp (1..4 blocks, out_features 1..64 per block, in_features unbounded).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "algebra.hpp"
#include "cemlp_f64.hpp"

namespace csmpn {
namespace sig {

using f64::kThreads;
using f64::kMaxBlocks;
using f64::kMaxWidth;
using f64::kGridCap;
using f64::kMaxTileRows;
using f64::kTensors;
using f64::kLdsSmall;
using f64::kLdsMax;

// true when the structural sign has to be flipped: the blades (bitmaps a, b) share an odd number of generators of `neg`.
// sign(i, k): a = bitmap[i], b = bitmap[k]; qsign(d): a = b = bitmap[d].
__host__ __device__ inline bool sig_flip(unsigned a, unsigned b, unsigned neg) {
    unsigned v = a & b & neg;   // at most 5 bits
    v ^= v >> 4; v ^= v >> 2; v ^= v >> 1;
    return (v & 1u) != 0;
}

// bytes of the per-workgroup sign table (sign [D * D], qsign [D]), a multiple of 16
constexpr size_t table_bytes(int D) { return (size_t)((D * D + D + 15) / 16 * 16); }

template <class Real>
struct Blk {
    int I, O, sub;
    const Real *W1, *b1, *sa, *sb, *w, *an, *WR, *WL, *bL, *la;
    long slice_off, act_off;   // as f64::Blk, in elements
};

template <class Real>
struct Seg {   // f64::Seg
    const Real *a, *b;
    const int *ia, *ib, *deg, *gi;
    Real* g;
    int ch, off;
    long a_rows;
};

template <class Real>
struct Args {   // f64::Args, and the signature
    Blk<Real> blk[kMaxBlocks];
    Seg<Real> seg[3];
    int nblk, nseg, R, maxO, resid_bwd;
    unsigned neg;
    long rows, tiles, gy_rows;
    Real* y;
    const Real* resid;
    const Real* gy;
    const int* gy_idx;
    Real* ws;
    long wg_elems, slice_elems, act_elems, g_elems;
};

// elements of LDS per tile row: f64::lds_row_doubles
inline long lds_row_elems(int maxO, int D, int G) { return f64::lds_row_doubles(maxO, D, G); }

template <int N>
struct Tab {
    f64::Tab<Alg<N, 0u>> t;            // structure: out, sgn and qs of the all-positive signature, paths, grades
    unsigned char bm[1 << N];          // blade index -> bitmap
};

template <int N>
constexpr Tab<N> make_tab() {
    Tab<N> s{};
    s.t = f64::make_tab<Alg<N, 0u>>();
    for (int d = 0; d < (1 << N); ++d) s.bm[d] = (unsigned char)Alg<N, 0u>::t.bo.bitmap[d];
    return s;
}

template <int N>
__constant__ const Tab<N> g_tab = make_tab<N>();

template <class Real> struct Const;
template <> struct Const<double> { static constexpr double tiny = 1e-16, eps = 1e-6; };
template <> struct Const<float> { static constexpr float tiny = 1e-16f, eps = 1e-6f; };

template <class Real> __device__ __forceinline__ Real sigmoid(Real x) { return Real(1) / (Real(1) + exp(-x)); }
template <class Real> __device__ __forceinline__ Real smooth_abs_sqrt(Real q) { return sqrt(sqrt(q * q + Const<Real>::tiny)); }

template <class Real>
struct Lds {   // f64::Lds, and the expanded signs
    Real *Y, *Z, *RR, *S, *GGP, *GZ, *GR, *gate, *invden, *uu, *gpre, *ganc, *qs, *nl, *dot, *invMn, *gMn;
    const signed char *sgn, *qsgn;
    __device__ Lds(Real* p, int R, int maxO, int D, int G) {
        const long t = (long)R * maxO * D, c = (long)R * maxO * G, o = (long)R * maxO;
        Y = p; Z = Y + t; RR = Z + t; S = RR + t; GGP = S + t; GZ = GGP + t; GR = GZ + t;
        gate = GR + t; invden = gate + c; uu = invden + c; gpre = uu + c; ganc = gpre + c;
        qs = ganc + c; nl = qs + o; dot = nl + o; invMn = dot + o; gMn = invMn + R;
        sgn = reinterpret_cast<const signed char*>(gMn + R);
        qsgn = sgn + D * D;
    }
};

template <int N, class Real>
__device__ void block_forward(const Blk<Real>& B, int nr, const Real* __restrict__ x, Real* __restrict__ dst,
                              const Real* __restrict__ resid, const Lds<Real>& l) {
    using A = Alg<N, 0u>;
    constexpr int D = A::D, G = A::G, P = A::P;
    const f64::Tab<A>& T = g_tab<N>.t;
    constexpr Real kEps = Const<Real>::eps, kInvSqrt2 = Real(0.70710678118654752440);
    const int tid = threadIdx.x, I = B.I, O = B.O, OD = O * D, OG = O * G;
    for (int e = tid; e < nr * OD; e += kThreads) {            // MVLinear
        const int r = e / OD, f = e - r * OD, o = f / D, d = f - o * D, g = T.grade[d];
        Real acc = (d == 0 && B.b1) ? B.b1[o] : Real(0);
        const Real* xr = x + (long)r * I * D + d;
        const Real* w = B.sub ? B.W1 + (long)o * I * G + g : B.W1 + (long)o * I;
        const int wst = B.sub ? G : 1;
        for (int i = 0; i < I; ++i) acc += w[(long)i * wst] * xr[(long)i * D];
        l.Y[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // MVSiLU
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const Real* y = l.Y + r * OD + o * D;
        Real* z = l.Z + r * OD + o * D;
        Real u = Real(0);
        if (g == 0) u = y[0];
        else for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) u += Real(l.qsgn[d]) * y[d] * y[d];
        const Real gt = sigmoid<Real>(B.sa[o * G + g] * u + B.sb[o * G + g]);
        l.gate[e] = gt; l.uu[e] = u;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) z[d] = gt * y[d];
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // linear_right, linear_left (into S)
        const int r = e / OD, f = e - r * OD, o = f / D, d = f - o * D, g = T.grade[d];
        Real ar = Real(0), al = (d == 0) ? B.bL[o] : Real(0);
        const Real* z = l.Z + r * OD + d;
        const Real *wr = B.WR + (long)o * O * G + g, *wl = B.WL + (long)o * O * G + g;
        for (int i = 0; i < O; ++i) { ar += wr[i * G] * z[i * D]; al += wl[i * G] * z[i * D]; }
        l.RR[e] = ar; l.S[e] = al;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // NormalizationLayer
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const Real* R = l.RR + r * OD + o * D;
        Real qq = Real(0);
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) qq += Real(l.qsgn[d]) * R[d] * R[d];
        const Real m = sigmoid<Real>(B.an[o * G + g]) * (smooth_abs_sqrt<Real>(qq) - Real(1)) + Real(1);
        l.invden[e] = Real(1) / (m + kEps);
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // geometric product: blade j of the output, left blades ascending
        const int r = e / OD, f = e - r * OD, o = f / D, j = f - o * D;
        const Real *z = l.Z + r * OD + o * D, *R = l.RR + r * OD + o * D, *inv = l.invden + r * OG + o * G, *w = B.w + (long)o * P;
        Real acc = l.S[e];
        for (int i = 0; i < D; ++i) {
            const int k = T.out[i * D + j], q = i * D + k;
            acc += Real(l.sgn[q]) * w[T.pid[q]] * z[i] * (R[k] * inv[T.grade[k]]);
        }
        l.S[e] = acc * kInvSqrt2;
    }
    __syncthreads();
    for (int e = tid; e < nr * O; e += kThreads) {             // MVLayerNorm
        const Real* s = l.S + (long)e * D;
        Real qs = Real(0);
        for (int d = 0; d < D; ++d) qs += Real(l.qsgn[d]) * s[d] * s[d];
        l.qs[e] = qs; l.nl[e] = smooth_abs_sqrt<Real>(qs);
    }
    __syncthreads();
    if (tid < nr) {
        Real nsum = Real(0);
        for (int o = 0; o < O; ++o) nsum += l.nl[tid * O + o];
        l.invMn[tid] = Real(1) / (nsum / Real(O) + kEps);
    }
    __syncthreads();
    if (dst)
        for (int e = tid; e < nr * OD; e += kThreads) {
            const int r = e / OD, o = (e - r * OD) / D;
            Real v = B.la[o] * l.S[e] * l.invMn[r];
            if (resid) v += resid[e];
            dst[e] = v;
        }
    __syncthreads();
}

template <int N, class Real>
__device__ void block_backward(const Blk<Real>& B, int nr, const Real* __restrict__ x, const Real* __restrict__ gout,
                               Real* __restrict__ gx, Real* __restrict__ slice, const Lds<Real>& l) {
    using A = Alg<N, 0u>;
    constexpr int D = A::D, G = A::G, P = A::P;
    const f64::Tab<A>& T = g_tab<N>.t;
    constexpr Real kInvSqrt2 = Real(0.70710678118654752440);
    const int tid = threadIdx.x, I = B.I, O = B.O, OD = O * D, OG = O * G;
    for (int e = tid; e < nr * O; e += kThreads) {             // MVLayerNorm
        Real dt = Real(0);
        for (int d = 0; d < D; ++d) dt += gout[(long)e * D + d] * l.S[(long)e * D + d];
        l.dot[e] = dt;
    }
    __syncthreads();
    if (tid < nr) {
        Real gm = Real(0);
        for (int o = 0; o < O; ++o) gm -= B.la[o] * l.dot[tid * O + o];
        l.gMn[tid] = gm * (l.invMn[tid] * l.invMn[tid] / Real(O));
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {
        const int r = e / OD, f = e - r * OD, o = f / D, d = f - o * D;
        const Real inl = Real(1) / l.nl[r * O + o];
        const Real gqs = l.gMn[r] * Real(0.5) * l.qs[r * O + o] * inl * inl * inl;
        l.GGP[e] = (B.la[o] * gout[e] * l.invMn[r] + gqs * Real(2) * Real(l.qsgn[d]) * l.S[e]) * kInvSqrt2;
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // linear_left and the geometric product: gz, gr
        const int r = e / OD, f = e - r * OD, c = f / D, b = f - c * D, g = T.grade[b];
        const Real *ggp = l.GGP + r * OD, *z = l.Z + r * OD + c * D, *R = l.RR + r * OD + c * D, *inv = l.invden + r * OG + c * G;
        const Real* w = B.w + (long)c * P;
        Real gz = Real(0), gr = Real(0);
        for (int o = 0; o < O; ++o) gz += B.WL[((long)o * O + c) * G + g] * ggp[o * D + b];
        for (int k = 0; k < D; ++k) {                          // b as the left blade i
            const int q = b * D + k, j = T.out[q];
            gz += w[T.pid[q]] * (Real(l.sgn[q]) * ggp[c * D + j]) * (R[k] * inv[T.grade[k]]);
        }
        for (int i = 0; i < D; ++i) {                          // b as the right blade k
            const int q = i * D + b, j = T.out[q];
            gr += w[T.pid[q]] * (Real(l.sgn[q]) * ggp[c * D + j]) * z[i];
        }
        l.GZ[e] = gz; l.GR[e] = gr;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // NormalizationLayer: gr -> gR in place
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const Real* R = l.RR + r * OD + o * D;
        Real* gr = l.GR + r * OD + o * D;
        Real gden = Real(0), qR = Real(0);
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) { gden -= gr[d] * R[d]; qR += Real(l.qsgn[d]) * R[d] * R[d]; }
        const Real inv = l.invden[e];
        gden *= inv * inv;
        const Real nu = smooth_abs_sqrt<Real>(qR), sg = sigmoid<Real>(B.an[o * G + g]);
        l.ganc[e] = gden * (nu - Real(1)) * sg * (Real(1) - sg);
        const Real gq = gden * sg * Real(0.5) * qR / (nu * nu * nu);
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) gr[d] = gr[d] * inv + gq * Real(2) * Real(l.qsgn[d]) * R[d];
    }
    __syncthreads();
    for (int e = tid; e < nr * OD; e += kThreads) {            // linear_right
        const int r = e / OD, f = e - r * OD, c = f / D, d = f - c * D, g = T.grade[d];
        Real gz = l.GZ[e];
        for (int o = 0; o < O; ++o) gz += B.WR[((long)o * O + c) * G + g] * l.GR[r * OD + o * D + d];
        l.GZ[e] = gz;
    }
    __syncthreads();
    for (int e = tid; e < nr * OG; e += kThreads) {            // MVSiLU: gz -> gy in place
        const int r = e / OG, f = e - r * OG, o = f / G, g = f - o * G;
        const Real* y = l.Y + r * OD + o * D;
        Real* gz = l.GZ + r * OD + o * D;
        Real ggate = Real(0);
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d) ggate += gz[d] * y[d];
        const Real gt = l.gate[e], gpre = ggate * gt * (Real(1) - gt), gu = gpre * B.sa[o * G + g];
        l.gpre[e] = gpre;
        for (int d = T.gstart[g]; d < T.gstart[g + 1]; ++d)
            gz[d] = gz[d] * gt + (g == 0 ? gu : gu * Real(2) * Real(l.qsgn[d]) * y[d]);
    }
    __syncthreads();
    if (gx)
        for (int e = tid; e < nr * I * D; e += kThreads) {     // MVLinear: d/dx
            const int r = e / (I * D), f = e - r * I * D, i = f / D, d = f - i * D, g = T.grade[d];
            const Real* gy = l.GZ + r * OD + d;
            Real acc = Real(0);
            for (int o = 0; o < O; ++o) acc += (B.sub ? B.W1[((long)o * I + i) * G + g] : B.W1[(long)o * I + i]) * gy[o * D];
            gx[e] = acc;
        }
    // parameter gradients, slice layout: W1 | b1 | sa | sb | w | an | WR | WL | bL | la
    const long nW1 = (long)O * I * (B.sub ? G : 1), oOG = OG, nw = (long)O * P, nOO = (long)O * O * G;
    const long o_b1 = nW1, o_sa = o_b1 + O, o_sb = o_sa + oOG, o_w = o_sb + oOG, o_an = o_w + nw, o_WR = o_an + oOG, o_WL = o_WR + nOO,
               o_bL = o_WL + nOO, o_la = o_bL + O, total = o_la + O;
    for (long e = tid; e < total; e += kThreads) {
        Real acc = slice[e];
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
                const Real *ggp = l.GGP + r * OD + o * D, *z = l.Z + r * OD + o * D, *R = l.RR + r * OD + o * D,
                           *inv = l.invden + r * OG + o * G;
                for (int q = T.pstart[p]; q < T.pstart[p + 1]; ++q) {
                    const int i = T.pi[q], k = T.pk[q], ik = i * D + k;
                    acc += Real(l.sgn[ik]) * ggp[T.out[ik]] * z[i] * (R[k] * inv[T.grade[k]]);
                }
            }
        } else if (e < o_WR) {
            const int f = int(e - o_an);
            for (int r = 0; r < nr; ++r) acc += l.ganc[r * OG + f];
        } else if (e < o_bL) {
            const bool left = e >= o_WL;
            const long f = e - (left ? o_WL : o_WR);
            const int g = int(f % G), o = int(f / G / O), i = int(f / G - (long)o * O);
            const Real* gsrc = left ? l.GGP : l.GR;
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

template <int N, class Real, bool BWD>
__global__ __launch_bounds__(kThreads) void cemlp_sig_kernel(const Args<Real> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sig_lds[];
    constexpr int D = 1 << N, G = N + 1;
    const int tid = threadIdx.x;
    const Lds<Real> l(reinterpret_cast<Real*>(sig_lds), a.R, a.maxO, D, G);
    {   // the signature, expanded once: sign [D * D] | qsign [D]
        const Tab<N>& S = g_tab<N>;
        signed char* tab = const_cast<signed char*>(l.sgn);
        for (int q = tid; q < D * D + D; q += kThreads) {
            if (q < D * D) {
                const int i = q / D, k = q - i * D;
                const signed char s = S.t.sgn[q];
                tab[q] = sig_flip(S.bm[i], S.bm[k], a.neg) ? (signed char)-s : s;
            } else {
                const int d = q - D * D;
                const signed char s = S.t.qs[d];
                tab[q] = sig_flip(S.bm[d], S.bm[d], a.neg) ? (signed char)-s : s;
            }
        }
    }
    Real* slice = a.ws + (long)blockIdx.x * a.wg_elems;
    Real* act = slice + a.slice_elems;
    Real* gbuf[2] = {act + a.act_elems, act + a.act_elems + a.g_elems};
    if (BWD)
        for (long e = tid; e < a.slice_elems; e += kThreads) slice[e] = Real(0);
    __syncthreads();
    const int I0 = a.blk[0].I, OL = a.blk[a.nblk - 1].O;
    for (long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const long r0 = t * a.R;
        const int nr = int(a.rows - r0 < a.R ? a.rows - r0 : a.R);
        for (int e = tid; e < nr * I0 * D; e += kThreads) {    // the input rows of block 0
            const int r = e / (I0 * D), f = e - r * I0 * D, c = f / D, d = f - c * D;
            const int s = (a.nseg > 2 && c >= a.seg[2].off) ? 2 : ((a.nseg > 1 && c >= a.seg[1].off) ? 1 : 0);
            const Seg<Real>& sg = a.seg[s];
            const long row = r0 + r, col = (long)(c - sg.off) * D + d, w = (long)sg.ch * D;
            Real v = sg.a[f64::clamp_row(sg.ia ? sg.ia[row] : row, sg.a_rows) * w + col];
            if (sg.b) v -= sg.b[f64::clamp_row(sg.ib[row], sg.a_rows) * w + col];
            if (sg.deg) { const int dg = sg.deg[row]; v *= Real(1) / Real(dg > 1 ? dg : 1); }
            act[e] = v;
        }
        __syncthreads();
        for (int k = 0; k < a.nblk; ++k) {
            const bool last = k + 1 == a.nblk;
            Real* dst = last ? (BWD ? nullptr : a.y + r0 * OL * D) : act + a.blk[k + 1].act_off;
            block_forward<N, Real>(a.blk[k], nr, act + a.blk[k].act_off, dst, (last && !BWD && a.resid) ? a.resid + r0 * OL * D : nullptr, l);
        }
        if (BWD) {
            for (int e = tid; e < nr * OL * D; e += kThreads) {
                const long row = r0 + e / (OL * D);
                gbuf[0][e] = a.gy[f64::clamp_row(a.gy_idx ? a.gy_idx[row] : row, a.gy_rows) * OL * D + e % (OL * D)];
            }
            __syncthreads();
            int cur = 0;
            for (int k = a.nblk - 1; k >= 0; --k) {
                const Real* xk = act + a.blk[k].act_off;
                if (k + 1 != a.nblk) block_forward<N, Real>(a.blk[k], nr, xk, nullptr, nullptr, l);   // the last block's state is still there
                block_backward<N, Real>(a.blk[k], nr, xk, gbuf[cur], gbuf[cur ^ 1], slice + a.blk[k].slice_off, l);
                cur ^= 1;
            }
            const Real* gx = gbuf[cur];
            for (int e = tid; e < nr * I0 * D; e += kThreads) {
                const int r = e / (I0 * D), f = e - r * I0 * D, c = f / D, d = f - c * D;
                const int s = (a.nseg > 2 && c >= a.seg[2].off) ? 2 : ((a.nseg > 1 && c >= a.seg[1].off) ? 1 : 0);
                const Seg<Real>& sg = a.seg[s];
                if (!sg.g) continue;
                const long row = r0 + r, col = (long)(c - sg.off) * D + d, w = (long)sg.ch * D;
                Real v = gx[e];
                if (sg.deg) { const int dg = sg.deg[row]; v *= Real(1) / Real(dg > 1 ? dg : 1); }
                if (s == 0 && a.resid_bwd) v += a.gy[row * OL * D + col];
                sg.g[(sg.gi ? f64::clamp_row(sg.gi[row], a.rows) : row) * w + col] = v;
            }
            __syncthreads();
        }
    }
}

// host side (sig.hip), shared with f64.hip
bool parse_signature(const float* metric, int n, unsigned& neg);   // n in 2..5 and every entry exactly +1 or -1: the mask
bool force_sig();                                                  // CSMPN_FORCE_SIG=1, read once per process
hipError_t launch_f64(int n, unsigned neg, bool bwd, unsigned grid, size_t lds_rows, hipStream_t st, const f64::Args& a);

}  // namespace sig
}  // namespace csmpn
