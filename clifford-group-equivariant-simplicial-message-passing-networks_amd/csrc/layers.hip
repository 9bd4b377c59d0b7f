// Standalone forms of the small Clifford layers (C-ABI in include/csmpn_hip.h):
//   csmpn_mvsilu_forward / _backward        MVSiLU, invariant "mag2"          cegnn_utils.py:53-83
//   csmpn_mvnorm_forward / _backward        NormalizationLayer                cegnn_utils.py:34-51
//   csmpn_mvlayernorm_forward / _backward   MVLayerNorm                       cegnn_utils.py:86-96
//   csmpn_wgp_forward / _backward           the path-weighted geometric product of
//                                           SteerableGeometricProductLayer    cegnn_utils.py:126-152
//   csmpn_mvlinear_forward / _backward      MVLinear                          cegnn_utils.py:287-338
// Inside a CEMLP these steps are fused into the row programs (cemlp_*.hpp); no reference model calls
// the layers on their own, so these kernels are the plain HBM-bound form: one thread per (row,
// channel) with the channel's D blades in registers (compile-time sign tables, algebra.hpp), rows of a
// workgroup contiguous in memory. Parameter gradients: per-workgroup sums in LDS, then one float
// atomic per parameter and workgroup. The csmpn_*_det forms of the four small layers use no float
// atomic: contributions parked in LDS and added in a fixed order, one partial row per workgroup in
// the caller's scratch, a second launch that adds the partial rows (see "_det forms" below).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/csmpn_hip.h"
#include "algebra.hpp"
#include "capi_common.hpp"

namespace {
using namespace csmpn;

constexpr float kEps = 1e-6f;       // cegnn_utils.py:5
constexpr float kSmooth = 1e-16f;   // cliffordalgebra.py:148
constexpr int kThreads = 256;
constexpr int kMaxChannels = 256;   // per-workgroup LDS sums: C * (parameters per channel) floats

__device__ __forceinline__ float sigmoid_sat(float x) { return 1.0f / (1.0f + __expf(-fmaxf(x, -87.0f))); }
__device__ __forceinline__ float smooth_abs_sqrt(float q) { return sqrtf(sqrtf(q * q + kSmooth)); }

template <class ALG, int d>
constexpr float qsf = float(ALG::t.qsign[d]);

template <class ALG>
__device__ __forceinline__ void load_row(float (&x)[ALG::D], const float* p) {
    constexpr int D = ALG::D;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
        const float4 v = *reinterpret_cast<const float4*>(p + d);
        x[d] = v.x; x[d + 1] = v.y; x[d + 2] = v.z; x[d + 3] = v.w;
    }
}
template <class ALG>
__device__ __forceinline__ void store_row(const float (&x)[ALG::D], float* p) {
    constexpr int D = ALG::D;
#pragma unroll
    for (int d = 0; d < D; d += 4) *reinterpret_cast<float4*>(p + d) = make_float4(x[d], x[d + 1], x[d + 2], x[d + 3]);
}
// q_g = sum over the blades of grade g of qsign[d] x_d^2 (cliffordalgebra.py:119-146)
template <class ALG>
__device__ __forceinline__ void grade_q(const float (&x)[ALG::D], float (&q)[ALG::G]) {
    static_for<0, ALG::G>([&](auto g) {
        float s = 0.f;
        static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) { s += qsf<ALG, d> * x[d] * x[d]; });
        q[g] = s;
    });
}

// per-workgroup parameter-gradient sums: acc[c * NP + k] in LDS, flushed with one atomic per entry
struct ParamSums {
    float* lds;
    __device__ void zero(int n) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) lds[i] = 0.f;
        __syncthreads();
    }
    __device__ void add(int i, float v) { atomicAdd(lds + i, v); }
};

// ---------------------------------------------------------------------------------- MVSiLU
template <class ALG, bool BWD>
__global__ void __launch_bounds__(kThreads) mvsilu_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                          const float* __restrict__ b, const float* __restrict__ gy, long rows,
                                                          int C, float* __restrict__ out, float* __restrict__ ga,
                                                          float* __restrict__ gb) {
    constexpr int D = ALG::D, G = ALG::G;
    extern __shared__ float smem[];
    ParamSums ps{smem};
    if constexpr (BWD) ps.zero(2 * G * C);
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t < rows * C) {
        const int c = (int)(t % C);
        float xv[D], u[G], gate[G];
        load_row<ALG>(xv, x + t * D);
        grade_q<ALG>(xv, u);
        u[0] = xv[0];
#pragma unroll
        for (int g = 0; g < G; ++g) gate[g] = sigmoid_sat(a[c * G + g] * u[g] + b[c * G + g]);
        if constexpr (!BWD) {
            float y[D];
            static_for<0, D>([&](auto d) { y[d] = gate[ALG::grade(d)] * xv[d]; });
            store_row<ALG>(y, out + t * D);
        } else {
            float gv[D], gx[D];
            load_row<ALG>(gv, gy + t * D);
            static_for<0, G>([&](auto g) {
                float gg = 0.f;
                static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) { gg += gv[d] * xv[d]; });
                const float gpre = gg * gate[g] * (1.0f - gate[g]);
                ps.add(c * 2 * G + g, gpre * u[g]);
                ps.add(c * 2 * G + G + g, gpre);
                const float gu = gpre * a[c * G + g];
                static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) {
                    gx[d] = gv[d] * gate[g] + (g == 0 ? gu : gu * (2.0f * qsf<ALG, d>) * xv[d]);
                });
            });
            store_row<ALG>(gx, out + t * D);
        }
    }
    if constexpr (BWD) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * G * C; i += kThreads) {
            const int c = i / (2 * G), k = i % (2 * G);
            const float v = smem[i];
            if (v != 0.f) atomicAdd((k < G ? ga : gb) + c * G + (k % G), v);
        }
    }
}

// ---------------------------------------------------------------------------------- NormalizationLayer
template <class ALG, bool BWD>
__global__ void __launch_bounds__(kThreads) mvnorm_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                          const float* __restrict__ gy, long rows, int C,
                                                          float* __restrict__ out, float* __restrict__ ga) {
    constexpr int D = ALG::D, G = ALG::G;
    extern __shared__ float smem[];
    ParamSums ps{smem};
    if constexpr (BWD) ps.zero(G * C);
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t < rows * C) {
        const int c = (int)(t % C);
        float xv[D], q[G], inv[G], sg[G], nu[G];
        load_row<ALG>(xv, x + t * D);
        grade_q<ALG>(xv, q);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            sg[g] = sigmoid_sat(a[c * G + g]);
            nu[g] = smooth_abs_sqrt(q[g]);
            inv[g] = 1.0f / (sg[g] * (nu[g] - 1.0f) + 1.0f + kEps);
        }
        if constexpr (!BWD) {
            float y[D];
            static_for<0, D>([&](auto d) { y[d] = xv[d] * inv[ALG::grade(d)]; });
            store_row<ALG>(y, out + t * D);
        } else {
            float gv[D], gx[D];
            load_row<ALG>(gv, gy + t * D);
            static_for<0, G>([&](auto g) {
                float dot = 0.f;
                static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) { dot += gv[d] * xv[d]; });
                const float gden = -dot * inv[g] * inv[g];
                ps.add(c * G + g, gden * (nu[g] - 1.0f) * sg[g] * (1.0f - sg[g]));
                const float inu = 1.0f / nu[g];
                const float gq = gden * sg[g] * (0.5f * q[g]) * (inu * inu * inu);   // d nu / d q = q / (2 nu^3)
                static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) {
                    gx[d] = gv[d] * inv[g] + gq * (2.0f * qsf<ALG, d>) * xv[d];
                });
            });
            store_row<ALG>(gx, out + t * D);
        }
    }
    if constexpr (BWD) {
        __syncthreads();
        for (int i = threadIdx.x; i < G * C; i += kThreads) {
            const float v = smem[i];
            if (v != 0.f) atomicAdd(ga + i, v);
        }
    }
}

// ---------------------------------------------------------------------------------- MVLayerNorm
// A workgroup covers kThreads / C whole rows (thread = (local row, channel)); the mean over the
// channels of a row goes through LDS.
template <class ALG, bool BWD>
__global__ void __launch_bounds__(kThreads) mvlayernorm_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                               const float* __restrict__ gy, long rows, int C,
                                                               float* __restrict__ out, float* __restrict__ ga) {
    constexpr int D = ALG::D;
    extern __shared__ float smem[];
    const int rpb = kThreads / C;                 // rows per workgroup
    float* rsum = smem;                           // [rpb] sum of the channel norms
    float* rdot = smem + rpb;                     // [rpb] sum_c a_c <gy_c, x_c>   (backward)
    float* psum = smem + 2 * rpb;                 // [C]   parameter-gradient sums (backward)
    for (int i = threadIdx.x; i < 2 * rpb + C; i += kThreads) smem[i] = 0.f;
    __syncthreads();
    const int lr = threadIdx.x / C, c = threadIdx.x % C;
    const long row = (long)blockIdx.x * rpb + lr;
    const bool act = lr < rpb && row < rows;
    float xv[D], gv[D];
    float q = 0.f, nl = 0.f, dot = 0.f, ac = 0.f;
    if (act) {
        ac = a[c];
        load_row<ALG>(xv, x + (row * C + c) * D);
        static_for<0, D>([&](auto d) { q += qsf<ALG, d> * xv[d] * xv[d]; });
        nl = smooth_abs_sqrt(q);
        atomicAdd(rsum + lr, nl);
        if constexpr (BWD) {
            load_row<ALG>(gv, gy + (row * C + c) * D);
            static_for<0, D>([&](auto d) { dot += gv[d] * xv[d]; });
            atomicAdd(rdot + lr, ac * dot);
        }
    }
    __syncthreads();
    if (act) {
        const float invM = 1.0f / (rsum[lr] / float(C) + kEps);
        if constexpr (!BWD) {
            float y[D];
            static_for<0, D>([&](auto d) { y[d] = ac * xv[d] * invM; });
            store_row<ALG>(y, out + (row * C + c) * D);
        } else {
            atomicAdd(psum + c, dot * invM);
            const float gM = -rdot[lr] * invM * invM / float(C);      // d/d(norm of one channel)
            const float inl = 1.0f / nl;
            const float gq = gM * (0.5f * q) * (inl * inl * inl);
            float gx[D];
            static_for<0, D>([&](auto d) { gx[d] = ac * gv[d] * invM + gq * (2.0f * qsf<ALG, d>) * xv[d]; });
            store_row<ALG>(gx, out + (row * C + c) * D);
        }
    }
    if constexpr (BWD) {
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += kThreads) {
            const float v = psum[i];
            if (v != 0.f) atomicAdd(ga + i, v);
        }
    }
}

// ---------------------------------------------------------------------------------- weighted product
//   out[j] = sum_{(i,k) -> j} sign(i,k) w[c][path(grade i, grade j, grade k)] z[i] r[k]
template <class ALG, bool BWD>
__global__ void __launch_bounds__(kThreads) wgp_kernel(const float* __restrict__ z, const float* __restrict__ r,
                                                       const float* __restrict__ w, const float* __restrict__ gy, long rows,
                                                       int C, float* __restrict__ out, float* __restrict__ gz,
                                                       float* __restrict__ gr, float* __restrict__ gw) {
    constexpr int D = ALG::D, P = ALG::P;
    extern __shared__ float smem[];
    ParamSums ps{smem};
    if constexpr (BWD) ps.zero(P * C);
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t < rows * C) {
        const int c = (int)(t % C);
        float zv[D], rv[D];
        load_row<ALG>(zv, z + t * D);
        load_row<ALG>(rv, r + t * D);
        if constexpr (!BWD) {
            float y[D];
#pragma unroll
            for (int d = 0; d < D; ++d) y[d] = 0.f;
            static_for<0, P>([&](auto p) {
                constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
                constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
                float tmp[nj];
#pragma unroll
                for (int u = 0; u < nj; ++u) tmp[u] = 0.f;
                static_for<ALG::gstart(gi), ALG::gstart(gi) + ALG::gsize(gi)>([&](auto i) {
                    static_for<ALG::gstart(gk), ALG::gstart(gk) + ALG::gsize(gk)>([&](auto k) {
                        constexpr int j = ALG::t.out[i][k];
                        if constexpr (j >= j0 && j < j0 + nj) tmp[j - j0] += float(ALG::t.sign[i][k]) * zv[i] * rv[k];
                    });
                });
                const float wp = w[c * P + p];
#pragma unroll
                for (int u = 0; u < nj; ++u) y[j0 + u] += wp * tmp[u];
            });
            store_row<ALG>(y, out + t * D);
        } else {
            float gv[D], gzv[D], grv[D];
            load_row<ALG>(gv, gy + t * D);
#pragma unroll
            for (int d = 0; d < D; ++d) { gzv[d] = 0.f; grv[d] = 0.f; }
            static_for<0, P>([&](auto p) {
                constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
                constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
                constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
                constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
                float U[ni], V[nk];   // unweighted d/dz, d/dr of this path
#pragma unroll
                for (int u = 0; u < ni; ++u) U[u] = 0.f;
#pragma unroll
                for (int u = 0; u < nk; ++u) V[u] = 0.f;
                static_for<0, ni>([&](auto ii) {
                    static_for<0, nk>([&](auto kk) {
                        constexpr int i = i0 + ii, k = k0 + kk;
                        constexpr int j = ALG::t.out[i][k];
                        if constexpr (j >= j0 && j < j0 + nj) {
                            const float sg = float(ALG::t.sign[i][k]) * gv[j];
                            U[ii] += sg * rv[k];
                            V[kk] += sg * zv[i];
                        }
                    });
                });
                const float wp = w[c * P + p];
                float gwp = 0.f;
#pragma unroll
                for (int u = 0; u < ni; ++u) { gzv[i0 + u] += wp * U[u]; gwp += zv[i0 + u] * U[u]; }
#pragma unroll
                for (int u = 0; u < nk; ++u) grv[k0 + u] += wp * V[u];
                ps.add(c * P + p, gwp);
            });
            store_row<ALG>(gzv, gz + t * D);
            store_row<ALG>(grv, gr + t * D);
        }
    }
    if constexpr (BWD) {
        __syncthreads();
        for (int i = threadIdx.x; i < P * C; i += kThreads) {
            const float v = smem[i];
            if (v != 0.f) atomicAdd(gw + i, v);
        }
    }
}

// ---------------------------------------------------------------------------------- dispatch
enum Op { OP_SILU = CSMPN_LAYER_MVSILU, OP_NORM = CSMPN_LAYER_MVNORM, OP_LNORM = CSMPN_LAYER_MVLAYERNORM, OP_WGP = CSMPN_LAYER_WGP };

struct Args {
    const float *x, *r, *p0, *p1, *gy;
    long rows;
    int C;
    float *out, *out2, *g0, *g1;
};

// ---------------------------------------------------------------------------------- _det forms (no float atomics)
// A tile is what one workgroup of the default form covers: kThreads consecutive (row, channel) elements, for MVLayerNorm
// floor(kThreads / C) whole rows. At most kDetMaxParts workgroups: workgroup w walks the tiles [w * tiles_per_wg,
// (w + 1) * tiles_per_wg) in ascending order and leaves ONE partial row of `entries` parameter-gradient sums in
// part[w][entry]; small_det_reduce_kernel adds the partial rows in ascending order into the gradients. Everything below
// follows from (op, n, rows, channels): det_shape().
constexpr long kDetMaxParts = 512;

// Where a lane's parameter-gradient contributions go: `add(k, v)` = contribution v of this lane to entry k of its channel,
// called exactly once per k, parks v in the lane's own LDS slot park[k][lane]. Row stride kThreads + 1, so that the threads
// that later walk different k at the same lane position hit different banks.
constexpr int kParkStride = kThreads + 1;
struct ParkSums {
    float* park;
    __device__ void add(int k, float v) { park[k * kParkStride + threadIdx.x] = v; }
};

// The backward of element t = (row, channel) of the three one-lane-per-element layers: the arithmetic of mvsilu_kernel /
// mvnorm_kernel / wgp_kernel<ALG, true>, statement for statement. Copies, not shared helpers: with one body behind both
// forms the default kernels compiled to other code (operand order, register allocation), and those stay as they are.
template <class ALG>
__device__ __forceinline__ void mvsilu_bwd_lane(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                                                const float* __restrict__ gy, long t, int C, float* __restrict__ out, ParkSums& ps) {
    constexpr int D = ALG::D, G = ALG::G;
    const int c = (int)(t % C);
    float xv[D], u[G], gate[G];
    load_row<ALG>(xv, x + t * D);
    grade_q<ALG>(xv, u);
    u[0] = xv[0];
#pragma unroll
    for (int g = 0; g < G; ++g) gate[g] = sigmoid_sat(a[c * G + g] * u[g] + b[c * G + g]);
    float gv[D], gx[D];
    load_row<ALG>(gv, gy + t * D);
    static_for<0, G>([&](auto g) {
        float gg = 0.f;
        static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) { gg += gv[d] * xv[d]; });
        const float gpre = gg * gate[g] * (1.0f - gate[g]);
        ps.add(g, gpre * u[g]);
        ps.add(G + g, gpre);
        const float gu = gpre * a[c * G + g];
        static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) {
            gx[d] = gv[d] * gate[g] + (g == 0 ? gu : gu * (2.0f * qsf<ALG, d>) * xv[d]);
        });
    });
    store_row<ALG>(gx, out + t * D);
}

template <class ALG>
__device__ __forceinline__ void mvnorm_bwd_lane(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ gy,
                                                long t, int C, float* __restrict__ out, ParkSums& ps) {
    constexpr int D = ALG::D, G = ALG::G;
    const int c = (int)(t % C);
    float xv[D], q[G], inv[G], sg[G], nu[G];
    load_row<ALG>(xv, x + t * D);
    grade_q<ALG>(xv, q);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        sg[g] = sigmoid_sat(a[c * G + g]);
        nu[g] = smooth_abs_sqrt(q[g]);
        inv[g] = 1.0f / (sg[g] * (nu[g] - 1.0f) + 1.0f + kEps);
    }
    float gv[D], gx[D];
    load_row<ALG>(gv, gy + t * D);
    static_for<0, G>([&](auto g) {
        float dot = 0.f;
        static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) { dot += gv[d] * xv[d]; });
        const float gden = -dot * inv[g] * inv[g];
        ps.add(g, gden * (nu[g] - 1.0f) * sg[g] * (1.0f - sg[g]));
        const float inu = 1.0f / nu[g];
        const float gq = gden * sg[g] * (0.5f * q[g]) * (inu * inu * inu);   // d nu / d q = q / (2 nu^3)
        static_for<ALG::gstart(g), ALG::gstart(g) + ALG::gsize(g)>([&](auto d) {
            gx[d] = gv[d] * inv[g] + gq * (2.0f * qsf<ALG, d>) * xv[d];
        });
    });
    store_row<ALG>(gx, out + t * D);
}

template <class ALG>
__device__ __forceinline__ void wgp_bwd_lane(const float* __restrict__ z, const float* __restrict__ r, const float* __restrict__ w,
                                             const float* __restrict__ gy, long t, int C, float* __restrict__ gz,
                                             float* __restrict__ gr, ParkSums& ps) {
    constexpr int D = ALG::D, P = ALG::P;
    const int c = (int)(t % C);
    float zv[D], rv[D], gv[D], gzv[D], grv[D];
    load_row<ALG>(zv, z + t * D);
    load_row<ALG>(rv, r + t * D);
    load_row<ALG>(gv, gy + t * D);
#pragma unroll
    for (int d = 0; d < D; ++d) { gzv[d] = 0.f; grv[d] = 0.f; }
    static_for<0, P>([&](auto p) {
        constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
        constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
        constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
        constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
        float U[ni], V[nk];   // unweighted d/dz, d/dr of this path
#pragma unroll
        for (int u = 0; u < ni; ++u) U[u] = 0.f;
#pragma unroll
        for (int u = 0; u < nk; ++u) V[u] = 0.f;
        static_for<0, ni>([&](auto ii) {
            static_for<0, nk>([&](auto kk) {
                constexpr int i = i0 + ii, k = k0 + kk;
                constexpr int j = ALG::t.out[i][k];
                if constexpr (j >= j0 && j < j0 + nj) {
                    const float sg = float(ALG::t.sign[i][k]) * gv[j];
                    U[ii] += sg * rv[k];
                    V[kk] += sg * zv[i];
                }
            });
        });
        const float wp = w[c * P + p];
        float gwp = 0.f;
#pragma unroll
        for (int u = 0; u < ni; ++u) { gzv[i0 + u] += wp * U[u]; gwp += zv[i0 + u] * U[u]; }
#pragma unroll
        for (int u = 0; u < nk; ++u) grv[k0 + u] += wp * V[u];
        ps.add(p, gwp);
    });
    store_row<ALG>(gzv, gz + t * D);
    store_row<ALG>(grv, gr + t * D);
}

struct DetShape {
    long tiles, tiles_per_wg, parts;   // parts = ceil(tiles / tiles_per_wg) <= min(tiles, kDetMaxParts)
    int entries;                       // parameter-gradient entries = floats of one partial row
};

constexpr int paths_of(int n) { return n == 2 ? Alg<2, 0u>::P : n == 3 ? Alg<3, 0u>::P : n == 4 ? Alg<4, 0u>::P : Alg<5, 0u>::P; }
static_assert(Alg<4, 0x8u>::P == Alg<4, 0u>::P && Alg<5, 0x10u>::P == Alg<5, 0u>::P, "the grade paths depend on n alone");
static_assert(sizeof(float) * Alg<5, 0u>::P * kParkStride <= 64 * 1024, "parked path-weight contributions exceed 64 KB of LDS");

inline bool det_shape(int op, int n, long rows, int C, DetShape& S) {
    if (n < 2 || n > 5 || rows <= 0 || C < 1 || C > kMaxChannels || rows > (1L << 40)) return false;
    const int G = n + 1;
    switch (op) {
        case OP_SILU: S.entries = 2 * G * C; break;
        case OP_NORM: S.entries = G * C; break;
        case OP_LNORM: S.entries = C; break;
        case OP_WGP: S.entries = paths_of(n) * C; break;
        default: return false;
    }
    const long per_tile = op == OP_LNORM ? kThreads / C : kThreads;   // rows, or elements
    const long units = op == OP_LNORM ? rows : rows * C;
    S.tiles = (units + per_tile - 1) / per_tile;
    S.tiles_per_wg = (S.tiles + kDetMaxParts - 1) / kDetMaxParts;
    S.parts = (S.tiles + S.tiles_per_wg - 1) / S.tiles_per_wg;
    return true;
}

// The three one-lane-per-element layers. After a tile's lanes have parked their contributions, thread i (i + kThreads, ...)
// owns entry i = c * NP + k and adds the slots of the lanes of channel c in ascending lane order; only lanes inside
// rows * C are visited, so a ragged tile's idle lanes park nothing and nothing of theirs is read. The sum of a tile is
// added to the workgroup's partial row in tile order (the row is written before it is read: the first tile stores).
template <class ALG, Op OP>
__global__ void __launch_bounds__(kThreads) elem_bwd_det_kernel(const Args A, long tiles, long tiles_per_wg, float* part) {
    constexpr int NP = OP == OP_SILU ? 2 * ALG::G : OP == OP_NORM ? ALG::G : ALG::P;
    __shared__ float park[NP * kParkStride];
    ParkSums ps{park};
    const int C = A.C, entries = NP * C;
    const long total = A.rows * C;
    float* const prow = part + (size_t)blockIdx.x * entries;
    const long tile0 = (long)blockIdx.x * tiles_per_wg;
    const long tile1 = tile0 + tiles_per_wg < tiles ? tile0 + tiles_per_wg : tiles;
    for (long tile = tile0; tile < tile1; ++tile) {
        const long base = tile * kThreads, t = base + threadIdx.x;
        if (t < total) {
            if constexpr (OP == OP_SILU) mvsilu_bwd_lane<ALG>(A.x, A.p0, A.p1, A.gy, t, C, A.out, ps);
            else if constexpr (OP == OP_NORM) mvnorm_bwd_lane<ALG>(A.x, A.p0, A.gy, t, C, A.out, ps);
            else wgp_bwd_lane<ALG>(A.x, A.r, A.p0, A.gy, t, C, A.out, A.out2, ps);
        }
        __syncthreads();
        const int nvalid = total - base < kThreads ? (int)(total - base) : kThreads;
        const int c0 = (int)(base % C);   // channel of the tile's lane 0
        for (int i = threadIdx.x; i < entries; i += kThreads) {
            const int c = i / NP, k = i % NP;
            float s = 0.f;
            for (int l = c >= c0 ? c - c0 : c - c0 + C; l < nvalid; l += C) s += park[k * kParkStride + l];
            prow[i] = tile == tile0 ? s : prow[i] + s;
        }
        __syncthreads();
    }
}

// MVLayerNorm, forward and backward: as mvlayernorm_kernel, but the lanes park their channel norm (and a_c <gy_c, x_c>) in
// LDS and the row's first lane adds them in ascending channel order; the backward's d/da contributions are parked the same
// way and thread c adds the tile's rows in ascending order, keeping the workgroup's sum over its tiles in a register.
// Forward: one tile per workgroup, part unused.
template <class ALG, bool BWD>
__global__ void __launch_bounds__(kThreads) mvlayernorm_det_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                                   const float* __restrict__ gy, long rows, int C,
                                                                   float* __restrict__ out, long tiles, long tiles_per_wg,
                                                                   float* __restrict__ part) {
    constexpr int D = ALG::D;
    __shared__ float pnorm[kThreads], pdot[kThreads], rsum[kThreads], rdot[kThreads];
    const int rpb = kThreads / C;                 // rows per tile
    const int lr = threadIdx.x / C, c = threadIdx.x % C;
    const long tile0 = (long)blockIdx.x * tiles_per_wg;
    const long tile1 = tile0 + tiles_per_wg < tiles ? tile0 + tiles_per_wg : tiles;
    float acc = 0.f;                              // thread c < C: d/da[c] over this workgroup's tiles
    for (long tile = tile0; tile < tile1; ++tile) {
        const long row = tile * rpb + lr;
        const bool act = lr < rpb && row < rows;
        float xv[D], gv[D];
        float q = 0.f, nl = 0.f, dot = 0.f, ac = 0.f;
        if (act) {
            ac = a[c];
            load_row<ALG>(xv, x + (row * C + c) * D);
            static_for<0, D>([&](auto d) { q += qsf<ALG, d> * xv[d] * xv[d]; });
            nl = smooth_abs_sqrt(q);
            pnorm[threadIdx.x] = nl;
            if constexpr (BWD) {
                load_row<ALG>(gv, gy + (row * C + c) * D);
                static_for<0, D>([&](auto d) { dot += gv[d] * xv[d]; });
                pdot[threadIdx.x] = ac * dot;
            }
        }
        __syncthreads();
        if (act && c == 0) {
            float s = 0.f, sd = 0.f;
            for (int j = 0; j < C; ++j) s += pnorm[threadIdx.x + j];
            rsum[lr] = s;
            if constexpr (BWD) {
                for (int j = 0; j < C; ++j) sd += pdot[threadIdx.x + j];
                rdot[lr] = sd;
            }
        }
        __syncthreads();
        if (act) {
            const float invM = 1.0f / (rsum[lr] / float(C) + kEps);
            if constexpr (!BWD) {
                float y[D];
                static_for<0, D>([&](auto d) { y[d] = ac * xv[d] * invM; });
                store_row<ALG>(y, out + (row * C + c) * D);
            } else {
                pnorm[threadIdx.x] = dot * invM;                          // every read of the norms lies before the barrier above
                const float gM = -rdot[lr] * invM * invM / float(C);      // d/d(norm of one channel)
                const float inl = 1.0f / nl;
                const float gq = gM * (0.5f * q) * (inl * inl * inl);
                float gx[D];
                static_for<0, D>([&](auto d) { gx[d] = ac * gv[d] * invM + gq * (2.0f * qsf<ALG, d>) * xv[d]; });
                store_row<ALG>(gx, out + (row * C + c) * D);
            }
        }
        if constexpr (BWD) {
            __syncthreads();
            if (threadIdx.x < C) {
                const long left = rows - tile * rpb;
                const int nr = left < rpb ? (int)left : rpb;              // rows of this tile: only their slots were written
                float s = 0.f;
                for (int j = 0; j < nr; ++j) s += pnorm[j * C + threadIdx.x];
                acc += s;
            }
            __syncthreads();
        }
    }
    if constexpr (BWD)
        if (threadIdx.x < C) part[(size_t)blockIdx.x * C + threadIdx.x] = acc;
}

// g += the partial rows in ascending order: one thread per entry, eight rows in flight. silu_G != 0: MVSiLU's entries
// c * 2G + k go to g0 (a) for k < G and to g1 (b) behind; every other layer's entry i is g0[i].
__global__ void __launch_bounds__(kThreads) small_det_reduce_kernel(const float* __restrict__ part, int parts, int entries, int silu_G,
                                                                    float* g0, float* g1) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= entries) return;
    float s = 0.f;
    int w = 0;
    for (; w + 8 <= parts; w += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(w + j) * entries + i];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; w < parts; ++w) s += part[(size_t)w * entries + i];
    float* dst = g0 + i;
    if (silu_G) {
        const int c = i / (2 * silu_G), k = i % (2 * silu_G);
        dst = (k < silu_G ? g0 : g1) + c * silu_G + k % silu_G;
    }
    *dst += s;
}

template <class ALG, bool BWD>
hipError_t launch_det(Op op, const Args& A, const DetShape& S, float* part, hipStream_t st) {
    const dim3 grid((unsigned)S.parts), block(kThreads);
    if constexpr (!BWD) {   // MVLayerNorm forward, the only forward with a sum across lanes
        hipLaunchKernelGGL((mvlayernorm_det_kernel<ALG, false>), dim3((unsigned)S.tiles), block, 0, st, A.x, A.p0, A.gy, A.rows, A.C,
                           A.out, S.tiles, 1L, (float*)nullptr);
        return hipGetLastError();
    } else {
        switch (op) {
            case OP_SILU: hipLaunchKernelGGL((elem_bwd_det_kernel<ALG, OP_SILU>), grid, block, 0, st, A, S.tiles, S.tiles_per_wg, part); break;
            case OP_NORM: hipLaunchKernelGGL((elem_bwd_det_kernel<ALG, OP_NORM>), grid, block, 0, st, A, S.tiles, S.tiles_per_wg, part); break;
            case OP_WGP: hipLaunchKernelGGL((elem_bwd_det_kernel<ALG, OP_WGP>), grid, block, 0, st, A, S.tiles, S.tiles_per_wg, part); break;
            case OP_LNORM:
                hipLaunchKernelGGL((mvlayernorm_det_kernel<ALG, true>), grid, block, 0, st, A.x, A.p0, A.gy, A.rows, A.C, A.out,
                                   S.tiles, S.tiles_per_wg, part);
                break;
        }
        hipLaunchKernelGGL(small_det_reduce_kernel, dim3((unsigned)((S.entries + kThreads - 1) / kThreads)), block, 0, st,
                           (const float*)part, (int)S.parts, S.entries, op == OP_SILU ? ALG::G : 0, A.g0, A.g1);
        return hipGetLastError();
    }
}

template <class ALG, bool BWD>
hipError_t launch(Op op, const Args& A, hipStream_t st) {
    constexpr int G = ALG::G, P = ALG::P;
    const long n = A.rows * A.C;
    const unsigned grid = (unsigned)((n + kThreads - 1) / kThreads);
    switch (op) {
        case OP_SILU:
            hipLaunchKernelGGL((mvsilu_kernel<ALG, BWD>), dim3(grid), dim3(kThreads), BWD ? sizeof(float) * 2 * G * A.C : 0, st, A.x,
                               A.p0, A.p1, A.gy, A.rows, A.C, A.out, A.g0, A.g1);
            break;
        case OP_NORM:
            hipLaunchKernelGGL((mvnorm_kernel<ALG, BWD>), dim3(grid), dim3(kThreads), BWD ? sizeof(float) * G * A.C : 0, st, A.x, A.p0,
                               A.gy, A.rows, A.C, A.out, A.g0);
            break;
        case OP_LNORM: {
            const int rpb = kThreads / A.C;
            hipLaunchKernelGGL((mvlayernorm_kernel<ALG, BWD>), dim3((unsigned)((A.rows + rpb - 1) / rpb)), dim3(kThreads),
                               sizeof(float) * (2 * rpb + A.C), st, A.x, A.p0, A.gy, A.rows, A.C, A.out, A.g0);
            break;
        }
        case OP_WGP:
            hipLaunchKernelGGL((wgp_kernel<ALG, BWD>), dim3(grid), dim3(kThreads), BWD ? sizeof(float) * P * A.C : 0, st, A.x, A.r, A.p0,
                               A.gy, A.rows, A.C, A.out, A.out, A.out2, A.g0);
            break;
    }
    return hipGetLastError();
}

// det: the _det form of (op, bwd); `workspace` holds its partial rows (backward only).
int run(const float* metric, int n, Op op, bool bwd, const Args& A, void* stream, bool det = false, void* workspace = nullptr,
        size_t workspace_bytes = 0) {
    if (!metric || n < 2 || n > 5) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "standalone layers: n=%d not in 2..5", n);
    unsigned neg = 0;
    for (int i = 0; i < n; ++i) {
        if (metric[i] == -1.0f) neg |= 1u << i;
        else if (metric[i] != 1.0f) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "standalone layers: metric entries must be +-1");
    }
    if (A.rows < 0 || A.C < 1 || A.C > kMaxChannels) return csmpn_fail(CSMPN_ERR_INVALID, "standalone layers: bad rows / channels (1..%d)", kMaxChannels);
    if (A.rows == 0) return CSMPN_OK;
    DetShape S{};
    if (det) {
        if (!det_shape(op, n, A.rows, A.C, S)) return csmpn_fail(CSMPN_ERR_INVALID, "standalone layers (_det): rows=%ld out of range", A.rows);
        const size_t need = csmpn_small_layer_det_bytes(op, n, A.rows, A.C);
        if (bwd && (!workspace || workspace_bytes < need))
            return csmpn_fail(CSMPN_ERR_INVALID, "standalone layers (_det): workspace %zu bytes < %zu (csmpn_small_layer_det_bytes)",
                              workspace ? workspace_bytes : (size_t)0, need);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipErrorInvalidValue;
#define CSMPN_LAYER_ALG(N_, NEG_)                                                                                       \
    if (n == N_ && neg == NEG_) {                                                                                       \
        using A_ = Alg<N_, NEG_>;                                                                                       \
        if (det) e = bwd ? launch_det<A_, true>(op, A, S, (float*)workspace, st) : launch_det<A_, false>(op, A, S, nullptr, st); \
        else e = bwd ? launch<A_, true>(op, A, st) : launch<A_, false>(op, A, st);                                      \
    } else
    CSMPN_LAYER_ALG(2, 0u) CSMPN_LAYER_ALG(3, 0u) CSMPN_LAYER_ALG(4, 0u) CSMPN_LAYER_ALG(4, 0x8u) CSMPN_LAYER_ALG(5, 0u)
    CSMPN_LAYER_ALG(5, 0x10u)
        return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "standalone layers: no kernels for this signature (n=%d, negative mask 0x%x)", n, neg);
#undef CSMPN_LAYER_ALG
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "standalone layer launch: %s", hipGetErrorString(e));
    return CSMPN_OK;
}

// ----------------------------------------------------------------------------- standalone MVLinear
// (cegnn_utils.py:287-338) for callers outside a CEMLP (projection heads, feature embeddings):
//   y[b,o,d] = sum_i W[o,i,grade(d)] x[b,i,d]  (+ bias[o] on blade 0);  W [O,I,G] or [O,I].
// HBM-bound ([rows, I, D] in, [rows, O, D] out); one thread per output element, blade index
// fastest so that a wave reads / writes whole rows; the grade table depends on n only.
struct MvLinDesc {
    const float *x, *w, *b, *gy;
    float *y, *gx, *gw, *gb;
    long rows;
    int I, O, D, G, sub;
    unsigned char grade[32];
};

__global__ void mvlinear_fwd_kernel(const MvLinDesc P) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = P.rows * P.O * P.D;
    if (e >= total) return;
    const int d = (int)(e % P.D);
    const int o = (int)((e / P.D) % P.O);
    const long r = e / ((long)P.D * P.O);
    const int g = P.sub ? P.grade[d] : 0, ws = P.sub ? P.G : 1;
    const float* xr = P.x + r * P.I * P.D + d;
    const float* wr = P.w + (long)o * P.I * ws + g;
    float acc = (P.b && d == 0) ? P.b[o] : 0.f;
    for (int i = 0; i < P.I; ++i) acc = fmaf(wr[i * ws], xr[(long)i * P.D], acc);
    P.y[e] = acc;
}

// d/dx[b,i,d] = sum_o gy[b,o,d] W[o,i,grade(d)]
__global__ void mvlinear_bwd_x_kernel(const MvLinDesc P) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = P.rows * P.I * P.D;
    if (e >= total) return;
    const int d = (int)(e % P.D);
    const int i = (int)((e / P.D) % P.I);
    const long r = e / ((long)P.D * P.I);
    const int g = P.sub ? P.grade[d] : 0, ws = P.sub ? P.G : 1;
    const float* gr = P.gy + r * P.O * P.D + d;
    const float* wc = P.w + (long)i * ws + g;
    float acc = 0.f;
    for (int o = 0; o < P.O; ++o) acc = fmaf(wc[(long)o * P.I * ws], gr[(long)o * P.D], acc);
    P.gx[e] = acc;
}

// d/dW[o,i,g] += sum_{rows, d in g} gy[b,o,d] x[b,i,d];  d/dbias[o] += sum_rows gy[b,o,0].
// Thread = one weight (or bias) element, blockIdx.y = a slab of rows it walks (x / gy rows of a slab are L1 / L2 hits:
// a wave's 64 elements share o or neighbour it); one atomic per element and slab. The slab is sized so that the launch
// has ~512 workgroups (8..64 rows): the first version gave every workgroup ALL elements of a 4-row slab - 235 workgroups x 1 152
// atomics onto the same 1 152 addresses took 28 us on the 940 rows of an md17 batch.
inline int mvlinear_slab(long rows, int elem_blocks) {
    long slabs = 512 / elem_blocks;
    if (slabs < 1) slabs = 1;
    long s = (rows + slabs - 1) / slabs;
    return (int)(s < 8 ? 8 : (s > 64 ? 64 : s));
}
// DET (csmpn_mvlinear_backward_det): the slab's sum is stored to partials[slab][element] instead of added with an atomic;
// mvlinear_det_reduce_kernel adds the slabs in ascending order. The walk over a slab's rows is the same in both forms.
template <bool DET>
__global__ void mvlinear_bwd_w_kernel(const MvLinDesc P, int slab, float* __restrict__ partials) {
    const long r0 = (long)blockIdx.y * slab;
    const long r1 = r0 + slab < P.rows ? r0 + slab : P.rows;
    const int ws = P.sub ? P.G : 1;
    const int nw = P.O * P.I * ws;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nw + P.O) return;
    float acc = 0.f;
    if (e < nw) {
        if (!P.gw) return;
        const int g = e % ws, i = (e / ws) % P.I, o = e / (ws * P.I);
        // blades of grade g are contiguous (blade order: by grade): [d0, d1)
        int d0 = 0, d1 = P.D;
        if (P.sub) {
            while (P.grade[d0] != g) ++d0;
            d1 = d0;
            while (d1 < P.D && P.grade[d1] == g) ++d1;
        }
        for (long r = r0; r < r1; ++r) {
            const float* gr = P.gy + (r * P.O + o) * P.D;
            const float* xr = P.x + (r * P.I + i) * P.D;
            for (int d = d0; d < d1; ++d) acc = fmaf(gr[d], xr[d], acc);
        }
        if constexpr (DET) partials[(size_t)blockIdx.y * (nw + P.O) + e] = acc;
        else atomicAdd(P.gw + e, acc);
    } else if (P.gb) {
        const int o = e - nw;
        for (long r = r0; r < r1; ++r) acc += P.gy[(r * P.O + o) * P.D];
        if constexpr (DET) partials[(size_t)blockIdx.y * (nw + P.O) + e] = acc;
        else atomicAdd(P.gb + o, acc);
    }
}

// Deterministic form: at most kMvDetMaxSlabs slabs (the scratch is kMvDetMaxSlabs * (weight + bias elements) floats at
// most, whatever the row count: 2.4 MB for md17's 35 -> 32 feature embedding); slab size and count follow from the call's
// sizes alone, so that two processes on the same inputs add in the same order.
constexpr long kMvDetMaxSlabs = 512;
inline int mvlinear_det_slab(long rows, int elem_blocks) {
    long s = mvlinear_slab(rows, elem_blocks);
    const long floor_rows = (rows + kMvDetMaxSlabs - 1) / kMvDetMaxSlabs;
    if (s < floor_rows) s = floor_rows;
    return (int)s;
}
// an upper bound of the slab count that does not shrink as the rows grow (the count itself wobbles where the slab widens)
inline long mvlinear_det_slab_bound(long rows) {
    const long s = (rows + 7) / 8;
    return s < kMvDetMaxSlabs ? s : kMvDetMaxSlabs;
}
// g_weight / g_bias += the slabs' partial sums in ascending slab order: one thread per element (consecutive threads read
// consecutive words of a slab's row), eight slabs in flight. Elements without a destination were never written: skipped.
__global__ void __launch_bounds__(256) mvlinear_det_reduce_kernel(const float* __restrict__ partials, int nslabs, int nw, int O,
                                                                  float* gw, float* gb) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = nw + O;
    if (e >= total) return;
    float* const dst = e < nw ? (gw ? gw + e : nullptr) : (gb ? gb + (e - nw) : nullptr);
    if (!dst) return;
    float s = 0.f;
    int w = 0;
    for (; w + 8 <= nslabs; w += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = partials[(size_t)(w + i) * total + e];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; w < nslabs; ++w) s += partials[(size_t)w * total + e];
    *dst += s;
}

int mvlinear_desc(int n, long rows, int I, int O, int sub, MvLinDesc& P) {
    if (n < 1 || n > 5) return csmpn_fail(CSMPN_ERR_UNSUPPORTED, "MVLinear: n=%d not in 1..5", n);
    if (I < 1 || O < 1 || rows < 0) return csmpn_fail(CSMPN_ERR_INVALID, "MVLinear: bad sizes rows=%ld I=%d O=%d", rows, I, O);
    memset(&P, 0, sizeof(P));
    P.rows = rows; P.I = I; P.O = O; P.D = 1 << n; P.G = n + 1; P.sub = sub ? 1 : 0;
    // blade order: by grade, then lexicographic (metric.py:18-29): the grade of index d is the
    // grade whose cumulative binomial range contains d
    int d = 0, c = 1;   // c = C(n, g)
    for (int g = 0; g <= n; ++g) {
        for (int k = 0; k < c; ++k) P.grade[d++] = (unsigned char)g;
        c = c * (n - g) / (g + 1);
    }
    return CSMPN_OK;
}

}  // namespace

extern "C" {

int csmpn_mvsilu_forward(const float* metric_host, int n, const float* x, const float* a, const float* b, int64_t rows,
                         int32_t channels, float* y, void* stream) {
    if (!x || !a || !b || !y) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvsilu_forward: null pointer");
    Args A{x, nullptr, a, b, nullptr, (long)rows, channels, y, nullptr, nullptr, nullptr};
    return run(metric_host, n, OP_SILU, false, A, stream);
}
int csmpn_mvsilu_backward(const float* metric_host, int n, const float* x, const float* a, const float* b, const float* gy,
                          int64_t rows, int32_t channels, float* gx, float* g_a, float* g_b, void* stream) {
    if (!x || !a || !b || !gy || !gx || !g_a || !g_b) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvsilu_backward: null pointer");
    Args A{x, nullptr, a, b, gy, (long)rows, channels, gx, nullptr, g_a, g_b};
    return run(metric_host, n, OP_SILU, true, A, stream);
}
int csmpn_mvnorm_forward(const float* metric_host, int n, const float* x, const float* a, int64_t rows, int32_t channels,
                         float* y, void* stream) {
    if (!x || !a || !y) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvnorm_forward: null pointer");
    Args A{x, nullptr, a, nullptr, nullptr, (long)rows, channels, y, nullptr, nullptr, nullptr};
    return run(metric_host, n, OP_NORM, false, A, stream);
}
int csmpn_mvnorm_backward(const float* metric_host, int n, const float* x, const float* a, const float* gy, int64_t rows,
                          int32_t channels, float* gx, float* g_a, void* stream) {
    if (!x || !a || !gy || !gx || !g_a) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvnorm_backward: null pointer");
    Args A{x, nullptr, a, nullptr, gy, (long)rows, channels, gx, nullptr, g_a, nullptr};
    return run(metric_host, n, OP_NORM, true, A, stream);
}
int csmpn_mvlayernorm_forward(const float* metric_host, int n, const float* x, const float* a, int64_t rows,
                              int32_t channels, float* y, void* stream) {
    if (!x || !a || !y) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvlayernorm_forward: null pointer");
    Args A{x, nullptr, a, nullptr, nullptr, (long)rows, channels, y, nullptr, nullptr, nullptr};
    return run(metric_host, n, OP_LNORM, false, A, stream);
}
int csmpn_mvlayernorm_backward(const float* metric_host, int n, const float* x, const float* a, const float* gy,
                               int64_t rows, int32_t channels, float* gx, float* g_a, void* stream) {
    if (!x || !a || !gy || !gx || !g_a) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvlayernorm_backward: null pointer");
    Args A{x, nullptr, a, nullptr, gy, (long)rows, channels, gx, nullptr, g_a, nullptr};
    return run(metric_host, n, OP_LNORM, true, A, stream);
}
int csmpn_wgp_forward(const float* metric_host, int n, const float* z, const float* r, const float* weight, int64_t rows,
                      int32_t channels, float* y, void* stream) {
    if (!z || !r || !weight || !y) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_wgp_forward: null pointer");
    Args A{z, r, weight, nullptr, nullptr, (long)rows, channels, y, nullptr, nullptr, nullptr};
    return run(metric_host, n, OP_WGP, false, A, stream);
}
int csmpn_wgp_backward(const float* metric_host, int n, const float* z, const float* r, const float* weight,
                       const float* gy, int64_t rows, int32_t channels, float* gz, float* gr, float* g_weight, void* stream) {
    if (!z || !r || !weight || !gy || !gz || !gr || !g_weight) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_wgp_backward: null pointer");
    Args A{z, r, weight, nullptr, gy, (long)rows, channels, gz, gr, g_weight, nullptr};
    return run(metric_host, n, OP_WGP, true, A, stream);
}

size_t csmpn_small_layer_det_bytes(int op, int n, int64_t rows, int32_t channels) {
    DetShape S;
    if (!det_shape(op, n, (long)rows, channels, S)) return 0;
    return (size_t)(S.tiles < kDetMaxParts ? S.tiles : kDetMaxParts) * S.entries * sizeof(float);
}
int csmpn_mvsilu_backward_det(const float* metric_host, int n, const float* x, const float* a, const float* b, const float* gy,
                              int64_t rows, int32_t channels, float* gx, float* g_a, float* g_b, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!x || !a || !b || !gy || !gx || !g_a || !g_b) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvsilu_backward_det: null pointer");
    Args A{x, nullptr, a, b, gy, (long)rows, channels, gx, nullptr, g_a, g_b};
    return run(metric_host, n, OP_SILU, true, A, stream, true, workspace, workspace_bytes);
}
int csmpn_mvnorm_backward_det(const float* metric_host, int n, const float* x, const float* a, const float* gy, int64_t rows,
                              int32_t channels, float* gx, float* g_a, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !a || !gy || !gx || !g_a) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvnorm_backward_det: null pointer");
    Args A{x, nullptr, a, nullptr, gy, (long)rows, channels, gx, nullptr, g_a, nullptr};
    return run(metric_host, n, OP_NORM, true, A, stream, true, workspace, workspace_bytes);
}
int csmpn_mvlayernorm_forward_det(const float* metric_host, int n, const float* x, const float* a, int64_t rows,
                                  int32_t channels, float* y, void* stream) {
    if (!x || !a || !y) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvlayernorm_forward_det: null pointer");
    Args A{x, nullptr, a, nullptr, nullptr, (long)rows, channels, y, nullptr, nullptr, nullptr};
    return run(metric_host, n, OP_LNORM, false, A, stream, true);
}
int csmpn_mvlayernorm_backward_det(const float* metric_host, int n, const float* x, const float* a, const float* gy,
                                   int64_t rows, int32_t channels, float* gx, float* g_a, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!x || !a || !gy || !gx || !g_a) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvlayernorm_backward_det: null pointer");
    Args A{x, nullptr, a, nullptr, gy, (long)rows, channels, gx, nullptr, g_a, nullptr};
    return run(metric_host, n, OP_LNORM, true, A, stream, true, workspace, workspace_bytes);
}
int csmpn_wgp_backward_det(const float* metric_host, int n, const float* z, const float* r, const float* weight, const float* gy,
                           int64_t rows, int32_t channels, float* gz, float* gr, float* g_weight, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!z || !r || !weight || !gy || !gz || !gr || !g_weight) return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_wgp_backward_det: null pointer");
    Args A{z, r, weight, nullptr, gy, (long)rows, channels, gz, gr, g_weight, nullptr};
    return run(metric_host, n, OP_WGP, true, A, stream, true, workspace, workspace_bytes);
}

int csmpn_mvlinear_forward(int n, const float* x, const float* weight, const float* bias, int64_t rows,
                           int32_t in_features, int32_t out_features, int32_t subspaces, float* y, void* stream) {
    MvLinDesc P;
    int rc = mvlinear_desc(n, (long)rows, in_features, out_features, subspaces, P);
    if (rc) return rc;
    if (rows == 0) return CSMPN_OK;
    if (!x || !weight || !y) return csmpn_fail(CSMPN_ERR_INVALID, "MVLinear: null pointer");
    P.x = x; P.w = weight; P.b = bias; P.y = y;
    const long total = (long)rows * out_features * P.D;
    const unsigned block = 256, grid = (unsigned)((total + block - 1) / block);
    hipLaunchKernelGGL(mvlinear_fwd_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "hipGetLastError(): %s", hipGetErrorString(e));
    return CSMPN_OK;
}

int csmpn_mvlinear_backward(int n, const float* x, const float* weight, const float* gy, int64_t rows,
                            int32_t in_features, int32_t out_features, int32_t subspaces, float* gx, float* g_weight,
                            float* g_bias, void* stream) {
    MvLinDesc P;
    int rc = mvlinear_desc(n, (long)rows, in_features, out_features, subspaces, P);
    if (rc) return rc;
    if (rows == 0) return CSMPN_OK;
    if (!x || !weight || !gy) return csmpn_fail(CSMPN_ERR_INVALID, "MVLinear: null pointer");
    P.x = x; P.w = weight; P.gy = gy; P.gx = gx; P.gw = g_weight; P.gb = g_bias;
    const unsigned block = 256;
    if (gx) {
        const long total = (long)rows * in_features * P.D;
        hipLaunchKernelGGL(mvlinear_bwd_x_kernel, dim3((unsigned)((total + block - 1) / block)), dim3(block), 0,
                           (hipStream_t)stream, P);
    }
    if (g_weight || g_bias) {   // the bias gradient comes from the same kernel: a frozen weight must not silence it
        const int nelem = out_features * in_features * (P.sub ? P.G : 1) + out_features;
        const unsigned eb = (unsigned)((nelem + block - 1) / block);
        const int slab = mvlinear_slab(rows, (int)eb);
        hipLaunchKernelGGL(mvlinear_bwd_w_kernel<false>, dim3(eb, (unsigned)((rows + slab - 1) / slab)), dim3(block), 0,
                           (hipStream_t)stream, P, slab, (float*)nullptr);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "hipGetLastError(): %s", hipGetErrorString(e));
    return CSMPN_OK;
}

size_t csmpn_mvlinear_backward_det_bytes(int n, int64_t rows, int32_t in_features, int32_t out_features, int32_t subspaces) {
    if (n < 1 || n > 5 || rows <= 0 || in_features < 1 || out_features < 1) return 0;
    const size_t nelem = (size_t)out_features * in_features * (subspaces ? n + 1 : 1) + out_features;
    if (nelem > 0x7fffffffu) return 0;
    return (size_t)mvlinear_det_slab_bound((long)rows) * nelem * sizeof(float);
}

int csmpn_mvlinear_backward_det(int n, const float* x, const float* weight, const float* gy, int64_t rows,
                                int32_t in_features, int32_t out_features, int32_t subspaces, float* gx, float* g_weight,
                                float* g_bias, void* workspace, size_t workspace_bytes, void* stream) {
    MvLinDesc P;
    int rc = mvlinear_desc(n, (long)rows, in_features, out_features, subspaces, P);
    if (rc) return rc;
    if (rows == 0) return CSMPN_OK;
    if (!x || !weight || !gy) return csmpn_fail(CSMPN_ERR_INVALID, "MVLinear: null pointer");
    P.x = x; P.w = weight; P.gy = gy; P.gx = gx; P.gw = g_weight; P.gb = g_bias;
    const unsigned block = 256;
    const size_t nelem = (size_t)out_features * in_features * (P.sub ? P.G : 1) + out_features;
    const size_t need = csmpn_mvlinear_backward_det_bytes(n, rows, in_features, out_features, subspaces);
    if (g_weight || g_bias) {
        if (nelem > 0x7fffffffu) return csmpn_fail(CSMPN_ERR_INVALID, "MVLinear: too many weight elements");
        if (!workspace || workspace_bytes < need)
            return csmpn_fail(CSMPN_ERR_INVALID, "csmpn_mvlinear_backward_det: workspace %zu bytes < %zu (csmpn_mvlinear_backward_det_bytes)",
                              workspace ? workspace_bytes : (size_t)0, need);
    }
    if (gx) {
        const long total = (long)rows * in_features * P.D;
        hipLaunchKernelGGL(mvlinear_bwd_x_kernel, dim3((unsigned)((total + block - 1) / block)), dim3(block), 0,
                           (hipStream_t)stream, P);
    }
    if (g_weight || g_bias) {
        const unsigned eb = (unsigned)((nelem + block - 1) / block);
        const int slab = mvlinear_det_slab(rows, (int)eb);
        const long nslabs = (rows + slab - 1) / slab;   // <= mvlinear_det_slab_bound(rows): slab >= 8 and >= rows / kMvDetMaxSlabs
        hipLaunchKernelGGL(mvlinear_bwd_w_kernel<true>, dim3(eb, (unsigned)nslabs), dim3(block), 0, (hipStream_t)stream, P, slab,
                           (float*)workspace);
        hipLaunchKernelGGL(mvlinear_det_reduce_kernel, dim3(eb), dim3(block), 0, (hipStream_t)stream, (const float*)workspace,
                           (int)nslabs, (int)(nelem - out_features), (int)out_features, g_weight, g_bias);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return csmpn_fail(CSMPN_ERR_HIP, "hipGetLastError(): %s", hipGetErrorString(e));
    return CSMPN_OK;
}


}  // extern "C"
