// Device helpers shared by the kernel families (ONE copy each; every family header includes this file, directly or through
// the header it builds on): the in-place kernel-argument access, the 16-byte load / store, and - for the families that keep a
// whole multivector in a lane (cemlp_pg.hpp: 32 blades, cemlp_pq.hpp: 8) - the path-weighted geometric product with its
// two-pass backward and the 16-row butterfly with its collector.
// Everything is a CSMPN_DEV template whose loops are resolved at compile time: sharing changes no device instruction.
#pragma once
#include "cemlp_device.hpp"

namespace csmpn {

// First statement of a kernel `(const DevCemlp C_arg, const RowIO io_arg)`: CD and `io` are references to the descriptors IN
// the kernarg segment (constant address space, scalar loads). Indexing the by-value arguments dynamically (C_arg.b[k]) makes
// the compiler copy the whole struct to scratch and turns every field access into a scratch load.
#define CSMPN_KERNEL_ARGS(CD)                                                                                       \
    typedef const char __attribute__((address_space(4))) * KArgPtr;                                                 \
    const KArgPtr ka = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();                                             \
    constexpr size_t kIoOffset = (sizeof(DevCemlp) + alignof(RowIO) - 1) / alignof(RowIO) * alignof(RowIO);         \
    const DevCemlp& CD = *(const DevCemlp*)(const char*)ka;                                                         \
    const RowIO& io = *(const RowIO*)(const char*)(ka + kIoOffset);                                                 \
    (void)C_arg; (void)io_arg

CSMPN_DEV f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
CSMPN_DEV void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }

// ---------------------------------------------------------------------------------
// all D blades of a multivector in the lane's registers (float t[D])
//
// out[j] += sum_p w[p] sum_{(i,k) -> j in path p} sign(i,k) z[i] r[k]   (cegnn_utils.py:126-152), in-lane, no exchange;
// wrow: this channel's P path weights (LDS, 16-byte aligned)
// (cemlp_cl.hpp keeps cl_weighted_gp: it fetches all path weights before the first term, another instruction order)
template <class ALG>
CSMPN_DEV void lane_weighted_gp(float (&out)[ALG::D], const float (&z)[ALG::D], const float (&r)[ALG::D], const float* wrow) {
    constexpr int P = ALG::P;
    static_assert(P % 4 == 0, "whole 16-byte pieces of path weights");
    static_for<0, P / 4>([&](auto qq) {
        const f4 wv = ld4(wrow + 4 * decltype(qq)::value);
        static_for<0, 4>([&](auto pp) {
            constexpr int p = 4 * decltype(qq)::value + decltype(pp)::value;
            constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
            constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
            constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
            constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
            const float w = wv[decltype(pp)::value];
            float tmp[nj];
#pragma unroll
            for (int t = 0; t < nj; ++t) tmp[t] = 0.f;
            static_for<0, ni>([&](auto ii) {
                static_for<0, nk>([&](auto kk) {
                    constexpr int i = i0 + ii, k = k0 + kk;
                    constexpr int j = ALG::t.out[i][k];
                    if constexpr (j >= j0 && j < j0 + nj) {
                        constexpr float sg = float(ALG::t.sign[i][k]);
                        tmp[j - j0] = __builtin_fmaf(sg * z[i], r[k], tmp[j - j0]);
                    }
                });
            });
#pragma unroll
            for (int t = 0; t < nj; ++t) out[j0 + t] = __builtin_fmaf(w, tmp[t], out[j0 + t]);
        });
    });
}

// 16 values in, lane j of the 16-lane DPP row keeps the sum over the row's lanes of value j (cb_rows_sum of cemlp_cmb.hpp)
CSMPN_DEV float rows16_sum(float (&x)[16], int l16) {
    const bool b0 = l16 & 1, b1 = l16 & 2, b2 = l16 & 4, b3 = l16 & 8;
    float y[8], z[4], u[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float keep = b0 ? x[2 * j + 1] : x[2 * j], send = b0 ? x[2 * j] : x[2 * j + 1];
        y[j] = keep + dpp_mov<0xB1>(send);   // quad_perm [1,0,3,2]
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float keep = b1 ? y[2 * j + 1] : y[2 * j], send = b1 ? y[2 * j] : y[2 * j + 1];
        z[j] = keep + dpp_mov<0x4E>(send);   // quad_perm [2,3,0,1]
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float keep = b2 ? z[2 * j + 1] : z[2 * j], send = b2 ? z[2 * j] : z[2 * j + 1];
        u[j] = keep + dpp_mov<0x124>(send);  // row_ror 4
    }
    const float keep = b3 ? u[1] : u[0], send = b3 ? u[0] : u[1];
    return keep + dpp_mov<0x128>(send);      // row_ror 8
}
// collects the per-channel gradients of a tile in slot order and runs a butterfly whenever 16 are there (NS groups of 16 slots)
template <int NS>
struct RowsCollect {
    float buf[16];
    template <int IDX>
    CSMPN_DEV void add(float v, float (&small)[NS], int l16) {
        buf[IDX % 16] = v;
        if constexpr (IDX % 16 == 15) small[IDX / 16] += rows16_sum(buf, l16);
    }
};

// geometric product backward, two passes (each keeps four tensors live):
//   Z: gz[i] += w_p U[i], gw_p = sum_i z[i] U[i],  U[i] = sum sign ggp[j] r[k];   R: gr[k] = sum_p w_p sum sign ggp[j] z[i]
template <class ALG, int NS>
CSMPN_DEV void lane_gp_bwd_z(const float (&ggp)[ALG::D], const float (&z)[ALG::D], const float (&rf)[ALG::D], float (&gz)[ALG::D],
                             const float* wrow, RowsCollect<NS>& col, float (&small)[NS], int l16) {
    constexpr int P = ALG::P;
    static_for<0, P / 4>([&](auto qq) {
        const f4 wv = ld4(wrow + 4 * decltype(qq)::value);
        static_for<0, 4>([&](auto pp) {
            constexpr int p = 4 * decltype(qq)::value + decltype(pp)::value;
            constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
            constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
            constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
            constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
            const float w = wv[decltype(pp)::value];
            float U[ni];
#pragma unroll
            for (int t = 0; t < ni; ++t) U[t] = 0.f;
            static_for<0, ni>([&](auto ii) {
                static_for<0, nk>([&](auto kk) {
                    constexpr int i = i0 + ii, k = k0 + kk;
                    constexpr int j = ALG::t.out[i][k];
                    if constexpr (j >= j0 && j < j0 + nj) {
                        constexpr float sg = float(ALG::t.sign[i][k]);
                        U[ii] = __builtin_fmaf(sg * ggp[j], rf[k], U[ii]);
                    }
                });
            });
            float gwv = 0.f;
#pragma unroll
            for (int t = 0; t < ni; ++t) { gz[i0 + t] = __builtin_fmaf(w, U[t], gz[i0 + t]); gwv = __builtin_fmaf(z[i0 + t], U[t], gwv); }
            col.template add<p>(gwv, small, l16);
        });
    });
}
template <class ALG>
CSMPN_DEV void lane_gp_bwd_r(const float (&ggp)[ALG::D], const float (&z)[ALG::D], float (&gr)[ALG::D], const float* wrow) {
    constexpr int P = ALG::P;
    static_for<0, P / 4>([&](auto qq) {
        const f4 wv = ld4(wrow + 4 * decltype(qq)::value);
        static_for<0, 4>([&](auto pp) {
            constexpr int p = 4 * decltype(qq)::value + decltype(pp)::value;
            constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
            constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
            constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
            constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
            const float w = wv[decltype(pp)::value];
            float V[nk];
#pragma unroll
            for (int t = 0; t < nk; ++t) V[t] = 0.f;
            static_for<0, ni>([&](auto ii) {
                static_for<0, nk>([&](auto kk) {
                    constexpr int i = i0 + ii, k = k0 + kk;
                    constexpr int j = ALG::t.out[i][k];
                    if constexpr (j >= j0 && j < j0 + nj) {
                        constexpr float sg = float(ALG::t.sign[i][k]);
                        V[kk] = __builtin_fmaf(sg * ggp[j], z[i], V[kk]);
                    }
                });
            });
#pragma unroll
            for (int t = 0; t < nk; ++t) gr[k0 + t] = __builtin_fmaf(w, V[t], gr[k0 + t]);
        });
    });
}

// The thread id through an empty asm statement, once per phase of the 16-row backward kernels: derived from the same value in
// every phase, the LDS addresses of all phases (hundreds: the XOR swizzle makes every (row, piece) pair its own value) are
// loop invariants that the compiler computes once and keeps alive across the tile loop - 370 spills per tile.
CSMPN_DEV int fenced_tid() { int t = threadIdx.x; asm volatile("" : "+v"(t)); return t; }

}  // namespace csmpn
