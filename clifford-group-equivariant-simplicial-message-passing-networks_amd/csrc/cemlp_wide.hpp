// Wide row-tile kernel: the general kernel's program (cemlp_kernel.hpp) for CEMLP blocks of 65..256 output channels.
//
// The general kernel gives every 16-channel tile of a row tile its own wave (MT = ceil(max O / 16) waves), and keeps the
// tile's whole block state in registers between the workgroup barriers of block_forward / block_backward. Its backward
// holds ~500 VGPRs, one wave per SIMD: 4 waves, 64 channels. Here the channel tiles are decoupled from the waves:
//   CT = ceil(max O / 16) channel tiles, MT = min(CT, 4 backward / 8 forward) waves; wave mt runs tiles mt, mt + MT, ...
// Every phase that needs all channels of the previous one (the MVLinear reads of the input tile, linear_left / right
// reading z, the cross-channel LayerNorm sum) already goes through a tile buffer, so each phase becomes a loop over the
// wave's channel tiles between the same barriers. What a tile's registers held from one phase to the next is parked in a
// region of the row tile, [slot][CT][D][64 lanes] f4 (one b128 per blade and lane, as park() / unpark()):
//   slot 0  y   (MVLinear output; the MVSiLU gates are recomputed from it)
//   slot 1  R   (linear_right output; the normalization denominators are recomputed from it), later d/dR, later d/dy
//   slot 2  s   (input of the layer norm), later d/dz
//   slot 3  d/d(block output) of the block below the last one (the transposed MVLinear of the block above)
// The forward parks s only (slot 0). The row tile (input / z / gradient tiles, LayerNorm scratch sized by CT, row indices,
// parking region) lives in LDS when it fits, else in the per-workgroup global scratch behind the packed weights (C.gtiles);
// the pointers are generic, so ONE instantiation per (algebra, mode, direction) serves both and every width. Weights come
// from the packed fragments (global), parameter gradients go to the global accumulators (or the workgroup's copy of them in
// deterministic mode: every gradient word has one writing wave, the owner of its channel tile).
#pragma once
#include "cemlp_kernel.hpp"

namespace csmpn {

constexpr int kWideSlotsFwd = 1, kWideSlotsBwd = 4;

// parking slot s of channel tile ct (CT tiles per slot)
template <class ALG>
CSMPN_DEV float* wide_slot(float* pk, int CT, int s, int ct) {
    return pk + (size_t)(s * CT + ct) * ALG::D * 256;
}

// inverse of store_tile: channel tile ct of a tile [channel][D][R] in lane layout (channels >= CP read as zero)
template <class ALG>
CSMPN_DEV void load_tile(f4 (&t)[ALG::D], const float* tile, int CP, int ct, const Geo<ALG, 1>& ge) {
    using GE = Geo<ALG, 1>;
    constexpr int D = ALG::D, R = GE::R, CS = GE::CS, NW = GE::NW;
    const int c = NW * ct + ge.cn;
    const float* p = tile + (c < CP ? c : 0) * CS + ge.r0;
#pragma unroll
    for (int d = 0; d < D; ++d) t[d] = c < CP ? *reinterpret_cast<const f4*>(p + d * R) : splat(0.f);
}

// MVSiLU gates of y (block_forward phase 2)
template <class ALG>
CSMPN_DEV void wide_gates(const LaneParams<ALG>& lp, const f4 (&y)[ALG::D], f4 (&gate)[ALG::G]) {
    static_for<0, ALG::G>([&](auto g) {
        constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
        f4 u;
        if constexpr (g == 0) {
            u = y[0];
        } else {
            u = splat(0.f);
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                u += qsf<ALG, d> * y[d] * y[d];
            });
        }
        gate[g] = sigmoid4(lp.sa[g] * u + lp.sb[g]);
    });
}

// 1 / (interpolated norm + eps) of the right operand R (block_forward phase 4)
template <class ALG>
CSMPN_DEV void wide_invden(const LaneParams<ALG>& lp, const f4 (&R)[ALG::D], f4 (&invden)[ALG::G]) {
    static_for<0, ALG::G>([&](auto g) {
        constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
        f4 qq = splat(0.f);
        static_for<0, nd>([&](auto t) {
            constexpr int d = d0 + decltype(t)::value;
            qq += qsf<ALG, d> * R[d] * R[d];
        });
        const f4 m = lp.sg[g] * (smooth_abs_sqrt4(qq) - 1.0f) + 1.0f;
        invden[g] = rcp4(m + kEps);
    });
}

// Phases 1-6 of block_forward for every channel tile of this wave, up to the layer-norm scale: s (input of the layer norm)
// of tile ct goes to parking slot PS, y / R to slots PY / PR when >= 0 (backward). Returns 1 / (mean norm + eps) of the
// lane's rows. Starts with the input tile complete (barrier behind the caller), ends with a barrier.
template <class ALG, bool SPEC>
CSMPN_DEV f4 wide_forward_state(const DevBlock& B, const float* xin, float* zbuf, float* red, float* pk, int CT, int MT,
                                int mt, const Geo<ALG, 1>& ge, int PY, int PR, int PS) {
    using GE = Geo<ALG, 1>;
    constexpr int D = ALG::D, G = ALG::G, NW = GE::NW;
    const WSrc sW1{B.pfW1, nullptr, B.O, B.CPi, B.w1_sub};
    const WSrc sWR{B.pfWR, nullptr, B.O, B.CPo, 1};
    const WSrc sWL{B.pfWL, nullptr, B.O, B.CPo, 1};
    // 1. MVLinear, 2. MVSiLU -> z tile
    for (int ct = mt; ct < B.NTo; ct += MT) {
        const LaneParams<ALG> lp = load_lane_params<ALG>(B, NW * ct + ge.cn);
        f4 y[D];
#pragma unroll
        for (int d = 0; d < D; ++d) y[d] = splat(0.f);
        linear_from_tile<ALG, 1, false, false, SPEC>(y, xin, B.CPi, B.KKi, sW1, ct, ge);
        y[0] += lp.b1;
        f4 gate[G], z[D];
        wide_gates<ALG>(lp, y, gate);
        static_for<0, G>([&](auto g) {
            constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
#pragma unroll
            for (int t = 0; t < nd; ++t) z[d0 + t] = gate[g] * y[d0 + t];
        });
        store_tile<ALG, 1>(z, zbuf, B.CPo, ct, ge);
        if (PY >= 0) park<ALG>(y, wide_slot<ALG>(pk, CT, PY, ct), ge.lane);
    }
    __syncthreads();
    // 3. linear_right / left, 4. normalization, 5. geometric product, 6. the row's channel-norm partial sums
    for (int ct = mt; ct < B.NTo; ct += MT) {
        const int c = NW * ct + ge.cn;
        const LaneParams<ALG> lp = load_lane_params<ALG>(B, c);
        f4 R[D], L[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { R[d] = splat(0.f); L[d] = splat(0.f); }
        linear_from_tile<ALG, 1, false, false, SPEC>(R, zbuf, B.CPo, B.KKo, sWR, ct, ge);
        linear_from_tile<ALG, 1, false, false, SPEC>(L, zbuf, B.CPo, B.KKo, sWL, ct, ge);
        L[0] += lp.bL;
        f4 invden[G], r[D];
        wide_invden<ALG>(lp, R, invden);
        static_for<0, G>([&](auto g) {
            constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
#pragma unroll
            for (int t = 0; t < nd; ++t) r[d0 + t] = R[d0 + t] * invden[g];
        });
        if (lp.cvalid) {
            f4 z[D];
            load_tile<ALG>(z, zbuf, B.CPo, ct, ge);
            weighted_gp<ALG>(L, z, r, B.w + (size_t)c * ALG::P);
        }
        f4 s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = L[d] * kInvSqrt2;
        park<ALG>(s, wide_slot<ALG>(pk, CT, PS, ct), ge.lane);
        if (PR >= 0) park<ALG>(R, wide_slot<ALG>(pk, CT, PR, ct), ge.lane);
        f4 qs = splat(0.f);
        static_for<0, D>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            qs += qsf<ALG, d> * s[d] * s[d];
        });
        const f4 tot = chan_sum4<1>(lp.cvalid ? smooth_abs_sqrt4(qs) : splat(0.f));
        if (ge.n == 0) *reinterpret_cast<f4*>(red + ct * 16 + 4 * ge.q) = tot;
    }
    __syncthreads();
    f4 tot = splat(0.f);
    for (int m = 0; m < B.NTo; ++m) tot += *reinterpret_cast<const f4*>(red + m * 16 + 4 * ge.q);
    __syncthreads();
    return rcp4(tot * (1.0f / float(B.O)) + kEps);
}

// d/d(block output) of channel tile ct: rows of gsrc ([rows, O, D]; gathered through gidx when given) or parking slot 3
template <class ALG>
CSMPN_DEV void wide_gout(f4 (&g)[ALG::D], const float* gsrc, const int* gidx, long row0, long rows, int O, float* pk,
                         int CT, int ct, const Geo<ALG, 1>& ge) {
    constexpr int D = ALG::D;
    if (!gsrc) {
        unpark<ALG>(g, wide_slot<ALG>(pk, CT, 3, ct), ge.lane);
        return;
    }
    const int c = 16 * ct + ge.cn;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const long grow = row0 + ge.r0 + v;
        const bool ok = grow < rows && c < O;
        long srow = grow;
        if (gidx && ok) srow = gidx[ge.r0 + v];
        const float* p = gsrc + (srow * O + c) * D;
#pragma unroll
        for (int d4 = 0; d4 < D; d4 += 4) {
            const f4 val = ok ? *reinterpret_cast<const f4*>(p + d4) : splat(0.f);
            g[d4][v] = val.x; g[d4 + 1][v] = val.y; g[d4 + 2][v] = val.z; g[d4 + 3][v] = val.w;
        }
    }
}

// Block backward over all channel tiles of this wave (block_backward, one loop per barrier interval), on the state that
// wide_forward_state parked in slots 0 (y), 1 (R), 2 (s) and the layer-norm scale invMn. Accumulates every parameter
// gradient and leaves d/d(MVLinear output) in the tile gbuf; ends with a barrier.
template <class ALG>
CSMPN_DEV void wide_block_backward(const DevBlock& B, const float* xin, const float* zbuf, float* gbuf, float* red, float* pk,
                                   int CT, int MT, int mt, const Geo<ALG, 1>& ge, f4 invMn, const float* gsrc, const int* gidx,
                                   long row0, long rows, size_t goff) {
    using GE = Geo<ALG, 1>;
    constexpr int D = ALG::D, G = ALG::G, P = ALG::P, NW = GE::NW;
    const WSrc sWRt{B.pbWR, nullptr, B.O, B.CPo, 1};
    const WSrc sWLt{B.pbWL, nullptr, B.O, B.CPo, 1};
    float *d_b1 = B.gb1 + goff, *d_sa = B.gsa + goff, *d_sb = B.gsb + goff, *d_w = B.gw + goff, *d_an = B.gan + goff;
    float *d_bL = B.gbL + goff, *d_la = B.gla + goff, *d_W1 = B.gW1 + goff, *d_WR = B.gWR + goff, *d_WL = B.gWL + goff;
    auto slot = [&](int s, int ct) { return wide_slot<ALG>(pk, CT, s, ct); };
    const bool lead = ge.q == 0;   // after channel_rows_sum every lane of a channel holds its sum: one of them adds it

    // ---- MVLayerNorm backward, 1: d/d(mean norm) of every row
    for (int ct = mt; ct < B.NTo; ct += MT) {
        const int c = NW * ct + ge.cn;
        const bool cv = c < B.O;
        const float la = cv ? B.la[c] : 0.f;
        f4 gout[D], s[D];
        wide_gout<ALG>(gout, gsrc, gidx, row0, rows, B.O, pk, CT, ct, ge);
        unpark<ALG>(s, slot(2, ct), ge.lane);
        f4 dot = splat(0.f);
#pragma unroll
        for (int d = 0; d < D; ++d) dot += gout[d] * s[d];
        const float p_la = channel_rows_sum<1>(hsum(dot * invMn));
        const f4 gMn = chan_sum4<1>(-(la * dot) * invMn * invMn);
        if (ge.n == 0) *reinterpret_cast<f4*>(red + ct * 16 + 4 * ge.q) = gMn;
        if (cv && lead) atomicAdd(d_la + c, p_la);
    }
    __syncthreads();
    f4 gMn = splat(0.f);
    for (int m = 0; m < B.NTo; ++m) gMn += *reinterpret_cast<const f4*>(red + m * 16 + 4 * ge.q);
    __syncthreads();
    // ---- 2: d/d(left) = d/d(gp) -> gbuf
    for (int ct = mt; ct < B.NTo; ct += MT) {
        const int c = NW * ct + ge.cn;
        const bool cv = c < B.O;
        const float la = cv ? B.la[c] : 0.f;
        f4 gout[D], s[D], ggp[D];
        wide_gout<ALG>(gout, gsrc, gidx, row0, rows, B.O, pk, CT, ct, ge);
        unpark<ALG>(s, slot(2, ct), ge.lane);
        f4 qs = splat(0.f);
        static_for<0, D>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            qs += qsf<ALG, d> * s[d] * s[d];
        });
        const f4 inl = rcp4(smooth_abs_sqrt4(qs));
        const f4 gqs = (gMn * (1.0f / float(B.O))) * (0.5f * qs) * (inl * inl * inl);
        static_for<0, D>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            const f4 gs = (la * gout[d]) * invMn + gqs * (2.0f * qsf<ALG, d>) * s[d];
            ggp[d] = cv ? gs * kInvSqrt2 : splat(0.f);
        });
        const float p_bL = channel_rows_sum<1>(hsum(ggp[0]));
        if (cv && lead) atomicAdd(d_bL + c, p_bL);
        store_tile<ALG, 1>(ggp, gbuf, B.CPo, ct, ge);
    }
    __syncthreads();
    // ---- linear_left backward, geometric product backward, NormalizationLayer backward
    for (int ct = mt; ct < B.NTo; ct += MT) {
        const int c = NW * ct + ge.cn;
        const LaneParams<ALG> lp = load_lane_params<ALG>(B, c);
        const bool cv = lp.cvalid;
        const int cc = cv ? c : 0;
        f4 ggp[D], gz[D];
        load_tile<ALG>(ggp, gbuf, B.CPo, ct, ge);
#pragma unroll
        for (int d = 0; d < D; ++d) gz[d] = splat(0.f);
        linear_from_tile<ALG, 1, false, true>(gz, gbuf, B.CPo, B.KKo, sWLt, ct, ge);
        weight_grad<ALG, 1, false>(ggp, zbuf, B.CPo, B.O, B.O, B.NTo, ct, ge, d_WL, true);
        f4 y[D], R[D], gate[G], invden[G];
        unpark<ALG>(y, slot(0, ct), ge.lane);
        unpark<ALG>(R, slot(1, ct), ge.lane);
        wide_gates<ALG>(lp, y, gate);
        wide_invden<ALG>(lp, R, invden);
        f4 gr[D];
        float p_w[P], p_an[G];
#pragma unroll
        for (int d = 0; d < D; ++d) gr[d] = splat(0.f);
        weighted_gp_bwd<ALG>(ggp, y, gate, R, invden, B.w + (size_t)cc * P, gz, gr, p_w);
        f4 gR[D];
        static_for<0, G>([&](auto g) {
            constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
            f4 gden = splat(0.f), qR = splat(0.f);
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                gden -= gr[d] * R[d];
                qR += qsf<ALG, d> * R[d] * R[d];
            });
            gden *= invden[g] * invden[g];
            const f4 nu = smooth_abs_sqrt4(qR);
            p_an[g] = hsum(gden * (nu - 1.0f)) * lp.sg[g] * (1.0f - lp.sg[g]);
            const f4 inu = rcp4(nu);
            const f4 gq = (gden * lp.sg[g]) * (0.5f * qR) * (inu * inu * inu);
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                gR[d] = cv ? gr[d] * invden[g] + gq * (2.0f * qsf<ALG, d>) * R[d] : splat(0.f);
            });
        });
#pragma unroll
        for (int p = 0; p < P; ++p) p_w[p] = channel_rows_sum<1>(p_w[p]);
#pragma unroll
        for (int g = 0; g < G; ++g) p_an[g] = channel_rows_sum<1>(p_an[g]);
        if (cv && lead) {
#pragma unroll
            for (int p = 0; p < P; ++p) atomicAdd(d_w + (size_t)c * P + p, p_w[p]);
#pragma unroll
            for (int g = 0; g < G; ++g) atomicAdd(d_an + c * G + g, p_an[g]);
        }
        park<ALG>(gz, slot(2, ct), ge.lane);
        park<ALG>(gR, slot(1, ct), ge.lane);
    }
    __syncthreads();   // all reads of gbuf (d/d(left)) done
    for (int ct = mt; ct < B.NTo; ct += MT) {
        f4 gR[D];
        unpark<ALG>(gR, slot(1, ct), ge.lane);
        store_tile<ALG, 1>(gR, gbuf, B.CPo, ct, ge);
    }
    __syncthreads();
    // ---- linear_right backward, MVSiLU backward -> d/dy
    for (int ct = mt; ct < B.NTo; ct += MT) {
        const int c = NW * ct + ge.cn;
        const LaneParams<ALG> lp = load_lane_params<ALG>(B, c);
        const bool cv = lp.cvalid;
        f4 gz[D], gR[D], y[D], gate[G], gy[D];
        unpark<ALG>(gz, slot(2, ct), ge.lane);
        unpark<ALG>(gR, slot(1, ct), ge.lane);
        linear_from_tile<ALG, 1, false, true>(gz, gbuf, B.CPo, B.KKo, sWRt, ct, ge);
        weight_grad<ALG, 1, false>(gR, zbuf, B.CPo, B.O, B.O, B.NTo, ct, ge, d_WR, true);
        unpark<ALG>(y, slot(0, ct), ge.lane);
        wide_gates<ALG>(lp, y, gate);
        float p_sa[G], p_sb[G];
        static_for<0, G>([&](auto g) {
            constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
            f4 ggate = splat(0.f);
#pragma unroll
            for (int t = 0; t < nd; ++t) ggate += gz[d0 + t] * y[d0 + t];
            const f4 gpre = ggate * gate[g] * (1.0f - gate[g]);
            f4 u;
            if constexpr (g == 0) {
                u = y[0];
            } else {
                u = splat(0.f);
                static_for<0, nd>([&](auto t) {
                    constexpr int d = d0 + decltype(t)::value;
                    u += qsf<ALG, d> * y[d] * y[d];
                });
            }
            p_sa[g] = hsum(gpre * u);
            p_sb[g] = hsum(gpre);
            const f4 gu = gpre * lp.sa[g];
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                f4 v = gz[d] * gate[g];
                if constexpr (g == 0) v += gu;
                else v += gu * (2.0f * qsf<ALG, d>) * y[d];
                gy[d] = cv ? v : splat(0.f);
            });
        });
        const float p_b1 = channel_rows_sum<1>(hsum(gy[0]));
#pragma unroll
        for (int g = 0; g < G; ++g) { p_sa[g] = channel_rows_sum<1>(p_sa[g]); p_sb[g] = channel_rows_sum<1>(p_sb[g]); }
        if (cv && lead) {
            if (B.has_b1) atomicAdd(d_b1 + c, p_b1);
#pragma unroll
            for (int g = 0; g < G; ++g) { atomicAdd(d_sa + c * G + g, p_sa[g]); atomicAdd(d_sb + c * G + g, p_sb[g]); }
        }
        park<ALG>(gy, slot(1, ct), ge.lane);
    }
    __syncthreads();   // all reads of gbuf (d/dR) done
    // ---- MVLinear weight gradient; d/dy tile to gbuf for the transposed MVLinear
    for (int ct = mt; ct < B.NTo; ct += MT) {
        f4 gy[D];
        unpark<ALG>(gy, slot(1, ct), ge.lane);
        store_tile<ALG, 1>(gy, gbuf, B.CPo, ct, ge);
        weight_grad<ALG, 1, false>(gy, xin, B.CPi, B.I, B.O, B.NTi, ct, ge, d_W1, B.w1_sub != 0);
    }
    __syncthreads();
}

template <class ALG, int MODE, bool BWD>
__global__ void __launch_bounds__(BWD ? 256 : 512) cemlp_wide_kernel(const DevCemlp C_arg, const RowIO io_arg) {
    // descriptors read in place from the kernarg segment (see cemlp_kernel)
    CSMPN_KERNEL_ARGS(C);
    using GE = Geo<ALG, 1>;
    constexpr int D = ALG::D, R = GE::R, NW = GE::NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int MT = C.MT, CT = C.CT;
    const int mt = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tid = threadIdx.x, nthr = MT * 64;
    const size_t det_goff = (size_t)blockIdx.x * (size_t)C.det_slice_floats;
    const GE ge(lane);
    // one row tile per workgroup: in LDS, or this workgroup's slice of the global scratch
    float* base = C.gtiles ? C.gtiles + (size_t)blockIdx.x * C.tile_floats : smem;
    float* buf_in = base + C.off_in;
    auto buf_p = [&](int i) -> float* { return base + ((i & 1) ? C.off_p1 : C.off_p0); };
    float* buf_z = base + C.off_z;
    float* buf_g = base + C.off_g;
    float* red = base + C.off_red;
    float* pk = base + C.off_park;
    int* tidx = reinterpret_cast<int*>(base + C.off_idx);
    const DevBlock& B0 = C.b[0];
    const DevBlock& BL = C.b[C.nblk - 1];
    const long ntiles = (io.rows + R - 1) / R;
    const long niter = (ntiles + gridDim.x - 1) / gridDim.x;
    auto save_off = [&](int kb) -> size_t {
        size_t o = 0;
        for (int j = 0; j + 1 < kb; ++j) o += (size_t)C.b[j].O;
        return o * (size_t)io.rows * D;
    };
    const bool use_saved = BWD && io.saved != nullptr && C.nblk > 1;

    TileIdx nidx = load_tile_indices<R>(io, (long)blockIdx.x * R, tid);
    for (long iter = 0; iter < niter; ++iter) {
        const long row0 = (iter * gridDim.x + blockIdx.x) * R;   // may be >= rows: fully masked tile
        store_tile_indices<R>(nidx, tidx, tid);
        __syncthreads();
        nidx = load_tile_indices<R>(io, row0 + (long)gridDim.x * R, tid);
        if (use_saved) {
            const DevBlock& Bl = C.b[C.nblk - 1];
            stage_plain<ALG, 1>(io.saved + save_off(C.nblk - 1), Bl.I, io.rows, buf_in, Bl.CPi, row0, tid, nthr);
        } else {
            stage_input<ALG, 1, kModeSegs<MODE>>(io, buf_in, tidx, B0.CPi, row0, tid, nthr);
        }
        __syncthreads();

        if constexpr (!BWD) {
            // ------------------------------------------------------------ forward
            const int O = BL.O;
            for (int k = 0; k < C.nblk; ++k) {
                const DevBlock& B = C.b[k];
                const f4 invMn = wide_forward_state<ALG, false>(B, buf_in, buf_z, red, pk, CT, MT, mt, ge, -1, -1, 0);
                const bool last = k + 1 == C.nblk;
                // the input tile is dead (read by the MVLinear only): block k's output replaces it
                for (int ct = mt; ct < B.NTo; ct += MT) {
                    const int c = NW * ct + ge.cn;
                    const float la = c < B.O ? B.la[c] : 0.f;
                    f4 s[D], out[D];
                    unpark<ALG>(s, wide_slot<ALG>(pk, CT, 0, ct), lane);
#pragma unroll
                    for (int d = 0; d < D; ++d) out[d] = la * s[d] * invMn;
                    if (!last) {
                        store_tile<ALG, 1>(out, buf_in, B.CPo, ct, ge);
                        if (io.save && c < B.O) {   // keep the next block's input for the backward
                            float* sp = io.save + save_off(k + 1);
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const long grow = row0 + ge.r0 + v;
                                if (grow < io.rows) {
#pragma unroll
                                    for (int d4 = 0; d4 < D; d4 += 4)
                                        *reinterpret_cast<f4*>(sp + (grow * B.O + c) * D + d4) =
                                            f4{out[d4][v], out[d4 + 1][v], out[d4 + 2][v], out[d4 + 3][v]};
                                }
                            }
                        }
                    } else if constexpr (MODE == MODE_EDGE) {
                        store_dense<ALG, 1>(out, buf_g, O, c, ge);   // buf_g is the z tile, dead by now
                    } else if (c < O) {
                        f4 res[4][D / 4];
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const long grow = row0 + ge.r0 + v;
                            const bool ok = MODE == MODE_NODE && io.resid && grow < io.rows;
#pragma unroll
                            for (int d4 = 0; d4 < D; d4 += 4)
                                res[v][d4 / 4] = ok ? *reinterpret_cast<const f4*>(io.resid + (grow * O + c) * D + d4) : splat(0.f);
                        }
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const long grow = row0 + ge.r0 + v;
                            if (grow < io.rows) {
                                float* p = io.y + (grow * O + c) * D;
#pragma unroll
                                for (int d4 = 0; d4 < D; d4 += 4)
                                    *reinterpret_cast<f4*>(p + d4) =
                                        f4{out[d4][v], out[d4 + 1][v], out[d4 + 2][v], out[d4 + 3][v]} + res[v][d4 / 4];
                            }
                        }
                    }
                }
                __syncthreads();
            }
            if constexpr (MODE == MODE_EDGE) {
                if (io.row_store) store_rows_dense<ALG, 1>(buf_g, O * D, row0, io.rows, io.agg, tid, nthr);
                else scatter_rows<ALG, 1, false>(buf_g, O * D, tidx, io.agg, 1.0f, tid, nthr);
                __syncthreads();
            }
        } else {
            // ------------------------------------------------------------ backward
            const int OL = BL.O;
            for (int k = C.nblk - 1; k >= 0; --k) {
                const DevBlock& B = C.b[k];
                const float* in = buf_in;
                if (use_saved && k + 1 < C.nblk) {   // this block's input replaces the previous one in the input buffer
                    if (k == 0) stage_input<ALG, 1, kModeSegs<MODE>>(io, buf_in, tidx, B0.CPi, row0, tid, nthr);
                    else stage_plain<ALG, 1>(io.saved + save_off(k), B.I, io.rows, buf_in, B.CPi, row0, tid, nthr);
                    __syncthreads();
                }
                // without saved inputs: recompute the input tile of block k from the tile's input
                for (int j = 0; !use_saved && j < k; ++j) {
                    const DevBlock& Bj = C.b[j];
                    const f4 iv = wide_forward_state<ALG, true>(Bj, in, buf_z, red, pk, CT, MT, mt, ge, -1, -1, 2);
                    for (int ct = mt; ct < Bj.NTo; ct += MT) {
                        const int c = NW * ct + ge.cn;
                        const float la = c < Bj.O ? Bj.la[c] : 0.f;
                        f4 s[D];
                        unpark<ALG>(s, wide_slot<ALG>(pk, CT, 2, ct), lane);
#pragma unroll
                        for (int d = 0; d < D; ++d) s[d] = la * s[d] * iv;
                        store_tile<ALG, 1>(s, buf_p(j), Bj.CPo, ct, ge);
                    }
                    __syncthreads();
                    in = buf_p(j);
                }
                const f4 invMn = wide_forward_state<ALG, true>(B, in, buf_z, red, pk, CT, MT, mt, ge, 0, 1, 2);
                const bool top = k + 1 == C.nblk;
                wide_block_backward<ALG>(B, in, buf_z, buf_g, red, pk, CT, MT, mt, ge, invMn, top ? io.gy : nullptr,
                                         top && MODE == MODE_EDGE ? tidx : nullptr, row0, io.rows, det_goff);
                // transposed MVLinear: gx[i] = sum_o W1[o][i][g] gy[o]   (A = gy tile in gbuf)
                const WSrc sW1t{B.pbW1, nullptr, B.O, B.CPi, B.w1_sub};
                if (k > 0) {
                    // d/d(output of block k - 1), channel tile it -> parking slot 3 of the same wave (it % MT == mt)
                    for (int it = mt; it < B.NTi; it += MT) {
                        f4 g[D];
#pragma unroll
                        for (int d = 0; d < D; ++d) g[d] = splat(0.f);
                        linear_from_tile<ALG, 1, false, true>(g, buf_g, B.CPo, B.KKo, sW1t, it, ge);
                        park<ALG>(g, wide_slot<ALG>(pk, CT, 3, it), lane);
                    }
                    __syncthreads();
                } else {
                    float* stage = buf_in;   // free: wide_block_backward ended with a barrier
                    const int Cs0 = io.seg[0].ch;
                    for (int it = mt; it < B.NTi; it += MT) {
                        // skip input-channel tiles none of whose segments wants a gradient (uniform per wave)
                        bool wanted = false;
                        for (int t = 0; t < io.nseg; ++t) {
                            const bool overlaps = io.seg[t].off < NW * (it + 1) && io.seg[t].off + io.seg[t].ch > NW * it;
                            wanted |= overlaps && ((MODE == MODE_EDGE && t == 0) || io.gx[t] != nullptr);
                        }
                        if (!wanted) continue;
                        f4 gx[D];
#pragma unroll
                        for (int d = 0; d < D; ++d) gx[d] = splat(0.f);
                        linear_from_tile<ALG, 1, false, true>(gx, buf_g, B.CPo, B.KKo, sW1t, it, ge);
                        const int i = NW * it + ge.cn;
                        int s = -1;
                        for (int t = 0; t < io.nseg; ++t)
                            if (i >= io.seg[t].off && i < io.seg[t].off + io.seg[t].ch) s = t;
                        if (MODE == MODE_EDGE && s == 0) {
                            store_dense<ALG, 1>(gx, stage, Cs0, i, ge);
                        } else if (s >= 0 && io.gx[s]) {
                            const Seg& sg = io.seg[s];
                            const int ci = i - sg.off;
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const long grow = row0 + ge.r0 + v;
                                if (grow < io.rows) {
                                    long trow = grow;
                                    if (MODE == MODE_EDGE) trow = tidx[2 * R + ge.r0 + v];   // edge_attr lives in original order
                                    float scale = 1.0f;
                                    if (sg.deg) { const int dg = sg.deg[grow]; scale = 1.0f / float(dg > 1 ? dg : 1); }
                                    float* p = io.gx[s] + (trow * sg.ch + ci) * D;
#pragma unroll
                                    for (int d4 = 0; d4 < D; d4 += 4) {
                                        f4 val = f4{gx[d4][v], gx[d4 + 1][v], gx[d4 + 2][v], gx[d4 + 3][v]} * scale;
                                        if (MODE == MODE_NODE && s == 0 && io.resid_bwd)
                                            val += *reinterpret_cast<const f4*>(io.gy + (grow * OL + ci) * D + d4);
                                        *reinterpret_cast<f4*>(p + d4) = val;
                                    }
                                }
                            }
                        }
                    }
                    if constexpr (MODE == MODE_EDGE) {
                        __syncthreads();
                        if (io.gx[0] && io.row_store) {
                            store_rows_dense<ALG, 1>(stage, Cs0 * D, row0, io.rows, io.gx[0], tid, nthr);
                        } else if (io.gx[0]) {
                            scatter_rows<ALG, 1, false>(stage, Cs0 * D, tidx, io.gx[0], 1.0f, tid, nthr);
                            scatter_rows<ALG, 1, false>(stage, Cs0 * D, tidx + R, io.gx[0], -1.0f, tid, nthr);
                        }
                    }
                    __syncthreads();
                }
            }
        }
    }
}

}  // namespace csmpn
