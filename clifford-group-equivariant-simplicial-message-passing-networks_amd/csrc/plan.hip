// LDS / tile planner of the general row-tile kernels (cemlp_kernel.hpp, cemlp_ps.hpp) and of the wide kernel
// (cemlp_wide.hpp): per-algebra table, tile layouts, storage variant, weight packing, deterministic gradient copies.
#include <cstring>

#include "plan.hpp"
#include "cemlp_wide.hpp"

namespace csmpn {

// ----------------------------------------------------------------------------- compiled algebras
AlgId alg_id(const float* metric, int n) {
    if (!metric || n < 2 || n > 5) return ALG_NONE;
    unsigned neg = 0;
    for (int i = 0; i < n; ++i) {
        if (metric[i] == 1.0f) continue;
        if (metric[i] == -1.0f) { neg |= 1u << i; continue; }
        return ALG_NONE;
    }
    if (n == 2 && neg == 0) return ALG_N2;
    if (n == 3 && neg == 0) return ALG_N3;
    if (n == 4 && neg == 0) return ALG_N4;
    if (n == 5 && neg == 0) return ALG_N5;
    if (n == 5 && neg == 0x10u) return ALG_N5M;
    if (n == 4 && neg == 0x8u) return ALG_N4M;
    return ALG_NONE;
}

#define CSMPN_ALG_OPS(tag, N, NEG, ...)                                                                                \
    {N, 1 << N, Alg<N, NEG>::P, has_h2_##tag(), has_ps_##tag(), "csmpn::Alg<" #N ", " #NEG ">", launch_cemlp_##tag,     \
     launch_cemlp_ps_##tag, launch_cemlp_wide_##tag, launch_gp_##tag, __VA_ARGS__}
#define CSMPN_D32_OPS(tag) &cemlp_pl_##tag(), &cemlp_plw_##tag(), &cemlp_pg_##tag()
const AlgOps& alg_ops(AlgId id) {
    static const AlgOps ops[ALG_COUNT] = {   // in AlgId order
        CSMPN_ALG_OPS(n2, 2, 0u),
        CSMPN_ALG_OPS(n3, 3, 0u),
        CSMPN_ALG_OPS(n4, 4, 0u),
        CSMPN_ALG_OPS(n5, 5, 0u, CSMPN_D32_OPS(n5)),
        CSMPN_ALG_OPS(n5m, 5, 16u, CSMPN_D32_OPS(n5m)),
        CSMPN_ALG_OPS(n4m, 4, 8u),
    };
    return ops[id];
}

namespace {
// ----------------------------------------------------------------------------- weight packing kernel
__global__ void pack_weights_kernel(const PackDesc P) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.total) return;
    int s = 0;
    while (e >= P.seg[s].count) { e -= P.seg[s].count; ++s; }
    const PackSeg& S = P.seg[s];
    const int H = P.H, NW = 16 / H;
    const int lane = e & 63;
    int rest = e >> 6;
    // fragment order [N tile][k-block][row half][grade][lane]
    const int g = rest % P.G; rest /= P.G;
    const int hp = rest % H; rest /= H;
    const int kk = rest % S.KK; rest /= S.KK;
    const int nt = rest;
    const int ncol = lane & 15;
    const int hcol = H == 1 ? 0 : (ncol >> 3);
    const int n = NW * nt + (H == 1 ? ncol : (ncol & 7));
    f4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 16 * kk + 4 * r + (lane >> 4);   // k-slot (q, v = r) -> channel 16 kk + 4 v + q
        const int o = S.transposed ? k : n, i = S.transposed ? n : k;
        float val = 0.f;
        if (hcol == hp && o < S.O && i < S.I)
            val = S.has_grades ? S.w[((size_t)o * S.I + i) * P.G + g] : S.w[(size_t)o * S.I + i];
        v[r] = val;
    }
    S.dst[e] = v;
}

// ----------------------------------------------------------------------------- planning
// floats of one row tile's buffers; tiles are [channel][D][R] with channel stride R*D + 4
struct TileLayout { int off_in, off_p0, off_p1, off_z, off_g, off_red, off_idx, total; int off_park = 0; };
TileLayout tile_layout(int D, int H, const csmpn_block_params* blocks, int nblk, bool bwd, int stage_rowlen,
                       bool use_saved = false, bool ps = false, bool share_inz = false) {
    int maxO = 0, maxCPo = 0;
    for (int k = 0; k < nblk; ++k) {
        maxO = blocks[k].out_features > maxO ? blocks[k].out_features : maxO;
        maxCPo = rup(blocks[k].out_features, 4) > maxCPo ? rup(blocks[k].out_features, 4) : maxCPo;
    }
    const int R = 16 * H, CS = R * D + 4, NW = 16 / H;
    const int MT = cdiv(maxO, NW);
    int sz_in = rup(blocks[0].in_features, 4) * CS;
    const int sz_o = maxCPo * CS;
    // backward with saved block inputs: ONE input buffer serves every block in turn
    const bool single_in = bwd && use_saved && nblk > 1;
    if ((single_in || share_inz) && sz_o > sz_in) sz_in = sz_o;
    TileLayout L;
    int off = 0;
    if (!bwd) {
        // forward: a block reads its input tile only in its first phase (MVLinear) and writes
        // its output after its last one, so the output of block k may overwrite the input of
        // block k (ping-pong degenerates to ONE input buffer); the dense scatter staging of
        // the edge forward reuses the z buffer, dead by then.
        const int sz_io = (nblk >= 2 && sz_o > sz_in) ? sz_o : sz_in;
        int sz_z = sz_o;
        if (stage_rowlen > 0 && R * stage_rowlen > sz_z) sz_z = rup(R * stage_rowlen, 4);
        if (MT == 1) {
            // single-wave tiles: the gated activations z are written after the block's only
            // read of its input (MVLinear) and the LDS executes a wave in order, so z (and the
            // scatter staging) share the input buffer too: ONE buffer per tile.
            const int sz_all = sz_io > sz_z ? sz_io : sz_z;
            L.off_in = off; L.off_p0 = off; L.off_p1 = off; L.off_z = off; L.off_g = off; off += sz_all;
        } else {
            L.off_in = off; L.off_p0 = off; L.off_p1 = off; off += sz_io;
            L.off_z = off; L.off_g = off; off += sz_z;
        }
    } else {
        L.off_in = off; off += sz_in;
        L.off_p0 = off; off += (nblk >= 2 && !single_in) ? sz_o : 0;
        L.off_p1 = off; off += (nblk >= 3 && !single_in) ? sz_o : 0;
        if (share_inz) L.off_z = L.off_in;   // z aliases the input buffer (sz_in >= sz_o, checked by the caller)
        else { L.off_z = off; off += sz_o; }
        L.off_g = off;
        int sz_g = sz_o;
        if (stage_rowlen > 0 && R * stage_rowlen > sz_g) sz_g = rup(R * stage_rowlen, 4);
        const int park = ps ? 128 * D : 256 * D;         // parking area of the incoming gradient
        if (MT == 1 && park > sz_g) sz_g = park;
        off += sz_g;
    }
    // cross-wave LayerNorm scratch of the barrier variants: reserved for single-wave tiles too (they
    // run a barrier variant when the weight store does not fit beside the tiles, or in global scratch)
    L.off_red = off; off += rup(MT * 16, 4);
    L.off_idx = off; off += rup(3 * R, 4);   // int copies of the tile's gathered row indices
    L.total = off;
    return L;
}
// Wide plans (65..256 output channels, cemlp_wide.hpp): one row tile per workgroup, H = 1, CT = ceil(max O / 16) channel
// tiles. As tile_layout, but the forward's block outputs always replace the input tile (z is a buffer of its own: several
// waves), the LayerNorm scratch has CT entries and a parking region of kWideSlots* x CT lane-layout tensors follows.
constexpr int kWideMaxChannels = 256;
TileLayout wide_layout(int D, const csmpn_block_params* blocks, int nblk, bool bwd, int stage_rowlen, bool use_saved) {
    int maxCPo = 0;
    for (int k = 0; k < nblk; ++k) maxCPo = rup(blocks[k].out_features, 4) > maxCPo ? rup(blocks[k].out_features, 4) : maxCPo;
    const int R = 16, CS = R * D + 4, CT = cdiv(maxCPo, 16);
    int sz_in = rup(blocks[0].in_features, 4) * CS;
    const int sz_o = maxCPo * CS;
    const bool single_in = !bwd || (use_saved && nblk > 1);
    if (single_in && sz_o > sz_in) sz_in = sz_o;
    int sz_g = sz_o;
    if (stage_rowlen > 0 && R * stage_rowlen > sz_g) sz_g = rup(R * stage_rowlen, 4);
    TileLayout L;
    int off = 0;
    L.off_in = off; off += sz_in;
    L.off_p0 = single_in ? L.off_in : off; off += (!single_in && nblk >= 2) ? sz_o : 0;
    L.off_p1 = single_in ? L.off_in : off; off += (!single_in && nblk >= 3) ? sz_o : 0;
    if (!bwd) {   // forward: the edge staging reuses the z tile, dead by then
        L.off_z = off; L.off_g = off; off += sz_g;
    } else {
        L.off_z = off; off += sz_o;
        L.off_g = off; off += sz_g;
    }
    L.off_red = off; off += rup(CT * 16, 4);
    L.off_idx = off; off += rup(3 * R, 4);
    L.off_park = off; off += (bwd ? kWideSlotsBwd : kWideSlotsFwd) * CT * D * 256;
    L.total = off;
    return L;
}

struct Choice { int var, rt, wgs; bool mirror; };
// backward kernels are built for 256 threads (512 VGPRs), forward for 512 threads
Choice choose_variant(int MT, size_t tile_bytes, size_t mirror_bytes, size_t wstore_bytes, bool bwd, bool ps = false) {
    // workgroups of at most 512 threads (forward, parity-split backward) / 256 threads (backward)
    // parity-split forward: 256-thread workgroups, three per CU (168 VGPRs: 3 waves per SIMD)
    const int waves = ps ? 4 : (bwd ? 4 : 8);
    const int max_wgs = (ps && !bwd) ? 3 : 2;
    const int max_rt = (waves / MT) > 0 ? waves / MT : 1;
    auto fit = [&](size_t fixed, int& rt_out, int& wgs_out) {
        int best_waves = 0;
        for (int wgs = 1; wgs <= max_wgs; ++wgs) {
            const size_t budget = (size_t)kMaxLdsBytes / wgs;
            if (budget <= fixed) continue;
            int rt = (int)((budget - fixed) / tile_bytes);
            if (rt > max_rt) rt = max_rt;
            if (rt < 1) continue;
            if (wgs * rt > best_waves) { best_waves = wgs * rt; rt_out = rt; wgs_out = wgs; }
        }
        return best_waves > 0;
    };
    Choice c{VAR_GLOBAL, 1, 1, false};
    int rt = 0, wgs = 1;
    const int min_lds_waves = sw().min_lds_tiles;
    // single-wave tiles with gradient mirror and weight store in LDS
    if (MT == 1 && fit(mirror_bytes + wstore_bytes, rt, wgs) && rt * wgs >= min_lds_waves) {
        c.var = VAR_WAVE; c.rt = rt; c.wgs = wgs; c.mirror = bwd && mirror_bytes > 0;
        return c;
    }
    if (fit(mirror_bytes, rt, wgs) && rt * wgs >= min_lds_waves) {
        c.var = VAR_GROUP; c.rt = rt; c.wgs = wgs; c.mirror = bwd && mirror_bytes > 0;
        return c;
    }
    if (fit(0, rt, wgs) && rt * wgs >= min_lds_waves) {   // tiles fit, the gradient mirror does not
        c.var = VAR_GROUP_NM; c.rt = rt; c.wgs = wgs; c.mirror = false;
        return c;
    }
    c.rt = (4 / MT) > 0 ? 4 / MT : 1;
    return c;
}
constexpr unsigned kGlobalTileGrid = 256;   // workgroups when the tiles live in global scratch

size_t packed_f4_count(int G, int H, const csmpn_block_params* blocks, int nblk) {
    size_t tot = 0;
    const int NW = 16 / H;
    for (int k = 0; k < nblk; ++k) {
        const int I = blocks[k].in_features, O = blocks[k].out_features;
        const size_t KKi = cdiv(I, 16), KKo = cdiv(O, 16), NTi = cdiv(I, NW), NTo = cdiv(O, NW);
        const size_t per = (size_t)H * G * 64;
        tot += per * (NTo * KKi + NTi * KKo);        // W1 forward + transposed
        tot += per * 4 * NTo * KKo;                  // WR, WL forward + transposed
    }
    return tot;
}

int mirror_floats_of(int I, int O, int G, int P, bool sub) {
    DevBlock B{};
    B.I = I; B.O = O; B.w1_sub = sub;
    int m = 0;
    for_each_grad_tensor(B, G, P, [&](float*, int count, bool) { m += count; });
    return m;
}

// Tile height per launch. H = 2 (32-row tiles, 8 lane columns per half) needs every width
// <= 8 channels, an algebra with H = 2 kernels and the single-wave variant (which stages raw
// weights in LDS, so no packed fragments are shared between launches of different H).
int wstore_floats_of(int I, int O, int G, int P, bool sub) {
    return (sub ? G : 1) * O * rup(I, 4) + 2 * G * O * rup(O, 4) + 3 * O + 3 * O * G + O * P;
}
int wstore_total(int G, int P, const csmpn_block_params* blocks, int nblk) {
    int m = 0;
    for (int k = 0; k < nblk; ++k)
        m += rup(wstore_floats_of(blocks[k].in_features, blocks[k].out_features, G, P, blocks[k].lin_subspaces != 0), 4);
    return m;
}

}  // namespace

int mirror_total(int G, int P, const csmpn_block_params* blocks, int nblk) {
    int m = 0;
    for (int k = 0; k < nblk; ++k)
        m += rup(mirror_floats_of(blocks[k].in_features, blocks[k].out_features, G, P, blocks[k].lin_subspaces != 0), 4);
    return m;
}

namespace {
// Parity-split kernels: odd n, every block at most 8 output channels, tiles + weight store +
// gradient mirror resident in LDS. The decision does not depend on the direction or the row
// count, so a forward and the backward that reads its saved block inputs always agree.
bool decide_ps(AlgId id, int n, const csmpn_block_params* blocks, int nblk) {
    if (!alg_ops(id).ps) return false;
    // Default: on for D = 32 (n = 5: half the registers per tensor and every lane column in use
    // instead of 8 of 16 - S3 runs 1.9x faster), off for Cl(3,0), where it measured 15-20 % slower
    // than the 32-row layout. CSMPN_FORCE_PS=0|1 overrides.
    if (sw().force_ps >= 0 ? sw().force_ps == 0 : n < 5) return false;
    for (int k = 0; k < nblk; ++k) if (blocks[k].out_features > 8) return false;
    const int D = 1 << n, G = n + 1;
    const size_t mirror = (size_t)mirror_total(G, alg_ops(id).paths, blocks, nblk) * 4;
    const size_t wst = (size_t)wstore_total(G, alg_ops(id).paths, blocks, nblk) * 4;
    // worst case: backward without saved inputs, forward with the widest staging row
    const TileLayout Lb = tile_layout(D, 1, blocks, nblk, true, 8 * D, false, true);
    const TileLayout Lf = tile_layout(D, 1, blocks, nblk, false, 8 * D, false, true);
    const Choice cb = choose_variant(1, (size_t)Lb.total * 4, mirror, wst, true, true);
    const Choice cf = choose_variant(1, (size_t)Lf.total * 4, 0, wst, false, true);
    const int need = n >= 5 ? 1 : 4;   // D = 32: one 16-row tile per CU is all the LDS holds in any layout
    return cb.var == VAR_WAVE && cf.var == VAR_WAVE && cb.rt * cb.wgs >= need && cf.rt * cf.wgs >= need;
}

int decide_h(AlgId id, int n, const csmpn_block_params* blocks, int nblk, bool bwd, int stage_rowlen,
             bool use_saved, long rows) {
    int maxO = 0;
    for (int k = 0; k < nblk; ++k) maxO = blocks[k].out_features > maxO ? blocks[k].out_features : maxO;
    if (maxO > 8 || !alg_ops(id).h2) return 1;
    const int D = 1 << n, G = n + 1;
    const TileLayout L2 = tile_layout(D, 2, blocks, nblk, bwd, stage_rowlen, use_saved);
    const size_t mirror = bwd ? (size_t)mirror_total(G, alg_ops(id).paths, blocks, nblk) * 4 : 0;
    const size_t wst = (size_t)wstore_total(G, alg_ops(id).paths, blocks, nblk) * 4;
    const Choice c2 = choose_variant(1, (size_t)L2.total * 4, mirror, wst, bwd);
    if (c2.var != VAR_WAVE || c2.rt * c2.wgs < 2) return 1;
    // 32-row tiles only when there are enough of them to occupy every wave slot of the chip;
    // small row counts (e.g. the node update of a 10k-node complex) get 16-row tiles
    if (sw().force_h) return sw().force_h;   // debugging aid
    const long tiles2 = (rows + 31) / 32;
    if (tiles2 < 256L * c2.rt * c2.wgs) return 1;
    return 2;
}

}  // namespace

// bwd / stage_rowlen decide the footprint. stage_rowlen: dense staging row length needed in
// buf_g (edge forward scatter).
int make_plan(AlgId id, const csmpn_block_params* blocks, const csmpn_block_grads* grads, int nblk, void* workspace,
              size_t workspace_bytes, bool bwd, int stage_rowlen, bool use_saved, long rows, Plan& plan, bool deterministic) {
    if (nblk < 1 || nblk > CSMPN_MAX_BLOCKS) return fail(CSMPN_ERR_INVALID, "n_blocks=%d not in 1..%d", nblk, CSMPN_MAX_BLOCKS);
    const int n = alg_ops(id).n, D = 1 << n, G = n + 1, P = alg_ops(id).paths;
    memset(&plan, 0, sizeof(plan));
    plan.id = id;
    plan.blocks = blocks;
    plan.workspace = workspace;
    plan.workspace_bytes = workspace_bytes;
    DevCemlp& C = plan.C;
    C.nblk = nblk;
    int maxO = 0;
    for (int k = 0; k < nblk; ++k) {
        const csmpn_block_params& b = blocks[k];
        if (b.in_features < 1 || b.out_features < 1) return fail(CSMPN_ERR_INVALID, "block %d: bad feature counts", k);
        if (k > 0 && b.in_features != blocks[k - 1].out_features)
            return fail(CSMPN_ERR_INVALID, "block %d: in_features %d != previous out_features %d", k, b.in_features,
                        blocks[k - 1].out_features);
        if (!b.lin_w || !b.silu_a || !b.silu_b || !b.gp_w || !b.norm_a || !b.right_w || !b.left_w || !b.left_b || !b.ln_a)
            return fail(CSMPN_ERR_INVALID, "block %d: null parameter pointer", k);
        maxO = b.out_features > maxO ? b.out_features : maxO;
    }
    const bool ps = decide_ps(id, n, blocks, nblk);
    const int H = ps ? 1 : decide_h(id, n, blocks, nblk, bwd, stage_rowlen, use_saved, rows);
    const int NW = ps ? 8 : 16 / H;
    const int MT = ps ? 1 : cdiv(maxO, NW);
    plan.ps = ps;
    // more than 4 channel tiles (64 channels): the wide kernel, up to kWideMaxChannels
    if (MT > 4 && maxO > kWideMaxChannels)
        return fail(CSMPN_ERR_UNSUPPORTED, "out_features %d > %d not supported", maxO, kWideMaxChannels);
    plan.wide = MT > 4;
    C.MT = MT;
    C.H = H;
    plan.H = H;

    const size_t need = packed_f4_count(G, H, blocks, nblk) * sizeof(f4);
    if (workspace_bytes < need || !workspace) return fail(CSMPN_ERR_INVALID, "workspace too small: %zu < %zu", workspace_bytes, need);
    f4* ws = reinterpret_cast<f4*>(workspace);
    PackDesc& PD = plan.P;
    PD.G = G;
    PD.H = H;
    size_t cursor = 0;
    int mirror = 0, wstore = 0;
    auto add_seg = [&](const float* w, int O, int I, int has_grades, int transposed, int NT, int KK) -> const f4* {
        PackSeg& s = PD.seg[PD.nseg++];
        s.w = w; s.dst = ws + cursor; s.O = O; s.I = I; s.has_grades = has_grades; s.transposed = transposed;
        s.NT = NT; s.KK = KK; s.count = NT * KK * H * G * 64;
        PD.total += s.count;
        const f4* p = s.dst;
        cursor += (size_t)s.count;
        return p;
    };
    for (int k = 0; k < nblk; ++k) {
        const csmpn_block_params& b = blocks[k];
        DevBlock& B = C.b[k];
        B.I = b.in_features; B.O = b.out_features;
        B.KKi = cdiv(B.I, 16); B.KKo = cdiv(B.O, 16);
        B.NTi = cdiv(B.I, NW); B.NTo = cdiv(B.O, NW);
        B.CPi = rup(B.I, 4); B.CPo = rup(B.O, 4);
        B.has_b1 = b.lin_b != nullptr;
        B.w1_sub = b.lin_subspaces ? 1 : 0;
        B.b1 = b.lin_b; B.sa = b.silu_a; B.sb = b.silu_b; B.w = b.gp_w; B.an = b.norm_a; B.bL = b.left_b; B.la = b.ln_a;
        B.pfW1 = add_seg(b.lin_w, B.O, B.I, B.w1_sub, 0, B.NTo, B.KKi);
        B.pfWR = add_seg(b.right_w, B.O, B.O, 1, 0, B.NTo, B.KKo);
        B.pfWL = add_seg(b.left_w, B.O, B.O, 1, 0, B.NTo, B.KKo);
        B.pbW1 = add_seg(b.lin_w, B.O, B.I, B.w1_sub, 1, B.NTi, B.KKo);
        B.pbWR = add_seg(b.right_w, B.O, B.O, 1, 1, B.NTo, B.KKo);
        B.pbWL = add_seg(b.left_w, B.O, B.O, 1, 1, B.NTo, B.KKo);
        B.W1 = b.lin_w; B.WR = b.right_w; B.WL = b.left_w;
        B.lds_goff = mirror;
        B.lds_woff = wstore;
        wstore += rup(wstore_floats_of(B.I, B.O, G, P, B.w1_sub != 0), 4);
        mirror += rup(mirror_floats_of(B.I, B.O, G, P, B.w1_sub), 4);
        if (bwd) {
            if (!grads) return fail(CSMPN_ERR_INVALID, "grads is null");
            const csmpn_block_grads& g = grads[k];
            if (!g.lin_w || !g.silu_a || !g.silu_b || !g.gp_w || !g.norm_a || !g.right_w || !g.left_w || !g.left_b ||
                !g.ln_a || (B.has_b1 && !g.lin_b))
                return fail(CSMPN_ERR_INVALID, "block %d: null gradient pointer", k);
            B.gW1 = g.lin_w; B.gb1 = g.lin_b; B.gsa = g.silu_a; B.gsb = g.silu_b; B.gw = g.gp_w; B.gan = g.norm_a;
            B.gWR = g.right_w; B.gWL = g.left_w; B.gbL = g.left_b; B.gla = g.ln_a;
        }
    }
    plan.pack_f4 = cursor;

    if (plan.wide) {
        // CT channel tiles on MT waves: 4 in the backward (one wave per SIMD at ~500 VGPRs), 8 in the forward; one row tile
        // per workgroup, in LDS when its buffers and parking region fit, else in the global scratch behind the packed weights
        const int CT = cdiv(maxO, 16), cap = bwd ? 4 : 8;
        const TileLayout L = wide_layout(D, blocks, nblk, bwd, stage_rowlen, use_saved);
        C.CT = CT; C.MT = CT < cap ? CT : cap; C.RT = 1;
        C.share_inz = 0; C.phased = 0; C.mirror_floats = 0; C.wstore_floats = 0;
        C.off_in = L.off_in; C.off_p0 = L.off_p0; C.off_p1 = L.off_p1; C.off_z = L.off_z; C.off_g = L.off_g;
        C.off_red = L.off_red; C.off_idx = L.off_idx; C.off_park = L.off_park; C.tile_floats = L.total;
        // deterministic mode (n <= 3): one row tile per workgroup already; every gradient word has one writing wave
        plan.det_general = deterministic && n <= 3;
        const size_t tile_bytes = (size_t)L.total * 4;
        if (tile_bytes <= (size_t)kMaxLdsBytes) {
            C.gtiles = nullptr;
            plan.lds_bytes = tile_bytes;
            plan.var = VAR_GROUP_NM;
        } else {
            const size_t scratch = (size_t)kGlobalTileGrid * tile_bytes;
            if (workspace_bytes < need + scratch)
                return fail(CSMPN_ERR_INVALID, "workspace too small: %zu < %zu", workspace_bytes, need + scratch);
            C.gtiles = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + need);
            plan.lds_bytes = 0;
            plan.var = VAR_GLOBAL;
        }
        plan.grid_cap = kGlobalTileGrid;
        plan.threads = (unsigned)(C.MT * 64);
        return CSMPN_OK;
    }

    // buffers of one row tile (floats)
    TileLayout L = tile_layout(D, H, blocks, nblk, bwd, stage_rowlen, use_saved, ps);
    // choose the storage variant, row tiles per workgroup and workgroups per CU
    Choice ch = choose_variant(MT, (size_t)L.total * 4, bwd ? (size_t)mirror * 4 : 0, (size_t)wstore * 4, bwd, ps);
    // Backward, when LDS (not registers) limits the resident waves: let z alias the input buffer and
    // stage the input tile a second time for the MVLinear weight gradient, if that buys a row tile
    // per CU (S2: 3 -> 4 waves per CU) or a better storage variant. Needs every block's input to be
    // re-stageable from memory: a single block, or saved block inputs.
    C.share_inz = 0;
    const bool allow_share = !sw().no_share;
    if (bwd && !ps && H == 1 && allow_share && (use_saved || nblk == 1)) {
        const TileLayout Ls = tile_layout(D, H, blocks, nblk, bwd, stage_rowlen, use_saved, ps, true);
        const Choice cs = choose_variant(MT, (size_t)Ls.total * 4, (size_t)mirror * 4, (size_t)wstore * 4, bwd, ps);
        // resident waves per CU: the backward kernels hold ~500 VGPRs, one wave per SIMD at most
        auto resident = [&](const Choice& c) { const int w = c.rt * c.wgs * MT; return w < 4 ? w : 4; };
        if (cs.var < ch.var || (cs.var == ch.var && resident(cs) > resident(ch))) {
            L = Ls; ch = cs; C.share_inz = 1;
        }
    }
    // Phased backward (round 3, cemlp_kernel.hpp): block by block, last first, each over all row tiles - the LDS mirror then
    // holds ONE block's gradient tensors. Taken when that puts more waves on the CU than the all-blocks mirror allows (md17's
    // 32-channel edge model: 110 KB of mirror left room for one 38 KB row tile = 2 waves per CU; 57 KB leave room for two).
    // Needs the saved block inputs and the hand-over region behind them (general_phased_shape: the same predicate sizes it).
    C.phased = 0;
    int mirror_used = mirror;
    const bool no_phased = sw().no_phased;
    // Only where the all-blocks form already keeps a mirror (never away from the no-mirror variant: switching the md17 task
    // model's small node stages to the mirror form cost 6 % of its step) and for launches of at least one row tile per CU
    // (measured on the md17 model, 11 266 adjacencies: step 4.62 ms with a 32 k-row threshold, 4.47 ms with 4 k or 8 k).
    const long phased_min_rows = sw().phased_min_rows;
    // From the no-mirror variant (per-tile float atomics onto the workgroup's copy) to the phased mirror form only for larger
    // launches (M32 node stage, 10 k rows: 0.59 -> 0.48 ms; the md17 model's 940-row node stages lose).
    const bool from_nm = ch.var == VAR_GROUP_NM && rows >= 2 * phased_min_rows;
    if (bwd && use_saved && nblk > 1 && !ps && H == 1 && !no_phased && rows >= phased_min_rows && (ch.var == VAR_GROUP || from_nm) &&
        general_phased_shape(n, blocks, nblk)) {
        int mirror_max = 0;
        for (int k = 0; k < nblk; ++k) {
            const int m = rup(mirror_floats_of(C.b[k].I, C.b[k].O, G, P, C.b[k].w1_sub), 4);
            mirror_max = m > mirror_max ? m : mirror_max;
        }
        auto resident = [&](const Choice& c) { const int w = c.rt * c.wgs * MT; return w < 4 ? w : 4; };
        for (int sh = 0; sh < (allow_share ? 2 : 1); ++sh) {
            const TileLayout Lp = tile_layout(D, H, blocks, nblk, bwd, stage_rowlen, use_saved, ps, sh != 0);
            const Choice cp = choose_variant(MT, (size_t)Lp.total * 4, (size_t)mirror_max * 4, (size_t)wstore * 4, bwd, ps);
            if (cp.var == VAR_GROUP && (resident(cp) > resident(ch) || (from_nm && !C.phased))) {
                L = Lp; ch = cp; C.share_inz = sh; C.phased = 1; mirror_used = mirror_max;
            }
        }
        if (C.phased)
            for (int k = 0; k < nblk; ++k) C.b[k].lds_goff = 0;
    }
    // Deterministic mode on these kernels (n <= 3: Cl(2,0), Cl(3,0) widths outside the lane kernels - the md17 / NBA layers):
    // ONE row tile per workgroup, so that every gradient word (LDS mirror or the workgroup's global copy) has one writing
    // wave - the MT waves of a tile own disjoint channels - and the order of its sums is the tile order.
    plan.det_general = false;
    if (deterministic && n <= 3 && !ps && ch.var != VAR_GLOBAL) {
        plan.det_general = true;
        if (bwd) ch.rt = 1;
    }
    C.off_in = L.off_in; C.off_p0 = L.off_p0; C.off_p1 = L.off_p1; C.off_z = L.off_z; C.off_g = L.off_g;
    C.off_red = L.off_red; C.off_idx = L.off_idx; C.tile_floats = L.total;
    const size_t tile_bytes = (size_t)L.total * 4;
    if (ps && ch.var != VAR_WAVE) return fail(CSMPN_ERR_INVALID, "internal: parity-split plan without the single-wave variant");
    if (H == 2 && ch.var != VAR_WAVE) return fail(CSMPN_ERR_INVALID, "internal: H=2 without the single-wave variant");
    C.RT = ch.rt;
    plan.var = ch.var;
    C.mirror_floats = ch.mirror ? mirror_used : 0;
    C.wstore_floats = ch.var == VAR_WAVE ? wstore : 0;
    if (ch.var != VAR_GLOBAL) {
        C.gtiles = nullptr;
        plan.lds_bytes = (size_t)(C.mirror_floats + C.wstore_floats) * 4 + (size_t)ch.rt * tile_bytes;
        plan.grid_cap = 256u * (unsigned)ch.wgs;
    } else {
        // tiles too large for the LDS: keep them in a global scratch behind the packed weights
        const size_t scratch = (size_t)kGlobalTileGrid * C.RT * tile_bytes;
        if (workspace_bytes < need + scratch)
            return fail(CSMPN_ERR_INVALID, "workspace too small: %zu < %zu", workspace_bytes, need + scratch);
        C.gtiles = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + need);
        plan.lds_bytes = 0;
        plan.grid_cap = kGlobalTileGrid;
    }
    plan.threads = (unsigned)(C.RT * MT * 64);
    return CSMPN_OK;
}

namespace {
// Wide plans: a copy grows with O^2 (a 128-channel Cl(3,0) node model: ~1 MB), so the number of copies (= workgroups of
// the deterministic launch) shrinks with it: as many as fit in kWideDetBudget, at least kWideDetMinGroups, at most kDetGroups.
constexpr size_t kWideDetBudget = (size_t)128 << 20;
constexpr int kWideDetMinGroups = 16;
int wide_det_groups(size_t slice_floats) {
    const size_t g = kWideDetBudget / (slice_floats * sizeof(float) > 0 ? slice_floats * sizeof(float) : 1);
    return g < (size_t)kWideDetMinGroups ? kWideDetMinGroups : (g > (size_t)kDetGroups ? kDetGroups : (int)g);
}
// bytes reserved for them: max(budget, kWideDetMinGroups copies) covers every slice up to slice_floats
size_t wide_det_reserve(size_t slice_floats) {
    const size_t floor_bytes = (size_t)kWideDetMinGroups * slice_floats * sizeof(float);
    return (floor_bytes > kWideDetBudget ? floor_bytes : kWideDetBudget) + 256;
}
struct DetMap {
    int n;
    int total;
    struct { float* dst; int off; int count; } t[40];
};
// grads += sum over the workgroups' copies, fixed order: one thread per word (consecutive threads read consecutive
// words of a copy), eight copies in flight
__global__ void __launch_bounds__(256) det_reduce_kernel(const DetMap M, const float* slices, int nslices) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M.total) return;
    float s = 0.f;
    int w = 0;
    for (; w + 8 <= nslices; w += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = slices[(size_t)(w + i) * M.total + e];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; w < nslices; ++w) s += slices[(size_t)w * M.total + e];
    for (int i = 0; i < M.n; ++i)
        if (e >= M.t[i].off && e < M.t[i].off + M.t[i].count) { M.t[i].dst[e - M.t[i].off] += s; return; }
}

}  // namespace

size_t det_slice_bytes(int n, const csmpn_block_params* blocks, int nblk) {
    if (n > 3 || nblk < 1) return 0;
    // upper bound over the algebras with n generators: paths <= (n + 1)^3 (Cl(3,0): 20 of 64, Cl(2,0): 10 of 27)
    const int G = n + 1, P = n == 3 ? 20 : (n == 2 ? 10 : (n + 1) * (n + 1) * (n + 1));
    const size_t slice = (size_t)mirror_total(G, P, blocks, nblk);
    int maxO = 0;
    for (int k = 0; k < nblk; ++k) maxO = blocks[k].out_features > maxO ? blocks[k].out_features : maxO;
    if (maxO > 64) return wide_det_reserve(slice);
    return slice * sizeof(float) * kDetGroups + 256;
}

// required: deterministic mode (too small a workspace is an error); otherwise a caller's smaller workspace means atomics
// onto the one copy
int det_slices(const Plan& plan, bool required, DetSlices& S) {
    const AlgOps& A = alg_ops(plan.id);
    S.base = nullptr;
    S.floats = mirror_total(A.n + 1, A.paths, plan.blocks, plan.C.nblk);
    S.groups = plan.wide ? wide_det_groups((size_t)S.floats) : kDetGroups;
    const size_t bytes = (size_t)S.floats * sizeof(float) * S.groups + 256;
    if (!plan.workspace || plan.workspace_bytes < bytes) {
        if (required)
            return fail(CSMPN_ERR_INVALID, "workspace too small for the deterministic backward: %zu < %zu", plan.workspace_bytes, bytes);
        return CSMPN_OK;
    }
    S.base = reinterpret_cast<float*>(tail_region(plan, bytes, 256));
    return CSMPN_OK;
}

// the kernels' accumulators = copy 0 of the zeroed region; workgroup b adds b * det_slice_floats
int det_launch_begin(const Plan& plan, const DetSlices& S, long grid, DevCemlp& Cd, hipStream_t st) {
    const AlgOps& A = alg_ops(plan.id);
    HIP_TRY(hipMemsetAsync(S.base, 0, (size_t)grid * S.floats * sizeof(float), st));
    Cd.det_slice_floats = S.floats;
    int j = 0;
    for (int k = 0; k < Cd.nblk; ++k) {
        for_each_grad_tensor(Cd.b[k], A.n + 1, A.paths, [&](float*& p, int count, bool present) {
            if (present) p = S.base + j;
            j += count;
        });
        j = rup(j, 4);
    }
    return CSMPN_OK;
}

int det_reduce(const Plan& plan, const DetSlices& S, long grid, hipStream_t st) {
    const AlgOps& A = alg_ops(plan.id);
    DetMap M;
    M.n = 0;
    int off = 0;
    for (int k = 0; k < plan.C.nblk; ++k) {
        for_each_grad_tensor(plan.C.b[k], A.n + 1, A.paths, [&](float* dst, int count, bool present) {
            if (present && dst) { M.t[M.n].dst = dst; M.t[M.n].off = off; M.t[M.n].count = count; ++M.n; }
            off += count;
        });
        off = rup(off, 4);
    }
    M.total = off;
    hipLaunchKernelGGL(det_reduce_kernel, dim3((M.total + 255) / 256), dim3(256), 0, st, M, (const float*)S.base, (int)grid);
    HIP_TRY(hipGetLastError());
    return CSMPN_OK;
}

int run_pack(const Plan& plan, hipStream_t st) {
    if (plan.P.total == 0 || plan.var == VAR_WAVE) return CSMPN_OK;   // VAR_WAVE stages raw weights in LDS
    const unsigned block = 256, grid = (unsigned)((plan.P.total + block - 1) / block);
    hipLaunchKernelGGL(pack_weights_kernel, dim3(grid), dim3(block), 0, st, plan.P);
    HIP_TRY(hipGetLastError());
    return CSMPN_OK;
}

size_t plan_front_bytes(int n, const csmpn_block_params* blocks, int n_blocks) {
    // H is not known without the metric: reserve for the larger packing (H = 2 when narrow)
    int maxO = 0;
    for (int k = 0; k < n_blocks; ++k) maxO = blocks[k].out_features > maxO ? blocks[k].out_features : maxO;
    size_t bytes = packed_f4_count(n + 1, 1, blocks, n_blocks) * sizeof(f4);
    if (maxO <= 8) {
        const size_t b2 = packed_f4_count(n + 1, 2, blocks, n_blocks) * sizeof(f4);
        bytes = b2 > bytes ? b2 : bytes;
    }
    const int D = 1 << n, MT = cdiv(maxO, 16);
    size_t scratch = 0;
    if (maxO > 64 && maxO <= kWideMaxChannels) {
        // wide kernel (cemlp_wide.hpp): packed weights (H = 1) and the global tile scratch of the largest layout (backward
        // without saved inputs, forward with the edge staging row; reserved even where the tile fits the LDS: the choice
        // needs no metric, but the scratch is cheap to reserve and keeps the sizing simple)
        const TileLayout Lb = wide_layout(D, blocks, n_blocks, true, 0, false);
        const TileLayout Lf = wide_layout(D, blocks, n_blocks, false, blocks[n_blocks - 1].out_features * D, false);
        scratch = (size_t)kGlobalTileGrid * (size_t)(Lb.total > Lf.total ? Lb.total : Lf.total) * 4;
    } else {
        // worst case over the entry points (H = 1): backward layout / forward layout with the edge-forward staging row
        const TileLayout Lb = tile_layout(D, 1, blocks, n_blocks, true, 0);
        const TileLayout Lf = tile_layout(D, 1, blocks, n_blocks, false, blocks[n_blocks - 1].out_features * D);
        const Choice cb = choose_variant(MT, (size_t)Lb.total * 4, 0, 0, true);
        const Choice cf = choose_variant(MT, (size_t)Lf.total * 4, 0, 0, false);
        // global tile scratch: reserved whenever a launch may choose it (the choice itself needs the metric: path count ->
        // mirror / weight-store size), i.e. for every tile too big to have a few copies in LDS
        const int grt = (4 / MT) > 0 ? 4 / MT : 1;
        if (cb.var == VAR_GLOBAL || (size_t)Lb.total * 4 > 36 * 1024) scratch = (size_t)kGlobalTileGrid * grt * Lb.total * 4;
        if (cf.var == VAR_GLOBAL || (size_t)Lf.total * 4 > 36 * 1024) {
            const size_t s2 = (size_t)kGlobalTileGrid * grt * Lf.total * 4;
            scratch = s2 > scratch ? s2 : scratch;
        }
    }
    return (bytes + scratch + 15) & ~(size_t)15;
}

}  // namespace csmpn
