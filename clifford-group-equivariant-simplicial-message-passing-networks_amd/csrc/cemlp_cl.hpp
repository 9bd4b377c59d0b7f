// (row, channel)-per-lane ("cl") CEMLP kernels for Cl(3,0) layers whose blocks are all C = 8 channels wide.
//
// Same arithmetic as cemlp_device.hpp / cemlp_rl.hpp (csmpn/models/cegnn_utils.py:34-155,287-338; SURVEY.md
// Appendix A); the mapping onto the hardware is chosen for OCCUPANCY: the row-per-lane-group kernels (cemlp_rl.hpp)
// keep 4 channels x 8 blades of every live tensor in a lane (32 registers per tensor, ~500 in the backward, one
// wave per SIMD, 45 % issue-active). Here
//
//  * lane = (row r, channel c): a tensor is `float t[8]` (the 8 blades). A wave covers 64 / C rows (8 rows at
//    8 channels); two rows are interleaved inside a 16-lane DPP row (lane = r0 | c << 1 | r_hi << 4) so that
//    `row_ror:2k` rotates the channels of a row. Forward ~100 registers (4 waves per SIMD), one block of the
//    backward ~200 including its persistent gradient sums (2 waves per SIMD).
//  * dense channel mixing  out[r,o,d] = sum_c W[o][c][grade d] x[r,c,d]  is C rotations x 8 blades of
//    `v_fmac_f32_dpp` (the rotated operand costs no instruction of its own): lane (r,o) multiplies the value of
//    lane (r, o + k) with W[o][o + k][g], read as ONE ds_read_b128 (4 grades) per rotation from a rotation-ordered
//    LDS table [k][o] built once per workgroup from the reference layout [o][c][g]. Measured (tools/dpp_probe.hip,
//    profiles/r03_dpp_probe.log): a DPP VALU instruction issues at HALF the plain VALU rate on gfx950 (4.2 against
//    2.4 cycles), so the mixing runs at ~15 MAC/cycle/SIMD where the 4x4x1 MFMA of cemlp_rl.hpp reaches ~26 - the
//    price of one channel per lane; it is paid back by occupancy, by the absence of any LDS round trip between
//    phases and by the weight-gradient form below. Input segments narrower than C (the attribute channels) are
//    replicated with their power-of-two period, so a 6-channel segment takes 8 and a 3-channel segment 4 rotations.
//  * weight gradients take the lane layout AS IT IS: v_mfma_f32_16x16x4_f32 with A = this lane's gradient blade and
//    B = this lane's input blade contracts over the lane bits 4-5 = r_hi; D[(o,r0)][(c,r0')] is the wanted sum on
//    r0 = r0' (half of the tile, the other half is discarded). One MFMA per (matrix, blade), no LDS transposition,
//    accumulators (4 grades x f4 per matrix) persistent over the tile loop.
//  * per-channel parameter gradients are lane-private running sums in LDS (the lane's channel is fixed; ClSums);
//    the sum over the rows of the WORKGROUP happens once per block, at its end, behind the barrier the end phase has anyway:
//    owner threads read the 32 sums of a channel (4 waves x 8 rows) where they lie and write the slice's entry.
//  * the backward is ONE launch for all blocks, run block by block (last block first): 48-80 accumulator registers +
//    35 running sums are alive per block instead of both blocks' at once; d/d(block input) rows travel through a
//    [rows, C, D] region behind the saved block inputs (through L2: a wave reads in block k - 1 what it wrote itself
//    in block k) or, with one tile per wave, stay in registers. One tile per wave (S1's node launch) is an instantiation
//    of its own inside the kernel (cl_bwd_blocks<..., SINGLE>): what it pays is latency, so every global read of the
//    launch - tables of both blocks, tile indices, the last block's rows - is requested before the first wait, block 0's
//    rows travel during block 1's end phase and no store is waited for. Every workgroup writes one slice of partial sums per
//    block; cl_reduce_kernel adds the slices of all blocks in a fixed order (no atomics on parameters: bit-reproducible).
//  * gathers: a lane loads its own 32 bytes of a row (2 x 16 bytes); scatters go through a per-wave LDS tile so that
//    one atomic instruction covers whole 256-byte rows, equal consecutive targets summed first.
//  * addressing: every array of a launch is a raw buffer resource and a lane's address a 32-bit byte offset (ClBuf); the
//    range check of the resource is the tail predication of the stores (no array of a launch above kClMaxArrayBytes: the
//    launch condition, launch.hpp).
#pragma once
#include "cemlp_lane.hpp"

namespace csmpn {

constexpr int kClWaves = 4;          // waves per workgroup
constexpr int kClSliceCap = 512;     // workgroups of a backward launch = slices of partial sums per block
constexpr int kClParStride = 36;     // floats per channel in the per-channel parameter table

// Ordering point between LDS accesses of DIFFERENT lanes of one wave (a lane stores into the per-wave staging tile, another
// lane reads those bytes; and the next tile's stores behind those reads): the LDS executes a wave's operations in issue
// order, so no wait is needed - but the compiler sees each lane's own stores and loads as disjoint addresses and may move
// them across each other (cemlp_cm.hpp met exactly that). A compiler barrier + the wave-barrier intrinsic (a scheduling
// barrier, no instruction) state the contract at every such hand-over.
#define CL_LDS_ORDER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); asm volatile("" ::: "memory"); } while (0)

// ---------------------------------------------------------------------------------
// Addressing. An array of a launch is a raw buffer resource, built once per kernel from launch-uniform values (base in
// SGPRs, num_records = its size in bytes); a lane addresses it with a 32-bit BYTE offset: (row or index) * row bytes + the
// lane's place in the row, the latter worked out once per kernel. An access costs at most one 32-bit multiply-add - the
// 64-bit address per lane and access of a flat load took three to four vector instructions. The hardware's range check
// is the tail predication: a store whose offset is not below num_records is dropped (a load reads zero), so the rows
// behind the last one of a partial tile store without a branch or a select - their offsets lie behind the array, or
// are kClNoStore where the layout (state regions) interleaves them with valid rows. No offset of a launch wraps:
// cl_eligible admits arrays of at most kClMaxArrayBytes (launch.hpp).
typedef unsigned cl_u4 __attribute__((ext_vector_type(4)));
constexpr unsigned kClNoStore = 0xFF000000u;   // = kClMaxArrayBytes: behind every array, and 16 MiB short of a wrap
constexpr int kClStream = 2;                   // the instruction's `nt` bit: rows written once and read once (state regions)
struct ClBuf {
    __amdgpu_buffer_rsrc_t r;
    CSMPN_DEV ClBuf() : r(__builtin_amdgcn_make_buffer_rsrc(nullptr, 0, 0, 0x00020000)) {}
    // bytes <= kClMaxArrayBytes (the launch condition); a null array has no records
    CSMPN_DEV ClBuf(const void* base, size_t bytes)
        : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, base ? (int)(unsigned)bytes : 0, 0x00020000)) {}
    template <int AUX = 0>
    CSMPN_DEV f4 ld4(unsigned off) const { return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, AUX)); }
    CSMPN_DEV int ldi(unsigned off) const { return (int)__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0); }
    template <int AUX = 0>
    CSMPN_DEV void st4(unsigned off, f4 v) const { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(cl_u4, v), r, (int)off, 0, AUX); }
    // the lane's 8 blades = 32 contiguous bytes of a row
    CSMPN_DEV void st8(unsigned off, const float (&x)[8]) const {
        st4(off, f4{x[0], x[1], x[2], x[3]});
        st4(off + 16, f4{x[4], x[5], x[6], x[7]});
    }
};

// diagnostic build only (-DCSMPN_STAMPS, never shipped, never timed): shader-clock cycles per phase, summed per wave.
// The scheduling barriers at a stamp forbid overlaps across phases (memory operations stay in flight: a phase is
// charged with the waits it executes): the output is a breakdown, not a duration.
struct ClStamp {
#ifdef CSMPN_STAMPS
    static constexpr int kSlots = 24;
    unsigned long long t0, acc[kSlots];
    CSMPN_DEV explicit ClStamp(int) {
#pragma unroll
        for (int i = 0; i < kSlots; ++i) acc[i] = 0;
        t0 = __builtin_amdgcn_s_memtime();
    }
    CSMPN_DEV void operator()(int id) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        acc[id] += t1 - t0;
        t0 = t1;
        __builtin_amdgcn_sched_barrier(0);
    }
    CSMPN_DEV void flush(unsigned long long* out, int lane) {
        if (out && lane == 0) {
#pragma unroll
            for (int i = 0; i < kSlots; ++i) atomicAdd(out + i, acc[i]);
            atomicAdd(out + kSlots, 1ull);
        }
    }
#else
    CSMPN_DEV explicit ClStamp(int) {}
    CSMPN_DEV void operator()(int) {}
    CSMPN_DEV void flush(unsigned long long*, int) {}
#endif
};

// ---------------------------------------------------------------------------------
// lane <-> (row, channel)
template <int C>
struct ClMap {
    static_assert(C == 8 || C == 16, "8 or 16 channels");
    static constexpr int RPW = 64 / C;             // rows per wave
    static constexpr int ROTL = C == 8 ? 2 : 1;    // lanes per channel step inside a DPP row
    static CSMPN_DEV int chan(int lane) { return C == 8 ? (lane >> 1) & 7 : lane & 15; }
    static CSMPN_DEV int row(int lane) { return C == 8 ? (lane & 1) | ((lane >> 4) << 1) : lane >> 4; }
    static constexpr int lane_of_row(int r) { return C == 8 ? ((r >> 1) << 4) | (r & 1) : r << 4; }   // its channel-0 lane
};

template <int CTRL>
CSMPN_DEV int cl_dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, true); }

// sum over the C lanes that hold the channels of one row; result in every lane
template <int C>
CSMPN_DEV float cl_chan_sum(float v) {
    if constexpr (C == 16) v += dpp_mov<0x121>(v);
    v += dpp_mov<0x122>(v);
    v += dpp_mov<0x124>(v);
    v += dpp_mov<0x128>(v);
    return v;
}

// acc[d] += w[grade d] * (x[d] of the lane ROT lanes away in the DPP row), the 8 blades of Cl(3,0): grades 0 1 1 1 2 2 2 3.
// Inline asm: hipcc folds a DPP move into v_add / v_mul but not into v_fmac. The statement is opaque to the hazard
// recognizer (a VALU write of a VGPR needs two wait states before a DPP read of it), hence the s_nop in front: whatever
// the compiler places before the statement - the producers of x or a register copy of its own - is covered.
template <int ROT>
CSMPN_DEV void cl_fmac8(float (&acc)[8], const float (&x)[8], f4 w) {
    static_assert(ROT >= 0 && ROT < 16, "rotation inside a DPP row");
    if constexpr (ROT == 0) {
        acc[0] = __builtin_fmaf(x[0], w.x, acc[0]);
        acc[1] = __builtin_fmaf(x[1], w.y, acc[1]); acc[2] = __builtin_fmaf(x[2], w.y, acc[2]); acc[3] = __builtin_fmaf(x[3], w.y, acc[3]);
        acc[4] = __builtin_fmaf(x[4], w.z, acc[4]); acc[5] = __builtin_fmaf(x[5], w.z, acc[5]); acc[6] = __builtin_fmaf(x[6], w.z, acc[6]);
        acc[7] = __builtin_fmaf(x[7], w.w, acc[7]);
    } else {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %8, %16 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %1, %9, %17 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %2, %10, %17 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %3, %11, %17 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %4, %12, %18 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %5, %13, %18 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %6, %14, %18 row_ror:%20 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %7, %15, %19 row_ror:%20 row_mask:0xf bank_mask:0xf"
            : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7])
            : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]),
              "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w), "n"(ROT));
    }
}

// acc += (table at float offset TOFF: NROT rotations x C lanes of f4) applied to x. ldsw = LDS + 4 * (this lane's channel).
// The weight vectors are read BATCH at a time, all of a batch in flight before the first is used (the empty volatile
// asm statement takes their results: left alone, the scheduler reads each vector right in front of its rotation and
// waits out an LDS round trip per rotation - 49 exposed round trips per backward tile at two waves per SIMD).
template <int NK>
CSMPN_DEV void cl_pin(f4 (&w)[NK]) {
    if constexpr (NK == 8) asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]));
    else if constexpr (NK == 4) asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
    else if constexpr (NK == 2) asm volatile("" : "+v"(w[0]), "+v"(w[1]));
    else static_assert(NK == 1 || NK == 2 || NK == 4 || NK == 8, "batch size");
}
template <int C, int NROT, int TOFF, int BATCH = 4>
CSMPN_DEV void cl_mix(float (&acc)[8], const float (&x)[8], const float* ldsw) {
    static_assert(NROT % BATCH == 0, "whole batches");
    constexpr int NB = NROT / BATCH;
    f4 w[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; ++i) w[i] = ld4(ldsw + (TOFF + 4 * C * i));
    cl_pin<BATCH>(w);
    static_for<0, NB>([&](auto b) {
        // the next batch travels while this one is used
        f4 wn[BATCH];
        if constexpr (b + 1 < NB) {
#pragma unroll
            for (int i = 0; i < BATCH; ++i) wn[i] = ld4(ldsw + (TOFF + 4 * C * (BATCH * (b + 1) + i)));
        }
        static_for<0, BATCH>([&](auto i) { cl_fmac8<ClMap<C>::ROTL * (BATCH * b + i)>(acc, x, w[i]); });
        if constexpr (b + 1 < NB) {
            cl_pin<BATCH>(wn);
#pragma unroll
            for (int i = 0; i < BATCH; ++i) w[i] = wn[i];
        }
    });
}

// ---------------------------------------------------------------------------------
// compile-time description of one block's input passes and of its LDS tables (float offsets from the block's base)
constexpr int cl_pow2_ge(int w) { int p = 1; while (p < w) p <<= 1; return p; }

// block K of a CEMLP in mode MODE with NA attribute channels: K = 0 concatenates the mode's input segments (each one a
// "pass" of at most C channels), later blocks have one pass of C channels
template <int C, int MODE, int NA, int K, bool BWD>
struct ClTab {
    static constexpr int NSEG = MODE == MODE_EDGE ? 1 : (MODE == MODE_NODE ? 2 : 0);   // full-width segments in front of the attributes
    static_assert(MODE == MODE_EDGE || MODE == MODE_NODE, "edge or node program");
    static constexpr int NP = K > 0 ? 1 : NSEG + (NA > 0 ? 1 : 0);
    static constexpr int width(int p) { return (K > 0 || p < NSEG) ? C : NA; }
    static constexpr int period(int p) { return (K > 0 || p < NSEG) ? C : cl_pow2_ge(NA); }
    static constexpr int coff(int p) { return C * p; }
    static constexpr int I = K > 0 ? C : NSEG * C + NA;
    static_assert(NA <= C, "attribute segment wider than the layer");
    static constexpr int W1(int p) { int o = 0; for (int q = 0; q < p; ++q) o += 4 * C * period(q); return o; }
    static constexpr int WR = W1(NP), WL = WR + 4 * C * C;
    static constexpr int fwd_end = WL + 4 * C * C;
    static constexpr int W1T(int p) { return fwd_end + 4 * C * C * p; }
    static constexpr int WRT = W1T(NP), WLT = WRT + 4 * C * C;
    static constexpr int par = BWD ? WLT + 4 * C * C : fwd_end;
    static constexpr int total = par + C * kClParStride;
    // number of f4 table entries (everything in front of `par`)
    static constexpr int n_entries = par / 4;
};

// forward state of one block kept for its backward
// offset of (row, channel)'s first piece inside a state region (CSMPN_FLAG_SAVE_STATE, cemlp_device.hpp): a tile is 64 / C rows
// = 64 (row, channel) positions; piece e (4 blades) of position l lies at (tile * 2 + e) * 256 + 4 l floats
// In bytes: a tile's pieces start kClStateTile bytes behind the previous tile's; the lane's place cl_state_lane inside
// piece 0 is fixed for the kernel, piece 1 lies kClStatePiece bytes further.
constexpr unsigned kClStateTile = 2048, kClStatePiece = 1024;
template <int C>
CSMPN_DEV unsigned cl_state_lane(int r, int c) { return 16u * (unsigned)(r * C + c); }
struct ClFwd {
    float y[8], gate[4], R[8], invden[4], s[8];
    float qs, nl, invMn;
};

CSMPN_DEV float cl_smooth_abs_sqrt(float q) { return sqrt_pos(sqrt_pos(__builtin_fmaf(q, q, kSmooth))); }

// ---------------------------------------------------------------------------------
// parameters -> LDS tables of one block (once per workgroup). dir = +1 / -1: the lane `row_ror:ROTL` reads from holds
// channel c + dir (probed on the device).
// Two steps - load: every global read of the block requested; store: into LDS - so that a kernel requests the tables of all
// its blocks before it waits for the first (one global round trip per launch instead of one per block).
// Every wave of a launch runs this before its first tile, all of them at the same time: it is priced in issue slots like the
// tile loop. So the work is dealt out in units a wave can address without per-lane decisions. A weight table is a sequence
// of PIECES of (at most) 64 entries - one rotation-ordered [k][o] image of one matrix (or input pass of W1), plain or
// transposed - and piece q belongs to wave q mod 4: which matrix, its row stride, its first channel, period and width
// are scalars chosen by the wave index, the lane's entry is (k, o) = (lane / C, lane mod C) in every piece, and an entry
// without a source (a replicated attribute channel past the width) is an offset behind the matrix: the range check reads
// it as the zero the table holds there. The per-channel parameters are dealt out likewise: wave 0 the path weights, wave 1
// the three gate / normalisation vectors, wave 2 the three per-channel scalars.
template <class ALG, int C, class TB, bool BWD>
struct ClStage {
    static constexpr int G = ALG::G, P = ALG::P, NP = TB::NP;
    static_assert(G == 4, "the weight of one (o, c) pair is one 16-byte vector of 4 grades");
    static_assert(16 + P <= kClParStride && P % 4 == 0, "parameter stride; path weights as 16-byte vectors");
    static_assert(C * C == 64, "a piece is one wave's worth of entries");
    static_assert(kClWaves >= 3, "three waves share the per-channel parameters");
    static_assert(C * P / 4 <= 64, "one wave deals out the path weights, a 16-byte vector per lane");
    static_assert(16 + P == kClParStride, "a channel's parameter row has no padding behind the path weights: every float of it is staged");
    static constexpr int NQ = BWD ? 2 * NP + 4 : NP + 2, NSLOT = (NQ + kClWaves - 1) / kClWaves;
    struct Piece {
        const float* base;   // the matrix [rows][I][G]
        unsigned bytes;      // its size
        int e0, n;           // first f4 entry of the table, entries
        int stride, coff;    // bytes between rows of the matrix; bytes in front of the pass's first channel
        int pm, width;       // period - 1 (channel c of a narrow pass sits at c mod period), channels of the pass
        bool transposed;     // entry (k, c) = W[(c + dir k) mod C][c mod period] instead of (k, o) = W[o][(o + dir k) mod period]
    };
    template <int Q>
    static CSMPN_DEV Piece piece(const DevBlock& B) {
        static_assert(Q >= 0 && Q < NQ, "piece index");
        constexpr bool T = Q >= NP + 2;
        constexpr int q = T ? Q - (NP + 2) : Q;   // 0 .. NP - 1: pass of W1; NP: linear_right; NP + 1: linear_left
        if constexpr (q < NP) {
            return Piece{B.W1, (unsigned)(C * TB::I * G * 4), (T ? TB::W1T(q) : TB::W1(q)) / 4, T ? C * C : TB::period(q) * C, TB::I * G * 4,
                         TB::coff(q) * G * 4, TB::period(q) - 1, TB::width(q), T};
        } else {
            constexpr int e0 = (q == NP ? (T ? TB::WRT : TB::WR) : (T ? TB::WLT : TB::WL)) / 4;
            return Piece{q == NP ? B.WR : B.WL, (unsigned)(C * C * G * 4), e0, C * C, C * G * 4, 0, C - 1, C, T};
        }
    }
    f4 v[NSLOT], pw, psa, psb, pan;
    float pb1, pbL, pla;
    int dst[NSLOT];   // the lane's f4 entry of slot s (-1: none)
    // wave: the wave's index as a scalar
    __device__ void load(const DevBlock& B, int wave, int lane, int dir) {
        const int o = lane % C, k = lane / C, t = o + dir * k, t7 = t & (C - 1);
        static_for<0, NSLOT>([&](auto s) {
            Piece d{B.W1, 0u, 0, 0, 0, 0, 0, 0, false};   // no piece in this slot: no records, no entries
            static_for<0, kClWaves>([&](auto j) {
                constexpr int Q = kClWaves * decltype(s)::value + decltype(j)::value;
                if constexpr (Q < NQ) {
                    if (wave == j) d = piece<Q>(B);
                }
            });
            const int row = d.transposed ? t7 : o, col = (d.transposed ? o : t) & d.pm;
            const bool in_piece = lane < d.n;
            const unsigned off = in_piece && col < d.width ? (unsigned)(row * d.stride + d.coff + col * (G * 4)) : kClNoStore;
            v[s] = ClBuf(d.base, d.bytes).ld4(off);
            dst[s] = in_piece ? d.e0 + lane : -1;
        });
        // per-channel parameters: [b1, bL, la, 0 | sa[4] | sb[4] | sigmoid(an)[4] | w[P]] per channel. A lane that owns nothing
        // reads behind the array (no memory access, zeros)
        constexpr int NW = C * P / 4;   // 16-byte vectors of the path weights [C][P]
        const unsigned ow = wave == 0 && lane < NW ? 16u * lane : kClNoStore;
        const unsigned ov = wave == 1 && lane < C ? 16u * lane : kClNoStore;
        const unsigned os = wave == 2 && lane < C ? 4u * lane : kClNoStore;
        pw = ClBuf(B.w, C * P * 4).ld4(ow);
        psa = ClBuf(B.sa, C * G * 4).ld4(ov);
        psb = ClBuf(B.sb, C * G * 4).ld4(ov);
        pan = ClBuf(B.an, C * G * 4).ld4(ov);
        pb1 = __builtin_bit_cast(float, ClBuf(B.has_b1 ? B.b1 : nullptr, C * 4).ldi(os));
        pbL = __builtin_bit_cast(float, ClBuf(B.bL, C * 4).ldi(os));
        pla = __builtin_bit_cast(float, ClBuf(B.la, C * 4).ldi(os));
    }
    __device__ void store(float* base, int wave, int lane) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            if (dst[s] >= 0) st4(base + 4 * dst[s], v[s]);
        }
        float* par = base + TB::par;
        constexpr int NW = C * P / 4;
        if (wave == 0 && lane < NW) st4(par + (lane / (P / 4)) * kClParStride + 16 + 4 * (lane % (P / 4)), pw);
        if (wave == 1 && lane < C) {
            float* p = par + lane * kClParStride;
            st4(p + 4, psa);
            st4(p + 8, psb);
            st4(p + 12, f4{sigmoidf(pan.x), sigmoidf(pan.y), sigmoidf(pan.z), sigmoidf(pan.w)});
        }
        if (wave == 2 && lane < C) st4(par + lane * kClParStride, f4{pb1, pbL, pla, 0.f});
    }
};

// ---------------------------------------------------------------------------------
// sign-table geometric product with per-path weights, one channel:
//   out[j] += sum_{(i,k)->j} sign(i,k) * w[path(g_i, g_j, g_k)] * z[i] * r[k]
template <class ALG>
CSMPN_DEV void cl_weighted_gp(float (&out)[8], const float (&z)[8], const float (&r)[8], const float* wp) {
    constexpr int P = ALG::P;
    f4 wv[(P + 3) / 4];
#pragma unroll
    for (int q = 0; q < (P + 3) / 4; ++q) wv[q] = ld4(wp + 4 * q);
    static_for<0, P>([&](auto p) {
        constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
        constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
        constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
        constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
        const float w = wv[p / 4][p % 4];
        float tmp[nj];
#pragma unroll
        for (int t = 0; t < nj; ++t) tmp[t] = 0.f;
        static_for<0, ni>([&](auto ii) {
            static_for<0, nk>([&](auto kk) {
                constexpr int i = i0 + ii, k = k0 + kk;
                constexpr int j = ALG::t.out[i][k];
                if constexpr (j >= j0 && j < j0 + nj) {
                    constexpr float sg = float(ALG::t.sign[i][k]);
                    tmp[j - j0] += (sg * z[i]) * r[k];
                }
            });
        });
#pragma unroll
        for (int t = 0; t < nj; ++t) out[j0 + t] = __builtin_fmaf(w, tmp[t], out[j0 + t]);
    });
}

// the part of a block forward behind its MVLinear: S.y holds the MVLinear output (without bias)
template <class ALG, int C, class TB, int BATCH>
CSMPN_DEV void cl_block_tail(const float* ldsw, const float* ldsp, ClFwd& S, float (&out)[8], ClStamp& stamp, int sid, bool have_s = false) {
    constexpr int D = ALG::D, G = ALG::G;
    static_assert(D == 8 && G == 4, "Cl(3,0)-shaped algebra");
    const f4 p0 = ld4(ldsp + TB::par);   // b1, bL, la
    const f4 sa = ld4(ldsp + (TB::par + 4)), sb = ld4(ldsp + (TB::par + 8));
    S.y[0] += p0.x;
    // MVSiLU, invariant "mag2" (cegnn_utils.py:76-83)
    float z[D];
    static_for<0, G>([&](auto g) {
        constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
        float u;
        if constexpr (g == 0) {
            u = S.y[0];
        } else {
            u = 0.f;
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                u += qsf<ALG, d> * S.y[d] * S.y[d];
            });
        }
        S.gate[g] = sigmoidf(__builtin_fmaf(sa[int(g)], u, sb[int(g)]));
#pragma unroll
        for (int t = 0; t < nd; ++t) z[d0 + t] = S.gate[g] * S.y[d0 + t];
    });
    stamp(sid);
    // linear_right / linear_left (cegnn_utils.py:143-148)
    float L[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { S.R[d] = 0.f; L[d] = 0.f; }
    cl_mix<C, C, TB::WR, BATCH>(S.R, z, ldsw);
    // CSMPN_FLAG_SAVE_STATE: with s given (have_s: the forward saved it) the backward's recompute stops behind linear_right
    // and the normalisation denominators - no linear_left mix, no geometric product
    if (have_s) {
        const f4 sg = ld4(ldsp + (TB::par + 12));
        static_for<0, G>([&](auto g) {
            constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
            float qq = 0.f;
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                qq += qsf<ALG, d> * S.R[d] * S.R[d];
            });
            const float m = __builtin_fmaf(sg[int(g)], cl_smooth_abs_sqrt(qq) - 1.0f, 1.0f);
            S.invden[g] = fast_rcp(m + kEps);
        });
        float qs = 0.f;
        static_for<0, D>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            qs += qsf<ALG, d> * S.s[d] * S.s[d];
        });
        S.qs = qs;
        S.nl = cl_smooth_abs_sqrt(qs);
        S.invMn = fast_rcp(__builtin_fmaf(cl_chan_sum<C>(S.nl), 1.0f / float(C), kEps));
        return;
    }
    cl_mix<C, C, TB::WL, BATCH>(L, z, ldsw);
    stamp(sid + 1);
    L[0] += p0.y;
    // NormalizationLayer on the right operand (cegnn_utils.py:42-51)
    const f4 sg = ld4(ldsp + (TB::par + 12));
    float r[D];
    static_for<0, G>([&](auto g) {
        constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
        float qq = 0.f;
        static_for<0, nd>([&](auto t) {
            constexpr int d = d0 + decltype(t)::value;
            qq += qsf<ALG, d> * S.R[d] * S.R[d];
        });
        const float m = __builtin_fmaf(sg[int(g)], cl_smooth_abs_sqrt(qq) - 1.0f, 1.0f);
        S.invden[g] = fast_rcp(m + kEps);
#pragma unroll
        for (int t = 0; t < nd; ++t) r[d0 + t] = S.R[d0 + t] * S.invden[g];
    });
    stamp(sid + 2);
    // steerable geometric product + first-order term (cegnn_utils.py:126-152)
    cl_weighted_gp<ALG>(L, z, r, ldsp + (TB::par + 16));
    stamp(sid + 3);
#pragma unroll
    for (int d = 0; d < D; ++d) S.s[d] = L[d] * kInvSqrt2;
    // MVLayerNorm (cegnn_utils.py:93-96): mean over the C channels of the row
    float qs = 0.f;
    static_for<0, D>([&](auto dd) {
        constexpr int d = decltype(dd)::value;
        qs += qsf<ALG, d> * S.s[d] * S.s[d];
    });
    S.qs = qs;
    S.nl = cl_smooth_abs_sqrt(qs);
    S.invMn = fast_rcp(__builtin_fmaf(cl_chan_sum<C>(S.nl), 1.0f / float(C), kEps));
    const float k = p0.z * S.invMn;
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = k * S.s[d];
    stamp(sid + 4);
}


// ---------------------------------------------------------------------------------
// order of the per-channel parameter gradients in the lane-private running sums
template <class ALG>
struct ClRed {
    static constexpr int G = ALG::G, P = ALG::P;
    static constexpr int i_la = 0, i_bL = 1, i_w = 2, i_an = 2 + P, i_sa = 2 + P + G, i_b1 = 2 + P + 3 * G, n = 3 + 3 * G + P;
};
// slice of partial sums of one block launch: reference layouts [W1 [C][I][G] | WR [C][C][G] | WL | small], small =
// b1 [C], sa [C][G], sb [C][G], w [C][P], an [C][G], bL [C], la [C]
template <class ALG, int C, int I>
struct ClPart {
    static constexpr int G = ALG::G, P = ALG::P;
    static constexpr int pWR = C * I * G, pWL = pWR + C * C * G, pS = pWL + C * C * G;
    static constexpr int qb1 = 0, qsa = qb1 + C, qsb = qsa + C * G, qw = qsb + C * G, qan = qw + C * P, qbL = qan + C * G, qla = qbL + C;
    static constexpr int m_small = C * (3 + 3 * G + P);
    static constexpr int total = pS + m_small;
    using RM = ClRed<ALG>;
    // running-sum index -> (offset of the parameter's first element inside `small`, stride between channels)
    static constexpr int off(int idx) {
        if (idx == RM::i_la) return qla;
        if (idx == RM::i_bL) return qbL;
        if (idx < RM::i_an) return qw + (idx - RM::i_w);
        if (idx < RM::i_sa) return qan + (idx - RM::i_an);
        if (idx < RM::i_b1) return ((idx - RM::i_sa) & 1 ? qsb : qsa) + (idx - RM::i_sa) / 2;
        return qb1;
    }
    static constexpr int stride(int idx) {
        if (idx == RM::i_la || idx == RM::i_bL) return 1;
        if (idx < RM::i_an) return P;
        if (idx < RM::i_b1) return G;
        return 1;
    }
};

// Lane-private running sums of the per-channel parameter gradients, kept in LDS ([group of 4][thread] f4: registers are
// the scarce resource of the backward - 35 of them spilled MFMA accumulators to scratch). Values arrive in index
// order; every fourth one triggers a 16-byte read-modify-write (measured, tools/lds_probe.hip: 9 of them cost 63 ns per
// tile at two waves per SIMD; ds_add_f32 takes ~640 ns EACH).
template <int N>
struct ClSums {
    static constexpr int kGroups = (N + 3) / 4;
    static constexpr int floats_per_wg = kGroups * 4 * 64 * kClWaves;
    float* base;   // LDS, this thread's f4 of group 0; group g is 4 * 64 * kClWaves floats further
    f4 pend;
    CSMPN_DEV explicit ClSums(float* b) : base(b), pend{0.f, 0.f, 0.f, 0.f} {}
    CSMPN_DEV void zero() {
#pragma unroll
        for (int g = 0; g < kGroups; ++g) st4(base + g * (4 * 64 * kClWaves), f4{0.f, 0.f, 0.f, 0.f});
    }
    template <int IDX>
    CSMPN_DEV void add(float v) {
        pend[IDX % 4] = v;
        if constexpr (IDX % 4 == 3 || IDX == N - 1) {
            if constexpr (IDX % 4 != 3) {
#pragma unroll
                for (int i = IDX % 4 + 1; i < 4; ++i) pend[i] = 0.f;
            }
            float* p = base + (IDX / 4) * (4 * 64 * kClWaves);
            st4(p, ld4(p) + pend);
        }
    }
    template <int IDX>
    CSMPN_DEV float get() const { return base[(IDX / 4) * (4 * 64 * kClWaves) + IDX % 4]; }
};

// block backward. S: the block's recomputed forward state; gout: d/d(out) of this lane's (row, channel).
// Adds this tile's contributions to the persistent sums (sm: per-channel parameters, accR / accL: linear_right /
// linear_left weight tiles per grade) and leaves d/d(MVLinear output) in gy. The MVLinear weight gradient and the
// transposed MVLinear are the caller's (they need the block's input).
template <class ALG, int C, class TB>
CSMPN_DEV void cl_block_backward(const float* ldsw, const float* ldsp, const ClFwd& S, const float (&gout)[8], float (&gy)[8],
                                 ClSums<ClRed<ALG>::n>& sm, f4 (&accR)[ALG::G], f4 (&accL)[ALG::G], ClStamp& stamp, int sid) {
    constexpr int D = ALG::D, G = ALG::G, P = ALG::P;
    using RM = ClRed<ALG>;
    const f4 p0 = ld4(ldsp + TB::par);
    // ---- MVLayerNorm backward
    const float la = p0.z;
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) dot = __builtin_fmaf(gout[d], S.s[d], dot);
    sm.template add<RM::i_la>(dot * S.invMn);
    const float gMn = -cl_chan_sum<C>(la * dot) * S.invMn * S.invMn * (1.0f / float(C));   // d/d(mean norm) / C
    float ggp[D];   // = d/d(left) = d/d(gp)
    {
        const float inl = fast_rcp(S.nl);
        const float gqs = gMn * (0.5f * S.qs) * (inl * inl * inl);   // d nl / d qs = 0.5 qs / nl^3
        const float k0 = la * S.invMn;
        static_for<0, D>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            const float gs = __builtin_fmaf(k0, gout[d], gqs * (2.0f * qsf<ALG, d>) * S.s[d]);
            ggp[d] = gs * kInvSqrt2;
        });
    }
    sm.template add<RM::i_bL>(ggp[0]);
    // ---- d/dz from linear_left
    float gz[D];
#pragma unroll
    for (int d = 0; d < D; ++d) gz[d] = 0.f;
    stamp(sid);
    cl_mix<C, C, TB::WLT>(gz, ggp, ldsw);
    stamp(sid + 1);
    // ---- geometric product backward (gz, gr accumulate; d/dw per path)
    float gr[D], zf[D], rf[D];
#pragma unroll
    for (int d = 0; d < D; ++d) gr[d] = 0.f;
    static_for<0, D>([&](auto d) {
        zf[d] = S.gate[ALG::grade(d)] * S.y[d];
        rf[d] = S.R[d] * S.invden[ALG::grade(d)];
    });
    {
        f4 wv[(P + 3) / 4];
#pragma unroll
        for (int q = 0; q < (P + 3) / 4; ++q) wv[q] = ld4(ldsp + (TB::par + 16 + 4 * q));
        static_for<0, P>([&](auto p) {
            constexpr int gi = ALG::t.path_g[p][0], gj = ALG::t.path_g[p][1], gk = ALG::t.path_g[p][2];
            constexpr int i0 = ALG::gstart(gi), ni = ALG::gsize(gi);
            constexpr int j0 = ALG::gstart(gj), nj = ALG::gsize(gj);
            constexpr int k0 = ALG::gstart(gk), nk = ALG::gsize(gk);
            const float w = wv[p / 4][p % 4];
            // U[i] = sum sign ggp[j] r[k] (unweighted d/dz), V[k] = sum sign ggp[j] z[i] (unweighted d/dr)
            float U[ni], V[nk];
#pragma unroll
            for (int t = 0; t < ni; ++t) U[t] = 0.f;
#pragma unroll
            for (int t = 0; t < nk; ++t) V[t] = 0.f;
            static_for<0, ni>([&](auto ii) {
                static_for<0, nk>([&](auto kk) {
                    constexpr int i = i0 + ii, k = k0 + kk;
                    constexpr int j = ALG::t.out[i][k];
                    if constexpr (j >= j0 && j < j0 + nj) {
                        constexpr float sg = float(ALG::t.sign[i][k]);
                        U[ii] += (sg * ggp[j]) * rf[k];
                        V[kk] += (sg * ggp[j]) * zf[i];
                    }
                });
            });
            float gwv = 0.f;
#pragma unroll
            for (int t = 0; t < ni; ++t) { gz[i0 + t] = __builtin_fmaf(w, U[t], gz[i0 + t]); gwv = __builtin_fmaf(zf[i0 + t], U[t], gwv); }
#pragma unroll
            for (int t = 0; t < nk; ++t) gr[k0 + t] = __builtin_fmaf(w, V[t], gr[k0 + t]);
            sm.template add<RM::i_w + p>(gwv);
        });
    }
    stamp(sid + 2);
    // ---- NormalizationLayer backward -> gR
    const f4 sgv = ld4(ldsp + (TB::par + 12));
    float gR[D];
    static_for<0, G>([&](auto g) {
        constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
        float gden = 0.f, qR = 0.f;
        static_for<0, nd>([&](auto t) {
            constexpr int d = d0 + decltype(t)::value;
            gden -= gr[d] * S.R[d];
            qR += qsf<ALG, d> * S.R[d] * S.R[d];
        });
        gden *= S.invden[g] * S.invden[g];      // d/d(den): -sum gr * R / den^2
        const float nu = cl_smooth_abs_sqrt(qR);
        const float sg = sgv[int(g)];
        sm.template add<RM::i_an + g>(gden * (nu - 1.0f) * sg * (1.0f - sg));
        const float inu = fast_rcp(nu);
        const float gq = (gden * sg) * (0.5f * qR) * (inu * inu * inu);
        static_for<0, nd>([&](auto t) {
            constexpr int d = d0 + decltype(t)::value;
            gR[d] = __builtin_fmaf(gr[d], S.invden[g], gq * (2.0f * qsf<ALG, d>) * S.R[d]);
        });
    });
    stamp(sid + 3);
    cl_mix<C, C, TB::WRT>(gz, gR, ldsw);
    stamp(sid + 4);
    // ---- weight gradients of linear_right and linear_left on the MFMA, B = z = gate * y
#ifndef CL_X_NOMFMA
    static_for<0, D>([&](auto d) {
        constexpr int g = ALG::grade(d);
        accR[g] = mfma16(gR[d], zf[d], accR[g]);
        accL[g] = mfma16(ggp[d], zf[d], accL[g]);
    });
#else
    static_for<0, D>([&](auto d) { constexpr int g = ALG::grade(d); accR[g][0] += gR[d] * zf[d]; accL[g][0] += ggp[d] * zf[d]; });
#endif
    stamp(sid + 5);
    // ---- MVSiLU backward -> gy
    const f4 sa = ld4(ldsp + (TB::par + 4));
    static_for<0, G>([&](auto g) {
        constexpr int d0 = ALG::gstart(g), nd = ALG::gsize(g);
        float ggate = 0.f;
#pragma unroll
        for (int t = 0; t < nd; ++t) ggate = __builtin_fmaf(gz[d0 + t], S.y[d0 + t], ggate);
        const float gpre = ggate * S.gate[g] * (1.0f - S.gate[g]);
        float u;
        if constexpr (g == 0) {
            u = S.y[0];
        } else {
            u = 0.f;
            static_for<0, nd>([&](auto t) {
                constexpr int d = d0 + decltype(t)::value;
                u += qsf<ALG, d> * S.y[d] * S.y[d];
            });
        }
        sm.template add<RM::i_sa + 2 * g>(gpre * u);
        sm.template add<RM::i_sa + 2 * g + 1>(gpre);
        const float gu = gpre * sa[int(g)];
        static_for<0, nd>([&](auto t) {
            constexpr int d = d0 + decltype(t)::value;
            float v = gz[d] * S.gate[g];
            if constexpr (g == 0) v += gu;
            else v = __builtin_fmaf(gu * (2.0f * qsf<ALG, d>), S.y[d], v);
            gy[d] = v;
        });
    });
    sm.template add<RM::i_b1>(gy[0]);
    stamp(sid + 6);
}

// ---------------------------------------------------------------------------------
// per-lane row access: the lane's 8 blades = 32 contiguous bytes
CSMPN_DEV void cl_st8(float* p, const float (&x)[8]) {
    st4(p, f4{x[0], x[1], x[2], x[3]});
    st4(p + 4, f4{x[4], x[5], x[6], x[7]});
}

// Rows of a staged tile [RPW][ROWLEN + 4] -> atomic adds into table rows of ROWLEN floats; lane = column. The row
// targets travel through SGPRs (v_readlane of the channel-0 lane of the row). Adds the rows to table[t_add[row]] (rows
// sorted by that index: equal consecutive targets are summed first) and, when SUB, subtracts them from
// table[t_sub[row]] (unsorted). Negative targets are skipped.
template <int C, int ROWLEN, bool SUB>
CSMPN_DEV void cl_scatter(const float* sc, int t_add, int t_sub, float* table, int lane) {
    using MP = ClMap<C>;
    constexpr int RPW = MP::RPW, SS = ROWLEN + 4, NC = ROWLEN / 64;
    static_assert(ROWLEN % 64 == 0, "whole columns");
    static_for<0, NC>([&](auto cc) {
        const int colx = 64 * cc + lane;
        const float* col = sc + colx;
        auto flush = [&](int target, float a) {
            if (target >= 0) atomicAdd(table + (size_t)target * ROWLEN + colx, a);
        };
        float val[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) val[i] = col[i * SS];
        float acc = 0.f;
        int cur = __builtin_amdgcn_readlane(t_add, MP::lane_of_row(0));
        static_for<0, RPW>([&](auto rr) {
            const int t = __builtin_amdgcn_readlane(t_add, MP::lane_of_row(rr));
            if (t != cur) {
                flush(cur, acc);
                cur = t;
                acc = 0.f;
            }
            acc += val[rr];
        });
        flush(cur, acc);
        if constexpr (SUB) {
            static_for<0, RPW>([&](auto rr) { flush(__builtin_amdgcn_readlane(t_sub, MP::lane_of_row(rr)), -val[rr]); });
        }
    });
}

// ---------------------------------------------------------------------------------
// The input arrays of a launch and the lane's byte offsets into their rows (worked out once per kernel).
template <class ALG, int C, int MODE, int NA>
struct ClIn {
    static constexpr int D = ALG::D, RB = C * D * 4, AB = NA * D * 4;   // bytes of a full row / of an attribute row
    ClBuf a, b, at;   // edge: h (gathered by target), h (by source), edge attributes (by permutation); node: h, agg, node attributes
    ClBuf i0, i1, i2; // edge: a row's target, source, permutation; node: i0 = in-degree (no degrees: no records, reads 0 = scale 1)
    unsigned rows;    // rows of the launch
    unsigned lo, la;  // the lane's channel in a full row; in an attribute row: channel c mod period, clamped to a valid one
                      // (its table entries are zero where it is not)
    bool in_attr;     // c < NA: the lane owns a channel of the attribute gradient
    // edge program: the attribute table is indexed by the permutation, and a launch may cover a SLICE of the edge list
    // (graph segments, sharded layers) whose permutation points into the table of the whole list: its size is not the
    // launch's to know. It keeps a 64-bit address (one multiply-add per tile) and no range check.
    const float* attr;
    CSMPN_DEV ClIn(const RowIO& io, int c) {
        rows = (unsigned)io.rows;
        lo = (unsigned)c * (D * 4);
        const int ca = c & (cl_pow2_ge(NA > 0 ? NA : 1) - 1);
        la = (unsigned)(ca < NA ? ca : NA - 1) * (D * 4);
        in_attr = c < NA;
        const size_t rb = (size_t)rows * RB, ib = (size_t)rows * 4;
        if constexpr (MODE == MODE_EDGE) {
            const size_t tb = (size_t)io.gather_rows * RB;
            a = ClBuf(io.seg[0].a, tb); b = ClBuf(io.seg[0].b, tb);
            i0 = ClBuf(io.seg[0].ia, ib); i1 = ClBuf(io.seg[0].ib, ib);
            if constexpr (NA > 0) { attr = io.seg[1].a; i2 = ClBuf(io.seg[1].ia, ib); }
        } else {
            attr = nullptr;
            a = ClBuf(io.seg[0].a, rb); b = ClBuf(io.seg[1].a, rb);
            i0 = ClBuf(io.seg[1].deg, ib);
            if constexpr (NA > 0) at = ClBuf(io.seg[2].a, (size_t)rows * AB);
        }
    }
    // a lane's offset in a [rows, C, D] array of the launch. A row behind the last one lies behind the array: its store is
    // dropped, its load reads zero
    CSMPN_DEV unsigned row_off(unsigned row) const { return row * RB + lo; }
};

// tile bookkeeping shared by the kernels
template <int C, int MODE>
struct ClTile {
    unsigned row, lrow;
    bool valid;
    int i_dst, i_src, i_perm, deg;
    // mean aggregation. Worked out where it is used: taken at load time, the division waits out the degree's round trip in
    // front of the row requests that follow the load
    CSMPN_DEV float scale() const { return 1.0f / float(deg > 1 ? deg : 1); }
    template <class ALG, int NA>
    CSMPN_DEV void load(const ClIn<ALG, C, MODE, NA>& in, unsigned tile, int r) {
        row = tile * ClMap<C>::RPW + r;
        valid = row < in.rows;
        lrow = valid ? row : 0;   // lanes past the end compute on row 0 and contribute nothing
        i_dst = i_src = i_perm = 0;
        deg = 1;
        if constexpr (MODE == MODE_EDGE) {
            i_dst = in.i0.ldi(4 * lrow);
            i_src = in.i1.ldi(4 * lrow);
            if constexpr (NA > 0) i_perm = in.i2.ldi(4 * lrow);
        }
        if constexpr (MODE == MODE_NODE) deg = in.i0.ldi(4 * lrow);   // mean aggregation
    }
};

// The gathered input passes of block 0, in two steps so that every load of a tile is in flight at once (left to the
// scheduler, the attribute loads were issued behind the wait for the feature rows: three dependent round trips per
// tile at two waves per SIMD). issue: raw 16-byte pieces; finish: x[p] = this lane's channel of pass p.
template <class ALG, int C, int MODE, int NA>
struct ClRaw {
    static constexpr int NSEG = MODE == MODE_EDGE ? 2 : 2;   // edge: h[dst], h[src]; node: h, agg
    using IN = ClIn<ALG, C, MODE, NA>;
    f4 v[2 * (NSEG + (NA > 0 ? 1 : 0))];
    CSMPN_DEV void issue(const IN& in, const ClTile<C, MODE>& T) {
        unsigned o0, o1, o2 = 0;
        if constexpr (MODE == MODE_EDGE) {
            o0 = (unsigned)T.i_dst * IN::RB + in.lo;
            o1 = (unsigned)T.i_src * IN::RB + in.lo;
        } else {
            o0 = o1 = in.row_off(T.lrow);
            if constexpr (NA > 0) o2 = T.lrow * IN::AB + in.la;
        }
        v[0] = in.a.ld4(o0); v[1] = in.a.ld4(o0 + 16);
        v[2] = in.b.ld4(o1); v[3] = in.b.ld4(o1 + 16);
        if constexpr (NA > 0 && MODE == MODE_EDGE) {
            const float* p2 = in.attr + ((size_t)(unsigned)T.i_perm * (IN::AB / 4) + in.la / 4);
            v[4] = ld4(p2); v[5] = ld4(p2 + 4);
        } else if constexpr (NA > 0) {
            v[4] = in.at.ld4(o2); v[5] = in.at.ld4(o2 + 16);
        }
    }
    // all of them requested before the first is used
    CSMPN_DEV void pin() {
        if constexpr (NA > 0) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
        else asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
    }
    template <class TB>
    CSMPN_DEV void finish(float (&x)[TB::NP][8], const ClTile<C, MODE>& T) const {
        auto unpack = [&](float (&t)[8], const f4& a, const f4& b) {
            t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
        };
        if constexpr (MODE == MODE_EDGE) {
            const f4 a = v[0] - v[2], b = v[1] - v[3];
            unpack(x[0], a, b);
            if constexpr (NA > 0) unpack(x[1], v[4], v[5]);
        } else {
            unpack(x[0], v[0], v[1]);
            const float sc_ = T.scale();
            unpack(x[1], v[2] * sc_, v[3] * sc_);
            if constexpr (NA > 0) unpack(x[2], v[4], v[5]);
        }
    }
};

template <int C>
CSMPN_DEV int cl_probe_dir(int c) {
    const int probe = cl_dpp_i<0x120 + ClMap<C>::ROTL>(c);
    return (((probe - c) & (C - 1)) == 1) ? 1 : -1;
}

// ---------------------------------------------------------------------------------
// forward kernel: NBLK blocks (1 or 2), all C channels wide. Tile t (64 / C rows) belongs to wave t mod (4 gridDim).
template <class ALG, int C, int MODE, int NBLK, int NA>
__global__ void __launch_bounds__(64 * kClWaves, 4) cemlp_cl_fwd_kernel(const DevCemlp C_arg, const RowIO io_arg) {
    CSMPN_KERNEL_ARGS(Cd);
    using MP = ClMap<C>;
    using T0 = ClTab<C, MODE, NA, 0, false>;
    using T1 = ClTab<C, MODE, NA, 1, false>;
    constexpr int D = ALG::D, ROW = C * D, RPW = MP::RPW, SS = ROW + 4;
    static_assert(NBLK == 1 || NBLK == 2, "one or two blocks");
    constexpr int tab_floats = T0::total + (NBLK > 1 ? T1::total : 0);
    constexpr int kBatch = 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lds = smem;
    // the wave index as the scalar it is: tile numbers, the loop and the tile's part of an offset stay on the scalar unit
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c = MP::chan(lane), r = MP::row(lane);
    float* sc = lds + tab_floats + wave * (RPW * SS);   // scatter staging tile (edge program)
    ClStamp stamp(0);
    using IN = ClIn<ALG, C, MODE, NA>;
    constexpr int RB = IN::RB;
    const IN in(io, c);
    const float* ldsw0 = lds + 4 * c;
    const float* ldsp0 = lds + kClParStride * c;
    const float* ldsw1 = ldsw0 + T0::total;
    const float* ldsp1 = ldsp0 + T0::total;

    const unsigned ntiles = (in.rows + RPW - 1) / RPW;
    const unsigned tstride = gridDim.x * kClWaves;
    const bool save_s = NBLK > 1 && io.save_state != 0 && io.save != nullptr;
    // outputs: [rows, C, D] arrays (a row behind the last one is dropped by the range check) and the state regions
    const size_t row_bytes = (size_t)in.rows * RB, state_bytes = state_rows(io.rows) * (size_t)RB;
    const ClBuf b_save(io.save, row_bytes);
    const ClBuf b_s0(save_s ? io.save + state_region<ROW, ROW>(io.rows, 0, 0) : nullptr, state_bytes);
    const ClBuf b_s1(save_s ? io.save + state_region<ROW, ROW>(io.rows, 0, 1) : nullptr, state_bytes);
    const ClBuf b_out(MODE == MODE_EDGE ? (io.row_store ? io.agg : nullptr) : io.y, row_bytes);
    const ClBuf b_res(MODE == MODE_NODE ? io.resid : nullptr, row_bytes);
    const unsigned st_lane = cl_state_lane<C>(r, c);
    // Software pipeline over the wave's tiles: the row pieces of tile t + 1 are requested (all together) BEFORE the stores
    // and atomics of tile t - vmcnt counts in issue order, a load behind an atomic waits for its acknowledgement
    // (~3000 cycles under load) - and the indices of tile t + 2 travel while tile t + 1 computes.
    const unsigned tile0 = blockIdx.x * kClWaves + wave;
    ClTile<C, MODE> T, Tn;
    T.load(in, tile0, r);
    ClRaw<ALG, C, MODE, NA> raw;
    raw.issue(in, T);
    Tn.load(in, tile0 + tstride, r);
    // the first tile's rows travel while the tables are staged
    {
        const int dir = cl_probe_dir<C>(c);
        ClStage<ALG, C, T0, false> st0;
        ClStage<ALG, C, T1, false> st1;
        st0.load(Cd.b[0], wave, lane, dir);
        if constexpr (NBLK > 1) st1.load(Cd.b[1], wave, lane, dir);
        st0.store(lds, wave, lane);
        if constexpr (NBLK > 1) st1.store(lds + T0::total, wave, lane);
    }
    __syncthreads();
    stamp(0);
    for (unsigned tile = tile0; tile < ntiles; tile += tstride) {
        raw.pin();
        stamp(1);
        // the residual row is requested here (most likely a cache hit: the node program has just read it as its first
        // segment) and not where it is added, at the end of the tile with nothing left to hide its round trip
        f4 res0, res1;
        if constexpr (MODE == MODE_NODE) {
            if (io.resid) {
                const unsigned o = in.row_off(T.lrow);
                res0 = b_res.ld4(o); res1 = b_res.ld4(o + 16);
            }
        }
        // the lane's place in the tile's state pieces; the rows behind the last one share their tile with valid rows: no store
        const unsigned st_off = T.valid ? tile * kClStateTile + st_lane : kClNoStore;
        float out[D], in1[D];
        {
            float x[T0::NP][D];
            raw.template finish<T0>(x, T);
            ClFwd S;
#pragma unroll
            for (int d = 0; d < D; ++d) S.y[d] = 0.f;
            static_for<0, T0::NP>([&](auto p) { cl_mix<C, T0::period(p), T0::W1(p), kBatch>(S.y, x[p], ldsw0); });
            stamp(2);
            cl_block_tail<ALG, C, T0, kBatch>(ldsw0, ldsp0, S, out, stamp, 3);
            if (save_s) {   // CSMPN_FLAG_SAVE_STATE: s of block 0 -> its state region (cemlp_device.hpp): whole tiles, two pieces per lane
                b_s0.template st4<kClStream>(st_off, f4{S.s[0], S.s[1], S.s[2], S.s[3]});       // streaming: read once, by the backward
                b_s0.template st4<kClStream>(st_off + kClStatePiece, f4{S.s[4], S.s[5], S.s[6], S.s[7]});
            }
        }
        if constexpr (NBLK > 1) {
#pragma unroll
            for (int d = 0; d < D; ++d) in1[d] = out[d];
            ClFwd S;
#pragma unroll
            for (int d = 0; d < D; ++d) S.y[d] = 0.f;
            cl_mix<C, C, T1::W1(0), kBatch>(S.y, in1, ldsw1);
            stamp(8);
            cl_block_tail<ALG, C, T1, kBatch>(ldsw1, ldsp1, S, out, stamp, 9);
            if (save_s) {   // ... s of block 1
                b_s1.template st4<kClStream>(st_off, f4{S.s[0], S.s[1], S.s[2], S.s[3]});
                b_s1.template st4<kClStream>(st_off + kClStatePiece, f4{S.s[4], S.s[5], S.s[6], S.s[7]});
            }
        }
        // next tile's rows, then this tile's stores
        const ClTile<C, MODE> Tc = T;
        T = Tn;
        raw.issue(in, T);
        Tn.load(in, tile + 2 * tstride, r);
        const unsigned o_row = in.row_off(Tc.row);
        if constexpr (NBLK > 1) {
            if (io.save) b_save.st8(o_row, in1);
        }
        if constexpr (MODE == MODE_EDGE) {
            if (io.row_store) {
                b_out.st8(o_row, out);
            } else {
                CL_LDS_ORDER();
                cl_st8(sc + r * SS + c * D, out);
                CL_LDS_ORDER();
                cl_scatter<C, ROW, false>(sc, Tc.valid ? Tc.i_dst : -1, -1, io.agg, lane);
            }
        } else {
            if (io.resid) {
                const float res[D] = {res0.x, res0.y, res0.z, res0.w, res1.x, res1.y, res1.z, res1.w};
#pragma unroll
                for (int d = 0; d < D; ++d) out[d] += res[d];
            }
            b_out.st8(o_row, out);
        }
        stamp(14);
    }
    stamp.flush(io.stamps, lane);
}
template <class ALG, int C, int MODE, int NBLK, int NA>
constexpr size_t cl_fwd_lds_bytes() {
    return sizeof(float) * (ClTab<C, MODE, NA, 0, false>::total + (NBLK > 1 ? ClTab<C, MODE, NA, 1, false>::total : 0) +
                            (MODE == MODE_EDGE ? kClWaves * ClMap<C>::RPW * (C * ALG::D + 4) : 0));
}

// ---------------------------------------------------------------------------------
// backward of block K (launched last block first). d/d(out of block K) comes from io.gy (last block; the edge program
// gathers it by target) or from the hand-over rows io.handover; d/d(input of block K) goes to the hand-over rows (K > 0)
// or to the program's gradient targets (K = 0). Block K > 0 reads its input from the saved rows.
struct ClCarry { f4 a, b; };
// The arrays of a backward launch beside its inputs, and the lane's offsets into them.
template <class ALG, int C, int MODE, int NA>
struct ClBwdIn : ClIn<ALG, C, MODE, NA> {
    using IN = ClIn<ALG, C, MODE, NA>;
    static constexpr int ROW = C * ALG::D;
    // d/d(out) (edge: [N] rows gathered by target) and the state regions. The arrays one block alone touches - saved block
    // inputs, hand-over rows, gradient targets - are built by that block: resources are four scalar registers each, and
    // with all of a launch's alive at once the backward runs out of them
    ClBuf gy, st0, st1;
    unsigned st_lane, st_row0;      // the lane's place in a tile's state piece; row 0's place (the rows behind the last one read it)
    CSMPN_DEV ClBwdIn(const RowIO& io, int c, int r) : IN(io, c) {
        const size_t rb = (size_t)this->rows * IN::RB, sb = state_rows(io.rows) * (size_t)IN::RB;
        gy = ClBuf(io.gy, MODE == MODE_EDGE ? (size_t)io.gather_rows * IN::RB : rb);
        st0 = ClBuf(io.saved + state_region<ROW, ROW>(io.rows, 0, 0), io.save_state ? sb : 0);
        st1 = ClBuf(io.saved + state_region<ROW, ROW>(io.rows, 0, 1), io.save_state ? sb : 0);
        st_lane = cl_state_lane<C>(r, c);
        st_row0 = cl_state_lane<C>(0, c);
    }
    // d/d(out) of the last block: a row behind the last one reads zero (it contributes nothing to any sum)
    CSMPN_DEV unsigned gy_off(const ClTile<C, MODE>& T) const {
        if constexpr (MODE == MODE_EDGE) return T.valid ? (unsigned)T.i_dst * IN::RB + this->lo : kClNoStore;
        else return this->row_off(T.row);
    }
    template <int K>
    CSMPN_DEV const ClBuf& state() const { if constexpr (K == 0) return st0; else return st1; }
    CSMPN_DEV unsigned state_off(const ClTile<C, MODE>& T) const {
        return T.valid ? (T.row / ClMap<C>::RPW) * kClStateTile + st_lane : st_row0;
    }
};
// What the first tile of a block reads from global memory, requested BEFORE the block starts: the last block's ahead of the
// table staging (as the forward does), block 0's - with one tile per wave - ahead of the end phase of the block in front
// of it. With one tile per wave every global round trip is exposed once per launch; here they travel behind work that
// is there anyway. d/d(out) of a block that is not the last is the caller's (hand-over rows or registers).
template <class ALG, int C, int MODE, int NBLK, int NA, bool SAVES>
struct ClBwdReq {
    f4 g0, g1, s0, s1, t0, t1;
    ClRaw<ALG, C, MODE, NA> raw;
    template <int K>
    CSMPN_DEV void request(const RowIO& io, const ClBwdIn<ALG, C, MODE, NA>& in, const ClTile<C, MODE>& Tl) {
        if constexpr (K == NBLK - 1) {
            const unsigned o = in.gy_off(Tl);
            g0 = in.gy.ld4(o); g1 = in.gy.ld4(o + 16);
        }
        if constexpr (K == 0) {
            raw.issue(in, Tl);
        } else {
            const ClBuf saved(io.saved, (size_t)in.rows * ClBwdIn<ALG, C, MODE, NA>::RB);
            const unsigned o = in.row_off(Tl.lrow);
            s0 = saved.ld4(o); s1 = saved.ld4(o + 16);
        }
        if constexpr (SAVES) {   // the block's saved state (row 0's for a wave without a tile: never used)
            const unsigned o = in.state_off(Tl);
            t0 = in.template state<K>().template ld4<kClStream>(o);
            t1 = in.template state<K>().template ld4<kClStream>(o + kClStatePiece);
        }
    }
    // block 0's requests have arrived (placed in front of stores whose acknowledgement nobody has to wait for: vmcnt counts
    // in issue order, a later wait for these rows would wait for those stores too)
    CSMPN_DEV void arrived0() {
        raw.pin();
        if constexpr (SAVES) asm volatile("" : "+v"(t0), "+v"(t1));
    }
};
// SINGLE: one tile per wave (uniform over the grid; an instantiation of its own inside the kernel: no tile loop, no next
// tile, and the waits the compiler places are exact instead of the loop's vmcnt(0)). T0: the wave's first tile (loaded once
// per launch). cur: the block's row registers; they hold the requests of T0 already for the last block and, when SINGLE,
// for every block. next: when SINGLE, receives the requests of T0 for block K - 1.
template <class ALG, int C, int MODE, int NBLK, int NA, int K, bool SAVES, bool SINGLE>
CSMPN_DEV ClCarry cl_bwd_block(const RowIO& io, const ClBwdIn<ALG, C, MODE, NA>& in, float* tab, float* work, const ClTile<C, MODE>& T0,
                               ClBwdReq<ALG, C, MODE, NBLK, NA, SAVES>& cur,
                               ClBwdReq<ALG, C, MODE, NBLK, NA, SAVES>& next, const ClCarry carry_in, ClStamp& stamp) {
    constexpr bool single = SINGLE, have_pre = SINGLE || K == NBLK - 1;
    f4 carry_a = carry_in.a, carry_b = carry_in.b;
    using MP = ClMap<C>;
    using TB = ClTab<C, MODE, NA, K, true>;
    using PT = ClPart<ALG, C, TB::I>;
    using RM = ClRed<ALG>;
    constexpr int D = ALG::D, G = ALG::G, ROW = C * D, RPW = MP::RPW, SS = ROW + 4, NP = TB::NP;
    static_assert(K >= 0 && K < NBLK && NBLK <= 2, "block index");
    constexpr bool kLast = K == NBLK - 1;
    // per-wave scratch: staging tile / image of the slice (the larger of the blocks' images: one layout for the launch)
    constexpr int img_max = NBLK > 1 && ClPart<ALG, C, C>::total > ClPart<ALG, C, ClTab<C, MODE, NA, 0, true>::I>::total
                                ? ClPart<ALG, C, C>::total : ClPart<ALG, C, ClTab<C, MODE, NA, 0, true>::I>::total;
    constexpr int scratch = (RPW * SS > img_max ? RPW * SS : img_max);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c = MP::chan(lane), r = MP::row(lane);
    float* sc = work + wave * scratch;
    const float* ldsw = tab + 4 * c;
    const float* ldsp = tab + kClParStride * c;

    // persistent sums of this wave
    f4 accW1[NP][G], accR[G], accL[G];
    ClSums<RM::n> sm(work + kClWaves * scratch + 4 * threadIdx.x);
    sm.zero();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        accR[g] = accL[g] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < NP; ++p) accW1[p][g] = f4{0.f, 0.f, 0.f, 0.f};
    }

    using IN = ClBwdIn<ALG, C, MODE, NA>;
    // this block's own arrays: saved block inputs and hand-over rows; gradient targets written by row (edge gx[0]: the
    // deterministic mode's [rows] table)
    const size_t row_bytes = (size_t)in.rows * IN::RB, attr_bytes = (size_t)in.rows * IN::AB;
    const ClBuf b_saved(K > 0 ? io.saved : nullptr, row_bytes);
    const ClBuf b_hand(NBLK > 1 && !single ? io.handover : nullptr, row_bytes);
    const ClBuf b_gx0(K > 0 ? nullptr : (MODE == MODE_EDGE && !io.row_store ? nullptr : io.gx[0]), row_bytes);
    const ClBuf b_gx1(K > 0 || MODE == MODE_EDGE ? nullptr : io.gx[1], row_bytes);
    const ClBuf b_gx2(K > 0 || MODE == MODE_EDGE ? nullptr : io.gx[2], attr_bytes);
    const unsigned ntiles = (in.rows + RPW - 1) / RPW;
    const unsigned tstride = gridDim.x * kClWaves;
    // Software pipeline as in the forward: the rows of tile t + 1 are requested in front of the stores / atomics of tile t.
    f4 &g0 = cur.g0, &g1 = cur.g1, &s0 = cur.s0, &s1 = cur.s1, &t0 = cur.t0, &t1 = cur.t1;
    ClRaw<ALG, C, MODE, NA>& raw = cur.raw;
    auto issue = [&](const ClTile<C, MODE>& Tl) {
        // d/d(out): zero for a row behind the last one (the hand-over rows end where the rows end)
        if constexpr (kLast) {
            const unsigned o = in.gy_off(Tl);
            g0 = in.gy.ld4(o); g1 = in.gy.ld4(o + 16);
        } else if constexpr (!single) {
            const unsigned o = in.row_off(Tl.row);
            g0 = b_hand.ld4(o); g1 = b_hand.ld4(o + 16);
        } else {   // one tile per wave: d/d(out) of this block stayed in registers
            g0 = carry_a; g1 = carry_b;
        }
        if constexpr (K == 0) {
            raw.issue(in, Tl);
        } else {
            const unsigned o = in.row_off(Tl.lrow);
            s0 = b_saved.ld4(o); s1 = b_saved.ld4(o + 16);
        }
    };
    const unsigned tile0 = blockIdx.x * kClWaves + wave;
    ClTile<C, MODE> T = T0, Tn = T0;
    if constexpr (have_pre) {
        if constexpr (!kLast) { g0 = carry_a; g1 = carry_b; }
    } else {
        issue(T);
    }
    if constexpr (!single) Tn.load(in, tile0 + tstride, r);
    stamp(20);
    for (unsigned tile = tile0; tile < ntiles; tile += tstride) {
        if constexpr (K == 0) {
            asm volatile("" : "+v"(g0), "+v"(g1));
            raw.pin();
        } else {
            asm volatile("" : "+v"(g0), "+v"(g1), "+v"(s0), "+v"(s1));
        }
        stamp(1);
        const ClTile<C, MODE> Tc = T;
        float gout[D] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        float x[NP][D];
        if constexpr (K == 0) {
            raw.template finish<TB>(x, Tc);
        } else {
            x[0][0] = s0.x; x[0][1] = s0.y; x[0][2] = s0.z; x[0][3] = s0.w; x[0][4] = s1.x; x[0][5] = s1.y; x[0][6] = s1.z; x[0][7] = s1.w;
        }
        float gy[D];
        {
            ClFwd S;
#pragma unroll
            for (int d = 0; d < D; ++d) S.y[d] = 0.f;
            constexpr bool have_s = SAVES;   // compile time: a run-time switch between the two recomputes spills the node program
            if constexpr (have_s) {   // CSMPN_FLAG_SAVE_STATE: the block's output in front of the layer norm, saved by the forward
                if (!have_pre || (!single && tile != tile0)) {
                    const unsigned o = in.state_off(Tc);
                    t0 = in.template state<K>().template ld4<kClStream>(o);
                    t1 = in.template state<K>().template ld4<kClStream>(o + kClStatePiece);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) { S.s[i] = t0[i]; S.s[4 + i] = t1[i]; }
            }
            static_for<0, NP>([&](auto p) { cl_mix<C, TB::period(p), TB::W1(p)>(S.y, x[p], ldsw); });
            stamp(2);
            float unused[D];
            cl_block_tail<ALG, C, TB, 4>(ldsw, ldsp, S, unused, stamp, 3, have_s);
            cl_block_backward<ALG, C, TB>(ldsw, ldsp, S, gout, gy, sm, accR, accL, stamp, 8);
        }
        // one tile per wave (registers to spare): the residual's gradient row travels behind the weight-gradient MFMAs and
        // the transposed mix
        f4 res0, res1;
        if constexpr (K == 0 && MODE == MODE_NODE && single) {
            if (io.gx[0] && io.resid_bwd) {
                const unsigned o = in.row_off(Tc.row);
                res0 = in.gy.ld4(o); res1 = in.gy.ld4(o + 16);
            }
        }
        // MVLinear weight gradient: A = gy, B = the pass's input blade
#ifndef CL_X_NOMFMA
        static_for<0, NP>([&](auto p) {
            static_for<0, D>([&](auto d) { accW1[p][ALG::grade(d)] = mfma16(gy[d], x[p][d], accW1[p][ALG::grade(d)]); });
        });
#else
        static_for<0, NP>([&](auto p) { static_for<0, D>([&](auto d) { accW1[p][ALG::grade(d)][0] += gy[d] * x[p][d]; }); });
#endif
        stamp(15);
        // next tile's rows, then this tile's stores / atomics
        if constexpr (!single) {
            T = Tn;
            issue(T);
            Tn.load(in, tile + 2 * tstride, r);
        }
        // d/d(input): a row behind the last one lies behind its array (no store); the attribute gradient is stored by the
        // lanes that own one of its channels
        const unsigned o_row = in.row_off(Tc.row);
        if constexpr (K > 0) {
            float gx[D];
#pragma unroll
            for (int d = 0; d < D; ++d) gx[d] = 0.f;
            cl_mix<C, C, TB::W1T(0)>(gx, gy, ldsw);
            if constexpr (single) {
                carry_a = f4{gx[0], gx[1], gx[2], gx[3]}; carry_b = f4{gx[4], gx[5], gx[6], gx[7]};
            } else {
                b_hand.st8(o_row, gx);
            }
        } else if constexpr (MODE == MODE_EDGE) {
            if (io.gx[0]) {
                float gx[D];
#pragma unroll
                for (int d = 0; d < D; ++d) gx[d] = 0.f;
                cl_mix<C, C, TB::W1T(0)>(gx, gy, ldsw);
                if (io.row_store) {
                    b_gx0.st8(o_row, gx);
                } else {
                    CL_LDS_ORDER();
                    cl_st8(sc + r * SS + c * D, gx);
                    CL_LDS_ORDER();
                    cl_scatter<C, ROW, true>(sc, Tc.valid ? Tc.i_dst : -1, Tc.valid ? Tc.i_src : -1, io.gx[0], lane);
                }
            }
            if constexpr (NA > 0) {
                if (io.gx[1]) {
                    float gx[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) gx[d] = 0.f;
                    cl_mix<C, C, TB::W1T(1)>(gx, gy, ldsw);
                    // by permutation into a table the launch may cover a slice of (ClIn::attr): 64-bit address, one branch
                    if (Tc.valid && in.in_attr) cl_st8(io.gx[1] + ((size_t)(unsigned)Tc.i_perm * (NA * D) + c * D), gx);
                }
            }
        } else {
            if (io.gx[0]) {
                float gx[D];
#pragma unroll
                for (int d = 0; d < D; ++d) gx[d] = 0.f;
                cl_mix<C, C, TB::W1T(0)>(gx, gy, ldsw);
                if (io.resid_bwd) {
                    if constexpr (!single) { res0 = in.gy.ld4(o_row); res1 = in.gy.ld4(o_row + 16); }
                    const float res[D] = {res0.x, res0.y, res0.z, res0.w, res1.x, res1.y, res1.z, res1.w};
#pragma unroll
                    for (int d = 0; d < D; ++d) gx[d] += res[d];
                }
                b_gx0.st8(o_row, gx);
            }
            if (io.gx[1]) {
                float gx[D];
#pragma unroll
                for (int d = 0; d < D; ++d) gx[d] = 0.f;
                cl_mix<C, C, TB::W1T(1)>(gx, gy, ldsw);
#pragma unroll
                for (int d = 0; d < D; ++d) gx[d] *= Tc.scale();
                b_gx1.st8(o_row, gx);
            }
            if constexpr (NA > 0) {
                if (io.gx[2]) {
                    float gx[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) gx[d] = 0.f;
                    cl_mix<C, C, TB::W1T(2)>(gx, gy, ldsw);
                    b_gx2.st8(in.in_attr ? Tc.row * IN::AB + in.lo : kClNoStore, gx);
                }
            }
        }
        stamp(16);
        if constexpr (single) break;
    }
    // one tile per wave: block K - 1 works on the same tile; its rows travel during this block's end phase
    if constexpr (K > 0 && single) next.template request<K - 1>(io, in, T0);

    // ---- end of the block: the weight-gradient tiles of this wave -> image of the slice in its scratch; behind ONE barrier
    // the workgroup adds its four images in wave order and writes the matrices of its slice (coalesced 16-byte stores),
    // and owner threads add the lane-private running sums of the whole workgroup into the slice's per-channel part.
    {
        float* img = sc;
        const int j = lane & 15, q = lane >> 4;
        // MFMA tiles. C = 8: tile element (i = 4q + v, j) = (o = i >> 1, r0 = i & 1) x (c = j >> 1, r0' = j & 1); the
        // wanted sum is on r0 = r0': even lanes take v = 0, 2 of their own and v = 1, 3 of their odd neighbour. The pair
        // adds of ALL matrices are issued before the first store: one exec switch for all image stores of the wave.
        constexpr int NM = NP + 2;
        f4 lo[NM], hi[NM];
        auto pair_tile = [&](const f4 (&acc)[G], int m) {
            if constexpr (C == 8) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    lo[m][g] = acc[g][0] + dpp_mov<0xB1>(acc[g][1]);   // quad_perm [1,0,3,2]: the odd neighbour's value
                    hi[m][g] = acc[g][2] + dpp_mov<0xB1>(acc[g][3]);
                }
            }
        };
        auto put_tile = [&](const f4 (&acc)[G], int m, int base, int I, int coff, int width) {
            if constexpr (C == 8) {
                const int cc = j >> 1;
                if ((j & 1) == 0 && cc < width) {
                    float* p0 = img + base + ((2 * q) * I + coff + cc) * G;
                    st4(p0, lo[m]);
                    st4(p0 + I * G, hi[m]);
                }
            } else {
                if (j < width) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        float* p0 = img + base + ((4 * q + v) * I + coff + j) * G;
                        st4(p0, f4{acc[0][v], acc[1][v], acc[2][v], acc[3][v]});
                    }
                }
            }
        };
        static_for<0, NP>([&](auto p) { pair_tile(accW1[p], p); });
        pair_tile(accR, NP);
        pair_tile(accL, NP + 1);
        if constexpr (C == 8) {
#pragma unroll
            for (int m = 0; m < NM; ++m) asm volatile("" : "+v"(lo[m]), "+v"(hi[m]) : : "memory");
        }
        static_for<0, NP>([&](auto p) { put_tile(accW1[p], p, 0, TB::I, TB::coff(p), TB::width(p)); });
        put_tile(accR, NP, PT::pWR, C, 0, C);
        put_tile(accL, NP + 1, PT::pWL, C, 0, C);
        stamp(21);
        // every wave's image and every thread's running sums are in LDS behind this barrier (a wave without a tile and the
        // rows behind the last valid one left exact zeros: the sums are zeroed at the top of the block, gout is 0 there)
        __syncthreads();
        stamp(22);
        // block k's slices start behind those of the blocks 0 .. k - 1 (kClSliceCap slices each)
        float* part = io.rl_partials + (K == 0 ? 0 : (size_t)kClSliceCap * ClPart<ALG, C, ClTab<C, MODE, NA, 0, true>::I>::total) +
                      (size_t)blockIdx.x * PT::total;
        // Per-channel sums. The running sums stay where the tile loop kept them: [group of 4][thread] f4, thread = wave * 64 +
        // lane, lane = (row, channel). Output (channel oc, group og) = the f4 sum over the kClWaves * RPW (32) threads of
        // channel oc. Two neighbouring threads own one output: thread `par` adds the rows of parity par, waves 0 .. 3 and
        // rows par, par + 2, .. in that order (16 independent ds_read_b128: the 16 lanes of 8 channels x 2 parities read 256
        // consecutive bytes), one DPP add joins the pair. The order is fixed: the sums are bit-identical from run to run.
        constexpr int KG = ClSums<RM::n>::kGroups, GS = 4 * 64 * kClWaves, HR = RPW / 2;
        static_assert(2 * C * KG <= 64 * kClWaves, "one pair of owner threads per (channel, group of four sums)");
        const int par = threadIdx.x & 1, own = threadIdx.x >> 1, oc = own % C, og = own / C;
        f4 s = f4{0.f, 0.f, 0.f, 0.f};
        if (own < C * KG) {
            const float* src = work + kClWaves * scratch + og * GS + 4 * (MP::lane_of_row(par) + oc * MP::ROTL);
            f4 v[kClWaves * HR];
#pragma unroll
            for (int w = 0; w < kClWaves; ++w) {
#pragma unroll
                for (int rh = 0; rh < HR; ++rh) v[w * HR + rh] = ld4(src + 4 * (w * 64 + MP::lane_of_row(2 * rh)));
            }
            s = v[0];
#pragma unroll
            for (int i = 1; i < kClWaves * HR; ++i) s += v[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] += dpp_mov<0xB1>(s[i]);   // the other parity's rows (both lanes: the same sum)
        }
        // block 0's rows are taken here: they had the tile images, the barrier and the sums to travel, and no store of this
        // end phase is in front of them
        if constexpr (K == 1 && single) next.arrived0();
        if (own < C * KG) {   // the pair's four values: the even thread stores 0 and 1, the odd one 2 and 3
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = 4 * og + 2 * par + i;
                const float val = par ? s[2 + i] : s[i];
                if (idx < RM::n) part[PT::pS + PT::off(idx) + oc * PT::stride(idx)] = val;
            }
        }
        // the matrices: four images -> slice
        const float* img0 = work;
        static_assert(PT::pS % 4 == 0, "matrix part of the slice");
        for (int e = 4 * threadIdx.x; e < PT::pS; e += 4 * 64 * kClWaves) {
            f4 v = ld4(img0 + e);
#pragma unroll
            for (int w = 1; w < kClWaves; ++w) v += ld4(img0 + w * scratch + e);
            st4(part + e, v);
        }
    }
    stamp(17);
    return ClCarry{carry_a, carry_b};
}
template <class ALG, int C, int MODE, int NBLK, int NA>
constexpr size_t cl_bwd_lds_bytes() {
    using TB0 = ClTab<C, MODE, NA, 0, true>;
    using TB1 = ClTab<C, MODE, NA, 1, true>;
    constexpr int tile = ClMap<C>::RPW * (C * ALG::D + 4);
    int img = ClPart<ALG, C, TB0::I>::total;
    if (NBLK > 1 && ClPart<ALG, C, C>::total > img) img = ClPart<ALG, C, C>::total;
    return sizeof(float) * (TB0::total + (NBLK > 1 ? TB1::total : 0) + kClWaves * (tile > img ? tile : img) +
                            ClSums<ClRed<ALG>::n>::floats_per_wg);
}
// the blocks of a backward launch, last block first
template <class ALG, int C, int MODE, int NBLK, int NA, bool SAVES, bool SINGLE>
CSMPN_DEV void cl_bwd_blocks(const RowIO& io, const ClBwdIn<ALG, C, MODE, NA>& in, float* smem, const ClTile<C, MODE>& T0, ClBwdReq<ALG, C, MODE, NBLK, NA, SAVES>& req,
                             ClStamp& stamp) {
    using TB0 = ClTab<C, MODE, NA, 0, true>;
    using TB1 = ClTab<C, MODE, NA, 1, true>;
    constexpr int tabs = TB0::total + (NBLK > 1 ? TB1::total : 0);
    ClCarry carry{f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
    if constexpr (NBLK > 1) {
        // req: block 1's row registers, filled by the kernel in front of the staging. req0: block 0's; block 1 fills them
        // ahead of its end phase when SINGLE, else block 0 requests into them itself. Block 0 has no block behind it: the
        // struct passed as its `next` is never written.
        ClBwdReq<ALG, C, MODE, NBLK, NA, SAVES> req0;
        carry = cl_bwd_block<ALG, C, MODE, NBLK, NA, 1, SAVES, SINGLE>(io, in, smem + TB0::total, smem + tabs, T0, req, req0, carry, stamp);
        // this wave's hand-over rows have left for L2. With one tile per wave there are none: the only stores in flight
        // are the workgroup's block-1 slice, which nobody reads in this launch
        if constexpr (!SINGLE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(18);
        __syncthreads();                                   // ... and every wave is done with the images
        stamp(19);
        cl_bwd_block<ALG, C, MODE, NBLK, NA, 0, SAVES, SINGLE>(io, in, smem, smem + tabs, T0, req0, req, carry, stamp);
    } else {
        // one block: it is the last one, `req` holds its requests; `next` (the same struct) is never written
        cl_bwd_block<ALG, C, MODE, NBLK, NA, 0, SAVES, SINGLE>(io, in, smem, smem + tabs, T0, req, req, carry, stamp);
    }
}
// The backward kernel: the blocks one after the other (last block first) in ONE launch. A wave keeps its tiles from
// block to block, so the hand-over rows d/d(block input) it reads in block k - 1 are the ones it wrote itself in block k
// (through L2: the region is not read earlier in the launch, its lines cannot sit stale in this CU's L1; the stores are
// drained before the workgroup's barrier) - no grid-wide synchronisation, one prologue less, and the node program
// (one tile per wave) is a single launch.
template <class ALG, int C, int MODE, int NBLK, int NA, bool SAVES = false>
__global__ void __launch_bounds__(64 * kClWaves, 2) cemlp_cl_bwd_kernel(const DevCemlp C_arg, const RowIO io_arg) {
    CSMPN_KERNEL_ARGS(Cd);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    ClStamp stamp(0);
    using TB0 = ClTab<C, MODE, NA, 0, true>;
    using TB1 = ClTab<C, MODE, NA, 1, true>;
    constexpr int tabs = TB0::total + (NBLK > 1 ? TB1::total : 0);
    // the wave's first tile: its indices once for all blocks, the last block's rows on their way while the tables are staged
    const int lane = threadIdx.x & 63;
    const ClBwdIn<ALG, C, MODE, NA> in(io, ClMap<C>::chan(lane), ClMap<C>::row(lane));
    ClTile<C, MODE> T0;
    ClBwdReq<ALG, C, MODE, NBLK, NA, SAVES> req;
    T0.load(in, blockIdx.x * kClWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), ClMap<C>::row(lane));
    req.template request<NBLK - 1>(io, in, T0);
    // the tables of every block are staged up front (one prologue per launch)
    {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int dir = cl_probe_dir<C>(ClMap<C>::chan(lane));
        ClStage<ALG, C, TB0, true> st0;
        ClStage<ALG, C, TB1, true> st1;
        st0.load(Cd.b[0], wave, lane, dir);
        if constexpr (NBLK > 1) st1.load(Cd.b[1], wave, lane, dir);
        st0.store(smem, wave, lane);
        if constexpr (NBLK > 1) st1.store(smem + TB0::total, wave, lane);
    }
    __syncthreads();
    stamp(0);
    const unsigned ntiles = (in.rows + ClMap<C>::RPW - 1) / ClMap<C>::RPW;
    // one tile per wave (uniform over the grid): the hand-over stays in registers, every block's rows are requested ahead
    if (ntiles <= gridDim.x * kClWaves) cl_bwd_blocks<ALG, C, MODE, NBLK, NA, SAVES, true>(io, in, smem, T0, req, stamp);
    else cl_bwd_blocks<ALG, C, MODE, NBLK, NA, SAVES, false>(io, in, smem, T0, req, stamp);
    stamp.flush(io.stamps, threadIdx.x & 63);
}

// last kernel of a backward: grads += sum over the workgroups' slices of EVERY block, fixed order (deterministic).
// The slices of block 1 start slice_cap * (slice length of block 0) floats behind those of block 0. A workgroup takes 16
// consecutive elements (64-byte pieces of every slice); thread (j = tid & 15, w = tid >> 4) adds the slices w, w + 16,
// ... sixteen loads in flight at a time; the 16 partial sums of an element meet in LDS and are added in order.
// `group`: the workgroup's index within this backward's element range (the launch may hold the ranges of two backwards).
template <class ALG, int C, int I0, int NBLK>
CSMPN_DEV void cl_reduce_group(const DevCemlp& Cd, const float* part, int nslices, int slice_cap, int group, float (*red)[17]) {
    constexpr int G = ALG::G;
    using P0 = ClPart<ALG, C, I0>;
    using P1 = ClPart<ALG, C, C>;
    constexpr int total = P0::total + (NBLK > 1 ? P1::total : 0);
    const int j = threadIdx.x & 15, w = threadIdx.x >> 4;
    int e = group * 16 + j;
    const bool live = e < total;
    if (!live) e = 0;
    const int k = (NBLK > 1 && e >= P0::total) ? 1 : 0;
    const int len = k == 0 ? P0::total : P1::total;
    const float* p = part + (k == 0 ? 0 : (size_t)slice_cap * P0::total);
    if (k == 1) e -= P0::total;
    float s = 0.f;
    for (int s0 = w; s0 < nslices; s0 += 256) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int sl = s0 + 16 * i;
            v[i] = sl < nslices ? p[(size_t)sl * len + e] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
    }
    red[w][j] = s;
    __syncthreads();
    if (w != 0 || !live) return;
#pragma unroll
    for (int i = 1; i < 16; ++i) s += red[i][j];
    const DevBlock& B = Cd.b[k];
    const int I = k == 0 ? I0 : C;
    int f = e;
    float* dst = nullptr;
    const int nW1 = C * I * G, nWC = C * C * G;
    if (f < nW1) dst = B.gW1 + f;
    else if ((f -= nW1) < nWC) dst = B.gWR + f;
    else if ((f -= nWC) < nWC) dst = B.gWL + f;
    else {
        f -= nWC;
        if (f < P0::qsa) dst = B.has_b1 ? B.gb1 + f : nullptr;
        else if (f < P0::qsb) dst = B.gsa + (f - P0::qsa);
        else if (f < P0::qw) dst = B.gsb + (f - P0::qsb);
        else if (f < P0::qan) dst = B.gw + (f - P0::qw);
        else if (f < P0::qbL) dst = B.gan + (f - P0::qan);
        else if (f < P0::qla) dst = B.gbL + (f - P0::qbL);
        else dst = B.gla + (f - P0::qla);
    }
    if (dst) *dst += s;
}
template <class ALG, int C, int I0, int NBLK>
constexpr int cl_reduce_groups() { return (ClPart<ALG, C, I0>::total + (NBLK > 1 ? ClPart<ALG, C, C>::total : 0) + 15) / 16; }
template <class ALG, int C, int I0, int NBLK>
__global__ void __launch_bounds__(256) cl_reduce_kernel(const DevCemlp Cd, const float* part, int nslices, int slice_cap) {
    __shared__ float red[16][17];
    cl_reduce_group<ALG, C, I0, NBLK>(Cd, part, nslices, slice_cap, blockIdx.x, red);
}
// The slice sums of TWO backwards in one launch (csmpn_egcl_backward: the node program's sum, deferred, beside the edge
// program's): the first cl_reduce_groups<A> workgroups take backward A's elements, the rest backward B's. Every element is
// summed exactly as cl_reduce_kernel sums it; the two ranges touch disjoint slices and gradient tensors.
template <class ALG, int C, int I0A, int NBLKA, int I0B, int NBLKB>
__global__ void __launch_bounds__(256) cl_reduce2_kernel(const DevCemlp CdA, const float* partA, int nslicesA, const DevCemlp CdB,
                                                         const float* partB, int nslicesB, int slice_cap) {
    __shared__ float red[16][17];
    constexpr int groupsA = cl_reduce_groups<ALG, C, I0A, NBLKA>();
    if ((int)blockIdx.x < groupsA) cl_reduce_group<ALG, C, I0A, NBLKA>(CdA, partA, nslicesA, slice_cap, blockIdx.x, red);
    else cl_reduce_group<ALG, C, I0B, NBLKB>(CdB, partB, nslicesB, slice_cap, (int)blockIdx.x - groupsA, red);
}

}  // namespace csmpn
