// Host-visible launcher declarations of every kernel family, one set per compiled algebra, and the launch caps the host
// sizes the families' workspace regions by.
#pragma once
#include <hip/hip_runtime.h>

#include "cemlp_device.hpp"

namespace csmpn {
constexpr int kMaxLdsBytes = 160 * 1024;

// general row-tile kernels (cemlp_kernel.hpp, cemlp_ps.hpp), wide row-tile kernel (cemlp_wide.hpp), geometric product
#define CSMPN_DECLARE_ALG(tag)                                                                                  \
    bool has_h2_##tag();                                                                                        \
    bool has_ps_##tag();                                                                                        \
    hipError_t launch_cemlp_ps_##tag(int mode, bool bwd, unsigned grid, unsigned block, size_t lds,            \
                                     hipStream_t st, const DevCemlp& C, const RowIO& io);                      \
    hipError_t launch_cemlp_##tag(int mode, int var, int h, bool bwd, unsigned grid, unsigned block, size_t lds,   \
                                  hipStream_t st, const DevCemlp& C, const RowIO& io);                          \
    hipError_t launch_cemlp_wide_##tag(int mode, bool bwd, unsigned grid, unsigned block, size_t lds, hipStream_t st, \
                                       const DevCemlp& C, const RowIO& io);                                    \
    hipError_t launch_gp_##tag(bool bwd, const float* a, const float* b, const float* gout, float* out,        \
                               float* ga, float* gb, long rows, hipStream_t st);

CSMPN_DECLARE_ALG(n2)      // Cl(2,0)
CSMPN_DECLARE_ALG(n3)      // Cl(3,0)
CSMPN_DECLARE_ALG(n4)      // Cl(4,0)
CSMPN_DECLARE_ALG(n5)      // Cl(5,0)
CSMPN_DECLARE_ALG(n5m)     // Cl(4,1): metric (1,1,1,1,-1)
CSMPN_DECLARE_ALG(n4m)     // Cl(3,1): metric (1,1,1,-1)

// (row, channel)-per-lane kernels (cemlp_cl.hpp)
constexpr int kClMaxFwdGroups = 1024;   // 4-wave workgroups of a forward launch: four per CU (4 waves per SIMD)
constexpr int kClMaxBwdGroups = 512;    // ... of a backward launch: two per CU; one slice of partial sums each (= kClSliceCap of cemlp_cl.hpp)
#define CSMPN_DECLARE_CL(tag)                                                                                  \
    bool has_cemlp_cl_##tag(int mode, int nblk, int channels, int i0);                                          \
    size_t cemlp_cl_partial_floats_##tag(int mode, int nblk, int channels, int i0);                             \
    hipError_t launch_cemlp_cl_##tag(int mode, int nblk, int channels, int i0, bool bwd, unsigned grid,         \
                                     hipStream_t st, const DevCemlp& C, const RowIO& io, bool* handled);
CSMPN_DECLARE_CL(n3)

// channel-MFMA kernels (cemlp_cm.hpp)
constexpr int kCmMaxFwdGroups = 768;   // 4-wave workgroups of a forward launch: three per CU
constexpr int kCmMaxBwdGroups = 256;   // ... of a backward launch (one per CU: 512 registers); one slice of partial sums each
constexpr int kCmSliceCap = 512;       // slices the partial buffer is laid out for (block 1's start behind kCmSliceCap of block 0: = kClSliceCap)
#define CSMPN_DECLARE_CM(tag)                                                                                  \
    bool has_cemlp_cm_##tag(int mode, int nblk, int channels, int i0, bool bwd);                                \
    size_t cemlp_cm_partial_floats_##tag(int mode, int nblk, int channels, int i0);                             \
    hipError_t launch_cemlp_cm_##tag(int mode, int nblk, int channels, int i0, bool bwd, unsigned grid,         \
                                     hipStream_t st, const DevCemlp& C, const RowIO& io, bool* handled);
CSMPN_DECLARE_CM(n3)

// parity-lane kernels (cemlp_pl.hpp): D = 32 algebras with an odd number of generators, every block 8 output channels
constexpr int kPlMaxBwdGroups = 256;   // one 4-wave workgroup per CU in the backward
#define CSMPN_DECLARE_PL(tag)                                                                                 \
    bool has_cemlp_pl_##tag(int mode, int nblk, int channels, int i0);                                         \
    size_t cemlp_pl_slice_floats_##tag(int mode, int nblk, int channels, int i0);                              \
    hipError_t launch_cemlp_pl_##tag(int mode, int nblk, int channels, int i0, bool bwd, unsigned grid,        \
                                     hipStream_t st, const DevCemlp& C, const RowIO& io, bool* handled);
CSMPN_DECLARE_PL(n5)
CSMPN_DECLARE_PL(n5m)

// wide parity-lane kernels (cemlp_plw.hpp)
constexpr int kPlwMaxGroups = 256;   // one workgroup per CU
// floats of the rotation tables for (mode, channels, attribute channels | input channels of MODE_PLAIN, blocks); 0: shape not served
#define CSMPN_DECLARE_PLW(tag)                                                                               \
    size_t cemlp_plw_table_floats_##tag(int mode, int channels, int attr, int nblk);                          \
    hipError_t launch_cemlp_plw_##tag(int mode, int channels, int attr, int nblk, bool bwd, unsigned grid,    \
                                      hipStream_t st, const DevCemlp& C, const RowIO& io, float* tabs, bool* handled);
CSMPN_DECLARE_PLW(n5)
CSMPN_DECLARE_PLW(n5m)

// 16-row-tile MFMA-mixing kernels for D = 32 (cemlp_pg.hpp)
// floats of the weight-fragment tables for (mode, channels, attribute channels); 0: shape not served
#define CSMPN_DECLARE_PG(tag)                                                                                       \
    size_t cemlp_pg_table_floats_##tag(int mode, int channels, int attr);                                            \
    size_t cemlp_pg_slice_floats_##tag(int mode, int channels, int attr);                                            \
    bool has_cemlp_pg_##tag(int mode, int channels, int attr, bool bwd);                                            \
    hipError_t launch_cemlp_pg_##tag(int mode, int channels, int attr, bool bwd, bool pack, unsigned grid, hipStream_t st,      \
                                     const DevCemlp& C, const RowIO& io, float* tabs, bool* handled);
CSMPN_DECLARE_PG(n5)
CSMPN_DECLARE_PG(n5m)

// 16-row-tile MFMA-mixing kernels for Cl(3,0) at 32 channels (cemlp_pq.hpp)
// workgroups a launch may have = gradient slices the workspace region holds (three 4-wave workgroups per CU)
constexpr unsigned kPqGridCap = 768;
// floats of the weight-fragment tables / of one workgroup's gradient slices (all blocks: each block's launch has its own region) for
// (mode, blocks, channels, attribute channels - MODE_PLAIN: input channels of block 0); 0: shape not served
size_t cemlp_pq_table_floats_n3(int mode, int nblk, int channels, int attr);
size_t cemlp_pq_slice_floats_n3(int mode, int nblk, int channels, int attr);
hipError_t launch_cemlp_pq_n3(int mode, int nblk, int channels, int attr, bool bwd, bool pack, unsigned grid, hipStream_t st, const DevCemlp& C,
                              const RowIO& io, float* tabs, bool* handled);
}  // namespace csmpn
