// The few constants of the operator layouts that the device side (device.h, the kernels) and the pure-host layout unit
// (operator_layout.h) share.  No HIP.
#pragma once

#include "qprop_internal.h"

namespace qp {

constexpr int kRB = 64;           // rows per row block = one wavefront

// mode of a block's column section (low two bits of its meta word, the rest is the byte offset)
enum { kColInt32 = 0, kColInt16 = 1, kColStencil = 2, kColBlockMap = 3 };

// the formats whose value array is in CSR order (rowptr / cols / vals[p])
inline bool csr_layout(int format) { return format == QP_FMT_CSR || format == QP_FMT_DENSE; }

// ---- plain data the planners (operator_plans.h) compute and the kernels read ------------------------------------------
// column-blocked mirror (device.h: ColBlockPlan, which adds the device arrays)
struct ColBlockShape {
  int valid = 0;
  int log2w = 17;               // columns per block = 1 << log2w  (2 MB of x)
  int P = 0;                    // column blocks
  int rpt = 2;                  // 64-row groups per tile
  int max_seg = 0;              // entries of the longest segment (the per-wavefront LDS buffer holds one segment)
  int64_t ntiles = 0, nnz = 0;
};
constexpr int kCbMaxTilesPerWave = 8;
constexpr int kCbMaxSeg = 1024;
// fixed choices that were knobs while they were being measured (docs/history/): the resident wavefronts per CU the column-blocked
// mirror is sized for (24 and 32 measured slower)
constexpr int kCbWavesPerCu = 16;
constexpr int kCbMinLog2N = 20;     // column-blocked mirror: smallest number of columns (log2) it is built for (measured: 2^18 columns 0.9 x, 2^19 1.04 x, 2^20 1.37 x, 2^21 1.62 x, 2^22 1.52 x)

// LDS tiles of the batched path (device.h: SpmmTiles)
constexpr int kSpmmTileMaxEntries = 24;   // entries per row (2 K + 2 NN + 1 = 17 at most; a multiple of 8: the sums go in groups of eight)
constexpr int kSpmmTileSlots = 80;        // staged rows at most (K = NN = 4): 80 KiB of LDS, two workgroups per compute unit
struct SpmmTileShape {
  int nd = 0, K = 0, NN = 0;
  int dfar[kSpmmTileMaxEntries] = {0};    // entry k: strip steps m (d = m g) when dnear[k] == 0 ...
  int dnear[kSpmmTileMaxEntries] = {0};   // ... else the near distance d
};
// the kernel's table (device, int32): [0, 80) row of staged slot s relative to the tile's first row r0; then for wavefront w = 4 i + j
// and entry k the LDS byte offset of that entry's operand (24 per wavefront); then the wavefront's own row relative to r0 (16) and
// the LDS byte offset of its own element (16)
constexpr int kSpmmTileTab = kSpmmTileSlots + 16 * kSpmmTileMaxEntries + 32;
constexpr int kSpmmTileRowBytes = 64 * 16;   // a staged row in LDS: 64 states of 16 bytes

}  // namespace qp
