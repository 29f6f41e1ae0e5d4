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

}  // namespace qp
