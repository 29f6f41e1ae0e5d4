// Which instance of the persistent single-workgroup kernels (kernels_small.hip) a small system takes: lanes per row, entries per
// lane and rows per lane group, as a pure function of plain numbers.  No HIP: the two gates (cheby_plan.cpp: cheby_small_gate, behind engine_cheby.hip: cheby_small_fits;
// engine_krylov.hip: small_sweep_fits), qp_small_plan_host and the tests of the non-GPU suite all call the same function.
#pragma once

#include <cstddef>
#include <cstdint>

namespace qp {

constexpr int kSmallThreads = 512;
constexpr int kSmallEpt = 16;          // register slots per lane of the persistent Chebychev kernel
constexpr int kSmallEptArnoldi = 32;   // ... of the persistent Arnoldi kernel (fewer live values per slot)
constexpr int64_t kSmallLdsRows = 2048;
constexpr size_t kSmallLdsBytes = 152 * 1024;

struct SmallPlan {
  int lanes = 1;            // lanes per row (power of two <= 64)
  int ent = 1;              // entries per lane per row
  int rows_per_group = 1;   // rows per lane group;  rows_per_group * ent <= max_slots
  int obs_lanes = 1;        // lanes per row for the observables
};

// lanes per row, entries per lane and rows per lane group such that the whole matrix is
// register-resident; false when the system does not fit (the caller then runs the general loop)
bool small_plan(int64_t n, int64_t maxrow, SmallPlan* p, int max_slots = kSmallEpt);

// arnoldi! in one launch keeps the Krylov basis (m + 1 vectors) and the work vector in LDS, after 16 bytes of reduction scratch per wavefront
inline bool small_arnoldi_fits(int64_t n, int m) {
  return 16 * ((size_t)kSmallThreads / 64 + (size_t)(m + 2) * (size_t)n) <= kSmallLdsBytes;
}

}  // namespace qp
