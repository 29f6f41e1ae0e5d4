// The complex-fp64 matrix-core tile core (gfx950, v_mfma_f64_16x16x4_f64) shared by the matrix-free Liouvillian
// (engine_liouville.hip: zgemm_sum32_kernel, zgemm_sum_kernel) and the dense panel Chebyshev term (kernels_dense.hip:
// dense_zgemm_cheby_kernel).  Build the including translation unit with -mllvm -amdgpu-mfma-vgpr-form (the accumulators stay
// in VGPRs across the k loop: no AGPR <-> VGPR copies per iteration).
//
// Layout.  One workgroup of four wavefronts = one (16 TA) x (16 TB) tile of the result.  Lane l = (li = l & 15, lk = l >> 4)
// feeds A[i = li][k = lk] and B[k = lk][j = li] and receives C[i = lk + 4 r][j = li] in accumulator register r (verified
// against the library GEMM by the Liouvillian tests).  A complex product is four real ones (Re += ar br - ai bi,
// Im += ar bi + ai br), two when A is real.  Each wavefront owns a quarter of the inner dimension (wave_quarter) and keeps the
// whole tile: TA x TB MFMA tiles, real and imaginary part, 8 TA TB accumulator registers; a k-step of 4 is TA + TB fragment
// loads for 4 TA TB MFMAs.  The four partial tiles are summed through LDS in wave order: deterministic.
//
// The measured rule of the k loop.  On MI355X the fp64 MFMA runs at the rate of the fp64 vector unit and shares its issue:
// every vector-ALU instruction between two MFMAs is time the matrix pipe stands still, from the same or from another
// wavefront (tools/probe/mfma_f64_rate.hip: 27.2 ns per v_mfma_f64_16x16x4_f64 and SIMD with none, 31.8 with two, 38.0 with
// six).  So the loop carries next to no vector-ALU work:
//   * the operands go from L2 into registers in the MFMA lane layout and from there into the MFMAs as they are; the only
//     vector-ALU instructions per k-step are the sign flips of the TA imaginary A fragments;
//   * addresses are a scalar base per operand, advanced by the scalar unit, plus a per-lane offset that never changes
//     (ld_off: buffer loads), and the caller's `load` advances its bases without branches, so that a k-step stays one basic
//     block and its refills and scalar work are spread between the MFMAs (sched_group_barrier);
//   * software pipeline of D slots: step g runs on slot g mod D while the slot of step g - 1 is refilled for step
//     g - 1 + D; no conditions between the first load and the last refill of the steady state (the compiler's vmcnt values
//     are exact only along an unconditional path).
#pragma once
#include <hip/hip_runtime.h>

namespace qp {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

// 16 (or 8: a real operand, imaginary part 0) bytes at (wave-uniform base) + (32-bit lane offset): a buffer load, whose
// descriptor the scalar unit builds from the base -- no vector-ALU address arithmetic in the k loop
__device__ __forceinline__ double2 ld_off(const double2* base, unsigned off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double2*>(base), (short)0, -1, 0x00020000);
  const u4v v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
  double2 d;
  __builtin_memcpy(&d, &v, 16);
  return d;
}
__device__ __forceinline__ double2 ld_off(const double* base, unsigned off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), (short)0, -1, 0x00020000);
  const u2v v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
  double d;
  __builtin_memcpy(&d, &v, 8);
  return make_double2(d, 0.0);
}

// wavefront `wave` of four takes k-steps sbeg .. sbeg + nsteps - 1 of `ksteps`
struct KQuarter {
  int sbeg, nsteps;
};
__device__ __forceinline__ KQuarter wave_quarter(int ksteps, int wave) {
  const int per = (ksteps + 3) / 4;
  const int sbeg = wave * per;
  return KQuarter{sbeg, max(min(ksteps, sbeg + per) - sbeg, 0)};
}

// the accumulators of one wavefront: TA x TB MFMA tiles, real and imaginary part
template <int TA, int TB>
struct ZgemmTile {
  v4d cr[TA][TB], ci[TA][TB];

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int c = 0; c < TB; ++c) cr[a][c] = ci[a][c] = v4d{0.0, 0.0, 0.0, 0.0};
  }

  // one k-step: 4 TA TB MFMAs (2 TA TB when A is real: CPLX false), the real-A products first, then the imaginary-A ones;
  // consecutive MFMAs never share an accumulator where TA TB > 1.  Per accumulator the order of the additions is fixed
  // (re: ar br, then -ai bi; im: ar bi, then ai br): it is what fixes the bits of every kernel built on this.
  template <bool CPLX>
  __device__ __forceinline__ void step(const double2 (&fa)[TA], const double2 (&fb)[TB]) {
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int c = 0; c < TB; ++c) {
        cr[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a].x, fb[c].x, cr[a][c], 0, 0, 0);
        ci[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a].x, fb[c].y, ci[a][c], 0, 0, 0);
      }
    if (CPLX) {
      double nai[TA];
#pragma unroll
      for (int a = 0; a < TA; ++a) nai[a] = -fa[a].y;
#pragma unroll
      for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int c = 0; c < TB; ++c) {
          cr[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai[a], fb[c].y, cr[a][c], 0, 0, 0);
          ci[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a].y, fb[c].x, ci[a][c], 0, 0, 0);
        }
    }
  }

  // this wavefront's partial tiles into red[wave][tile = a TB + c][re | im][r][lane]
  __device__ __forceinline__ void store(double (&red)[4][TA * TB][2][4][64], int wave, int lane) const {
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int c = 0; c < TB; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          red[wave][a * TB + c][0][r][lane] = cr[a][c][r];
          red[wave][a * TB + c][1][r][lane] = ci[a][c][r];
        }
  }
};

// The 4 NT (MFMA tile, accumulator register) pairs of the workgroup's tile are dealt to the four wavefronts, NT each: pair
// p = wave NT + i is register r = p & 3 of MFMA tile p >> 2 (for a 32 x 32 tile: wavefront w finishes MFMA tile w), i.e.
// element (row (tile / TB) 16 + lk + 4 r, column (tile % TB) 16 + li) of the workgroup's tile.
struct TilePair {
  int tile, r;
};
template <int NT>
__device__ __forceinline__ TilePair dealt_pair(int wave, int i) {
  const int p = wave * NT + i;
  return TilePair{p >> 2, p & 3};
}
// ... and summed over wavefronts 0, 1, 2, 3 in that order (after the __syncthreads() that follows ZgemmTile::store; all four
// partial tiles of everybody go through LDS, so that no register is indexed by the wave number)
template <int NT>
__device__ __forceinline__ double2 wave_order_sum(const double (&red)[4][NT][2][4][64], TilePair p, int lane) {
  double sr = red[0][p.tile][0][p.r][lane], si = red[0][p.tile][1][p.r][lane];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    sr += red[w][p.tile][0][p.r][lane];
    si += red[w][p.tile][1][p.r][lane];
  }
  return make_double2(sr, si);
}

// The software-pipelined k loop over `total` k-steps: load(slot) issues the NL fragment loads of the caller's next k-step
// into slot `slot` and advances the caller's cursor (no branches); step(slot) issues the NM MFMAs of the k-step in that slot.
// Steady state: the NL refills are placed behind the MFMAs g with g % (NM / NL) == REFILL_AT; each kernel passes the placement
// it was measured with.  NM < NL: NL / NM refills behind every MFMA, and REFILL_AT is ignored.  total < 2 D - 1: a guarded
// form of the same order.
template <int D, int NM, int NL, int REFILL_AT, class Load, class Step>
__device__ __forceinline__ void pipelined_ksteps(int total, Load&& load, Step&& step) {
  int s = 0;
  if (total >= 2 * D - 1) {
#pragma unroll
    for (int d = 0; d < D - 1; ++d) {
      load(d);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (; s + 2 * D - 1 <= total; s += D) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        load((j + D - 1) % D);
        step(j);
#pragma unroll
        for (int g = 0; g < NM; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);   // at most one vector-ALU instruction
          __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);   // scalar work of the cursor
          if (NM >= NL ? (g % (NM / NL) == REFILL_AT) : true)
            __builtin_amdgcn_sched_group_barrier(0x020, NM >= NL ? 1 : NL / NM, 0);   // the step's refills, spread over it
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // here steps s .. s + D - 2 are loaded or in flight, in slots 0 .. D - 2
    for (; s < total; s += D) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        if (s + j < total) {
          if (s + j + D - 1 < total) load((j + D - 1) % D);
          step(j);
        }
      }
    }
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (d < total) load(d);
    for (; s < total; s += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if (s + d < total) {
          step(d);
          if (s + d + D < total) load(d);
        }
      }
    }
  }
}

}  // namespace qp
