// Pure-host layout unit: everything an operator's device arrays ARE, computed on plain host data -- union pattern, Hermitian
// check, row-block pointers, the four column encodings with their decoders, Hermitian packing, the position rule, sparse control
// terms, the value dictionary.  No HIP and no handle type: shapes, vectors and knob values in, vectors out (operator_layout.cpp);
// engine_operator.hip uploads the results.  Index work: exact, and compiled as ordinary C++ by the sanitizer harness.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <system_error>
#include <thread>

#include "layout_constants.h"

// Host arrays of the size of a matrix (gigabytes at N = 2^24): resize() leaves the new elements unwritten -- whoever resizes fills them,
// on several threads -- instead of one thread zeroing them first (std::vector<T>: a serial pass over memory before the real one)
namespace qp {
template <class T>
struct NoInitAlloc {
  using value_type = T;
  NoInitAlloc() = default;
  template <class U>
  NoInitAlloc(const NoInitAlloc<U>&) {}
  T* allocate(size_t n) { return static_cast<T*>(::operator new(n * sizeof(T))); }
  void deallocate(T* p, size_t) { ::operator delete(p); }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    if constexpr (sizeof...(A) > 0) ::new ((void*)p) U(std::forward<A>(a)...);      // (no arguments: nothing written)
  }
  template <class U>
  bool operator==(const NoInitAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const NoInitAlloc<U>&) const { return false; }
};
template <class T>
using HostVec = std::vector<T, NoInitAlloc<T>>;
}  // namespace qp
using qp::cplx;
using qp::kRB;

// host threads the library may keep busy at once: at most 8, and never more than the container's CPU quota leaves (cgroup
// cpu.max: a control group that exceeds its quota is frozen for the rest of the scheduler period -- up to 100 ms in which the
// caller's enqueueing thread does not run either)
inline unsigned host_threads() {
  static const unsigned n = [] {
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      long period = 0;
      if (std::fscanf(f, "%31s %ld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) {
        const long quota = std::atol(q) / period;
        if (quota >= 1) hw = std::min<unsigned>(hw, (unsigned)quota);
      }
      std::fclose(f);
    }
    // up to 16 (the passes are memory-bound: more threads than that buy little; eight ranks of a node each take their share);
    // QP_HOST_THREADS overrides
    unsigned cap = 16;
    if (const char* e = std::getenv("QP_HOST_THREADS")) {
      const long v = std::atol(e);
      if (v >= 1) cap = (unsigned)std::min<long>(v, 256);
    }
    return std::max(1u, std::min(cap, hw > 2 ? hw - 1 : hw));
  }();
  return n;
}

// Phase timer of the host-side operator build (QP_BUILD_TRACE=1: one line per phase on stderr; otherwise two clock reads per phase)
struct BuildTrace {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  const bool on = std::getenv("QP_BUILD_TRACE") != nullptr;
  void mark(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[qp build] %-44s %9.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// The threaded-build harness (tests/sanitize_host_index.cpp --large, built with -DQP_PARALLEL_ROWS_TRACE) learns which call
// sites of parallel_rows really started threads: every call then carries its caller's file and line.  Without the macro nothing
// of this exists.
#ifdef QP_PARALLEL_ROWS_TRACE
void qp_parallel_rows_threaded(const char* file, int line, size_t nthreads);   // (the harness defines it)
#define QP_PARALLEL_ROWS_SITE , const char* site_file = __builtin_FILE(), int site_line = __builtin_LINE()
#else
#define QP_PARALLEL_ROWS_SITE
#endif

// rows [0, n) in contiguous chunks on a few host threads (index work whose iterations write disjoint positions).  A chunk that
// throws (std::bad_alloc of a worker's scratch vector) does not end the process: every thread is joined, and the first
// exception is rethrown on the calling thread, where the C ABI's QP_CATCH makes a status of it as it does on the serial path.
template <class F>
inline void parallel_rows(int64_t n, F&& fn, int64_t serial_below = (int64_t)1 << 16 QP_PARALLEL_ROWS_SITE) {
  const unsigned hw = host_threads();
  if (n < serial_below || hw == 1) {
    fn((int64_t)0, n);
    return;
  }
  std::exception_ptr err;
  std::atomic<bool> failed{false};
  auto guarded = [&fn, &err, &failed](int64_t a, int64_t b) {
    try {
      fn(a, b);
    } catch (...) {
      if (!failed.exchange(true)) err = std::current_exception();   // (read after the joins)
    }
  };
  std::vector<std::thread> th;
  th.reserve(hw);
  const int64_t chunk = (n + hw - 1) / hw;
  int64_t done = 0;   // rows [0, done) have been handed to a thread
  try {
    for (unsigned t = 0; t < hw; ++t) {
      const int64_t a = (int64_t)t * chunk, b = std::min(n, a + chunk);
      if (a >= b) break;
      th.emplace_back([&guarded, a, b] { guarded(a, b); });
      done = b;
    }
  } catch (const std::system_error&) {
    // no more threads to be had (resource limits): the started ones are joined below -- a joinable std::thread destroyed
    // means std::terminate -- and this thread takes the rest
  } catch (const std::bad_alloc&) {
    // (nor memory for a thread's start record: the same)
  }
#ifdef QP_PARALLEL_ROWS_TRACE
  if (th.size() >= 2) qp_parallel_rows_threaded(site_file, site_line, th.size());
#endif
  for (auto& x : th) x.join();
  if (done < n) guarded(done, n);
  if (err) std::rethrow_exception(err);
}

// dst[0, n) = src[0, n) on the host threads (gigabyte arrays: one thread's memcpy is a third of the machine's rate)
template <class T>
inline void parallel_copy(T* dst, const T* src, size_t n) {
  if (n == 0) return;      // (memcpy's pointers must not be null, even for no bytes)
  parallel_rows((int64_t)n, [&](int64_t a, int64_t b) { std::memcpy(static_cast<void*>(dst + a), static_cast<const void*>(src + a), (size_t)(b - a) * sizeof(T)); },
                (int64_t)1 << 20);
}

// ---- host-side layout of the two row-block formats --------------------------------
struct HostLayoutData {
  int format = QP_FMT_RBCSR;
  std::vector<int64_t> bptr;   // RBCSR: all entries; HRB: upper section (c >= r)
  std::vector<int64_t> lptr;   // HRB: lower section (c < r)
  std::vector<int32_t> nlow;   // HRB: number of lower entries per row
  std::vector<int64_t> cmeta, lcmeta;  // per block: (byte offset of the column section << 2) | mode (layout_constants.h)
  int64_t stored = 0, lstored = 0;
};
using HostLayout = HostLayoutData;

// Within a 64-row block, entry k of row r sits at  base + 64 k + (r % 64); column
// indices (and the lower section's positions, and the dictionary's codes) are packed four k per lane.
inline int64_t rb_val_pos(const std::vector<int64_t>& bptr, int64_t r, int64_t k) {
  return bptr[r / kRB] + k * kRB + (r % kRB);
}
inline int64_t rb_quad_pos(const std::vector<int64_t>& bptr, int64_t r, int64_t k) {
  return bptr[r / kRB] + (k >> 2) * (4 * kRB) + (r % kRB) * 4 + (k & 3);
}

using UnionRowptr = qp::HostVec<int64_t>;   // the union pattern: canonical CSR of all terms' positions
using UnionCols = qp::HostVec<int32_t>;

// index of (c, r) among row c's upper entries (Hermitian-packed: the transpose of lower entry (r, c), c < r)
inline int64_t upper_index_of(const UnionRowptr& ur, const UnionCols& uc, const std::vector<int32_t>& nlow, int64_t c, int64_t r) {
  const int32_t* b = uc.data() + ur[c];
  const int32_t* e = uc.data() + ur[c + 1];
  return (std::lower_bound(b, e, (int32_t)r) - b) - nlow[c];
}
// THE position rule: where entry k of union row r lives in the value array of layout `L`; -(position) - 1: the complex conjugate
// of the value there (a lower entry of a Hermitian-packed operator: its transpose is what is stored)
inline int64_t value_position(const HostLayout& L, const UnionRowptr& ur, const UnionCols& uc, int64_t r, int64_t k) {
  if (qp::csr_layout(L.format)) return ur[r] + k;
  const int64_t nl = (L.format == QP_FMT_HRB) ? L.nlow[r] : 0;
  if (k >= nl) return rb_val_pos(L.bptr, r, k - nl);
  const int64_t c = uc[ur[r] + k];
  return -rb_val_pos(L.bptr, c, upper_index_of(ur, uc, L.nlow, c, r)) - 1;
}
// position of every union-CSR entry in the value array (the rule above, per entry)
void csr_value_map(const HostLayout& L, int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, std::vector<int64_t>& map);
// position of the first stored value of 64-row unit u (row blocks of the two row-block formats, 64 rows of a CSR layout): the
// values of the rows of units [u0, u1) fill the positions [unit_pos(u0), unit_pos(u1)) and nothing else
inline int64_t unit_pos(const HostLayout& L, int64_t nrows, const UnionRowptr& ur, int64_t u) {
  if (qp::csr_layout(L.format)) return ur[std::min(nrows, u * kRB)];
  return L.bptr[(size_t)std::min<int64_t>(u, (int64_t)L.bptr.size() - 1)];
}

// A term's values in union order: the term's own array (one canonical term: the union pattern IS the term's -- no 4 GB copy at
// N = 2^24) or an array of its own.
struct PlaneView {
  qp::HostVec<cplx> own;
  const cplx* p = nullptr;
  size_t n = 0;
  PlaneView() = default;
  PlaneView(PlaneView&&) = default;
  PlaneView& operator=(PlaneView&&) = default;
  PlaneView(const PlaneView&) = delete;
  PlaneView& operator=(const PlaneView&) = delete;
  const cplx& operator[](size_t i) const { return p[i]; }
  size_t size() const { return n; }
  void borrow(const qp::HostVec<cplx>& v) {
    qp::HostVec<cplx>().swap(own);
    p = v.data();
    n = v.size();
  }
  qp::HostVec<cplx>& make_own(size_t count) {      // zeros, written by the host threads
    own.resize(count);
    cplx* o = own.data();
    parallel_rows((int64_t)count, [o](int64_t a, int64_t b) { std::fill(o + a, o + b, cplx(0.0)); }, (int64_t)1 << 20);
    p = own.data();
    n = count;
    return own;
  }
  void clear() {
    qp::HostVec<cplx>().swap(own);
    p = nullptr;
    n = 0;
  }
};
using Planes = std::vector<PlaneView>;

// ---- union pattern and the terms' values in its order -------------------------------------------------------------
struct TermCsr {   // one term's canonical host CSR (borrowed)
  const qp::HostVec<int64_t>& rowptr;
  const qp::HostVec<int32_t>& col;
  const qp::HostVec<cplx>& vals;
};
// sorted merge per row; true: ONE term with strictly ascending rows, whose pattern the union then is (a copy)
bool union_pattern(const std::vector<TermCsr>& terms, int64_t nrows, UnionRowptr& ur, UnionCols& uc);
// every position of the nrows x ncols matrix (QP_FMT_DENSE: the CSR-ordered value array IS the row-major matrix)
void dense_complete(int64_t nrows, int64_t ncols, UnionRowptr& ur, UnionCols& uc);
// per-term values in union order (duplicates within a row are summed, as Julia's sparse() does)
void scatter_terms(const std::vector<TermCsr>& terms, bool canonical, int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, Planes& planes);
bool csr_is_hermitian(int64_t n, const UnionRowptr& rp, const UnionCols& col, const PlaneView& vals);
bool planes_all_real(const Planes& planes);

// ---- row-block layout: pointers, column sections, transposed positions -----------------------------------------------
// nlow (HRB), bptr, lptr, stored, lstored of `L` (L.format set by the caller)
void block_pointers(int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, HostLayout& L);
// column sections of the upper (or only) / lower entries: the byte stream, and L.cmeta / L.lcmeta.  `stencil`, `block_map`: knobs
void encode_upper_sections(int64_t nrows, int64_t ncols, const UnionRowptr& ur, const UnionCols& uc, HostLayout& L, bool stencil,
                           bool block_map, std::vector<char>& bytes);
void encode_lower_sections(int64_t nrows, int64_t ncols, const UnionRowptr& ur, const UnionCols& uc, HostLayout& L,
                           const qp::HostVec<int32_t>& lpos, bool stencil, bool block_map, std::vector<char>& bytes);
// HRB: per lower entry (quad-packed like its column) the position of the conj-transposed value in the upper section; -1 = padding
void transposed_positions(int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, const HostLayout& L, qp::HostVec<int32_t>& lpos);
// 32-byte record of one slot of a *stencil* lower section
struct LowerStencilSlot {
  int32_t delta, cb0;
  int64_t pb0, pb1, pad;
};
static_assert(sizeof(LowerStencilSlot) == 32, "layout shared with kernel_common.h");
// decoders of the column sections (bytes and meta words as the device holds them)
int64_t decode_col(const std::vector<char>& bytes, const std::vector<int64_t>& meta, int64_t nrows, int64_t r, int64_t k, bool lower = false);
// position in the upper value array of the conj-transposed value of lower entry k of row r, for a block whose lower section
// is in the stencil encoding
int64_t decode_lower_stencil_pos(const std::vector<char>& bytes, const std::vector<int64_t>& meta, int64_t nrows, int64_t r, int64_t k);

// units [u0, u1) of a chunk of at most `cap` positions (at least one unit)
inline int64_t chunk_end(const HostLayout& L, int64_t nrows, const UnionRowptr& ur, int64_t nunits, int64_t u0, int64_t cap) {
  int64_t u1 = u0 + 1;
  while (u1 < nunits && unit_pos(L, nrows, ur, u1 + 1) - unit_pos(L, nrows, ur, u0) <= cap) ++u1;
  return u1;
}
// dst[0, p1 - p0) = positions [p0, p1) of a plane in device order: zeros, then the stored entries of rows [r0, r1) of the plane in
// union order, each at its position (the two serial_below thresholds of the fill and of the scatter)
void plane_device_order(const HostLayout& L, const UnionRowptr& ur, const UnionCols& uc, const PlaneView& pv, int64_t r0, int64_t r1,
                        int64_t p0, int64_t p1, cplx* dst, int64_t fill_serial_below, int64_t scatter_serial_below);

// ---- sparse control terms -------------------------------------------------------------------------------------------
// may term l belong to the sparse suffix at all?  (control terms beyond the first term of an operator with < 2^31 stored values)
inline bool sparse_candidate(int nops, int ncoeffs, int64_t stored, int l) {
  return nops >= 2 && ncoeffs >= 1 && stored < (int64_t)INT32_MAX && l >= nops - ncoeffs && l >= 1;
}
struct SparseControls {
  int sparse_from = -1;              // first term of the suffix, -1: none
  std::vector<int32_t> support;      // positions in the value array, ascending
  std::vector<cplx> support_vals;    // [nops - sparse_from][support.size()]
};
// the trailing control terms (at most `max_terms` of them) whose non-zero stored values cover at most a quarter of the positions
SparseControls find_sparse_controls(const HostLayout& L, int64_t nrows, int64_t stored, const UnionRowptr& ur, const UnionCols& uc,
                                    const Planes& planes, int ncoeffs, int max_terms);

// ---- value dictionary (device.h: CodedVals) ------------------------------------------------------------------------
struct ValueDict {
  int reason = 0;                    // 0 built, 1 format, 2 a block with > 256 tuples, 3 no saving, 4 knob off
  std::vector<uint8_t> codes;        // [stored], quad-packed (rb_quad_pos)
  std::vector<int64_t> tptr;         // [nblocks]: first entry << 9 | entries (<= 256)
  std::vector<std::vector<cplx>> tab;  // per term [ntab]
  int64_t ntab = 0, ntables = 0;
};
void build_value_dict(bool knob_on, int64_t nrows, int64_t nblocks, int64_t stored, bool planes_real, const HostLayout& L,
                      const UnionRowptr& ur, const Planes& planes, ValueDict& out);
// hv[position] = tab[first entry of the block + code] over every stored position of every block
void decode_value_dict(const HostLayout& L, int64_t nblocks, const std::vector<uint8_t>& codes, const std::vector<int64_t>& tptr,
                       const std::vector<cplx>& tab, std::vector<cplx>& hv);
