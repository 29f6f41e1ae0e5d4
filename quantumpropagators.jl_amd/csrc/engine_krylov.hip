// arnoldi!, newton!, ritzvals / specrange and the building blocks of their row-partitioned
// variants.
#include <functional>
#include <thread>

#include "engine.h"

// spin-wait hint of the host's polling loops (not only x86)
#if defined(__x86_64__) || defined(__i386__)
#define QP_CPU_RELAX() __builtin_ia32_pause()
#elif defined(__aarch64__)
#define QP_CPU_RELAX() asm volatile("yield" ::: "memory")
#else
#define QP_CPU_RELAX() std::this_thread::yield()
#endif

extern "C" {

// ---------------------------------------------------------------------------
// Arnoldi
// ---------------------------------------------------------------------------
int qp_krylov_create(qp_ctx* ctx, int64_t n, int nvec, qp_krylov** out) {
  QP_TRY
  if (!ctx || !out || n < 0 || nvec < 2) return qp::fail(QP_E_BAD_ARG, "qp_krylov_create: bad arguments");
  QP_CHECK(use(ctx));
  auto q = std::make_unique<qp_krylov>();
  q->ctx = ctx;
  q->n = n;
  q->nvec = nvec;
  QP_CHECK(dev_alloc(&q->Q, (size_t)n * nvec));
  QP_CHECK(dev_alloc(&q->hess_dev, (size_t)nvec * nvec));
  QP_CHECK(dev_alloc(&q->norms_dev, (size_t)nvec));
  QP_CHECK(dev_alloc(&q->part, (size_t)2 * kRedBlocks));
  QP_CHECK(dev_alloc(&q->md_part, (size_t)kRedBlocks * 2 * nvec));
  QP_CHECK(dev_alloc(&q->gram, (size_t)nvec * nvec));
  // rows that were never computed read as NaN: a use of a stale Gram row is loud, not subtle
  QP_HIP(hipMemsetAsync(q->gram, 0xFF, sizeof(double2) * (size_t)nvec * nvec, ctx->stream));
  QP_CHECK(dev_alloc(&q->hcoef, (size_t)2 * nvec));
  QP_CHECK(dev_alloc(&q->mgs_coef, (size_t)nvec));
  QP_HIP(hipMalloc((void**)&q->ticket, sizeof(unsigned)));
  QP_HIP(hipMemsetAsync(q->ticket, 0, sizeof(unsigned), ctx->stream));
  // coherent (fine-grained) pinned memory: what a kernel stores there is visible to the host while the sweep is
  // still running, which the flag hand-off of the folded sweep relies on
  const unsigned hflags = hipHostMallocMapped | hipHostMallocCoherent;
  QP_HIP(hipHostMalloc((void**)&q->h_hess, sizeof(double2) * (size_t)nvec * nvec, hflags));
  QP_HIP(hipHostMalloc((void**)&q->h_norms, sizeof(double) * (size_t)nvec, hflags));
  // [0, nvec): column complete (with its norm); [nvec, 2 nvec): the column's MGS coefficients are written (early flag)
  QP_HIP(hipHostMalloc((void**)&q->col_flags, sizeof(unsigned) * (size_t)nvec * 2, hflags));
  std::memset(q->col_flags, 0, sizeof(unsigned) * (size_t)nvec * 2);
  QP_HIP(hipHostGetDevicePointer((void**)&q->hess_map, q->h_hess, 0));
  QP_HIP(hipHostGetDevicePointer((void**)&q->norms_map, q->h_norms, 0));
  QP_HIP(hipHostGetDevicePointer((void**)&q->col_flags_map, q->col_flags, 0));
  *out = q.release();
  return QP_OK;
  QP_CATCH
}

int qp_krylov_destroy(qp_krylov* q) {
  QP_TRY
  if (!q) return QP_OK;
  (void)hipSetDevice(q->ctx->device);
  (void)hipStreamSynchronize(q->ctx->stream);
  dev_release(q->Q);
  dev_release(q->raw[0]);
  dev_release(q->raw[1]);
  dev_release(q->hess_dev);
  dev_release(q->norms_dev);
  dev_release(q->part);
  dev_release(q->md_part);
  dev_release(q->gram);
  dev_release(q->hcoef);
  dev_release(q->mgs_coef);
  dev_release(q->ticket);
  dev_release(q->op_gram);
  dev_release(q->op_hhat);
  dev_release(q->op_part[0]);
  dev_release(q->op_part[1]);
  dev_release(q->op_svals);
  dev_release(q->op_nu_dev);
  host_release(q->h_hess);
  host_release(q->h_norms);
  host_release(q->col_flags);
  host_release(q->h_nu);
  for (hipEvent_t e : q->col_events) (void)hipEventDestroy(e);
  delete q;
  return QP_OK;
  QP_CATCH
}

int qp_krylov_download(const qp_krylov* q, int i, qp_c128* host) {
  QP_TRY
  if (!q || !host || i < 0 || i >= q->nvec) return qp::fail(QP_E_BAD_ARG, "qp_krylov_download: bad arguments");
  QP_CHECK(use(q->ctx));
  QP_HIP(hipMemcpyAsync(host, q->q(i), (size_t)q->n * sizeof(double2), hipMemcpyDeviceToHost, q->ctx->stream));
  QP_HIP(hipStreamSynchronize(q->ctx->stream));
  return QP_OK;
  QP_CATCH
}

}  // extern "C"

namespace {

// One Arnoldi column: w = H x (x = q[j], or the UNNORMALISED q[j] with the previous column's norm + scale
// folded into this mat-vec, see PlainEpi), then modified Gram-Schmidt of w against q[0..j]; leaves |w|^2
// partials in part[(j+1)&1].  hess column `hcol` (device, length >= j+1) receives dt*<q_i|w>.
struct FoldArgs {
  const double2* norm_part;   // |x|^2 partials of the previous column's projection
  double2* hess_slot;         // Hess[j, j-1]
  double* norm_slot;          // norms[j-1]
  double norm_min;
  unsigned* flag;             // col_flags[j-1] (device address) or null
  unsigned flag_value;
  unsigned* early_flag = nullptr;   // this column's early flag (set by the projection kernel once Hess[0..j, j] is written)
  bool* early_armed = nullptr;
};

int arnoldi_column(qp_operator* op, qp_krylov* q, int j, double dt, double2* hcol, const double2* xin = nullptr,
                   double2* w = nullptr, const FoldArgs* fold = nullptr) {
  qp_ctx* ctx = op->ctx;
  if (!xin) xin = q->q(j);
  if (!w) w = q->q(j + 1);
  qp::PlainEpi pe;
  pe.y = w;
  pe.alpha = make_double2(1.0, 0.0);
  pe.beta = make_double2(0.0, 0.0);
  pe.beta_zero = 1;
  if (fold) {
    pe.norm_part = fold->norm_part;
    pe.xloc = xin;
    pe.qn_out = q->q(j);
    pe.hess_slot = fold->hess_slot;
    pe.norm_slot = fold->norm_slot;
    pe.dt = dt;
    pe.norm_min = fold->norm_min;
    pe.flag = fold->flag;
    pe.flag_value = fold->flag_value;
  }
  const bool lowsync = ctx->tun.arnoldi_mode == 1 && q->gram_rows >= j && qp::mgs_lowsync_fits(j);
  bool dots_done = false;
  {
    const qp::ScopedRange mv_range(ctx->tun.roctx != 0 || qp::ranges_enabled_by_env(), "matrix-vector product");   // src/arnoldi.jl:81
    if (lowsync && ctx->tun.arnoldi_fuse_dots)   // knob: the multidot in the mat-vec's epilogue (kernels_arnoldi.hip)
      QP_CHECK(qp::launch_arnoldi_matvec_dots(ctx->stream, op->A, xin, pe, q->Q, q->n, j, q->md_part, &dots_done, &ctx->stats));
    if (!dots_done) QP_CHECK(qp::launch_spmv_plain(ctx->stream, op->A, xin, pe, &ctx->stats));  // src/arnoldi.jl:82
  }
  if (lowsync) {
    // low-synchronisation MGS: same coefficients (to rounding), 3 launches per column;
    // leaves |w|^2 partials in part[(j+1)&1] like the sequential path.  Needs the Gram
    // rows of the earlier basis vectors, which only this path maintains (a basis built by
    // the persistent small-system kernel or by sequential passes continues sequentially).
    q->gram_rows = j + 1;
    return qp::launch_mgs_lowsync(ctx->stream, q->Q, q->n, j, w, q->md_part, q->gram, q->nvec, hcol,
                                  q->hcoef, q->mgs_coef, q->ticket, q->part + (size_t)((j + 1) & 1) * kRedBlocks, dt,
                                  q->n, &ctx->stats, /* reduction + solve in the projection's prologue */ true, fold ? fold->early_flag : nullptr,
                                  fold ? fold->flag_value : 0u, fold ? fold->early_armed : nullptr, dots_done,
                                  /* rows per XCD, basis back to front: L2 reuse of what the dots pass read last */ true);
  }
  q->gram_rows = std::min(q->gram_rows, j);
  for (int i = 0; i <= j + 1; ++i) {                                              // :84-87
    qp::MgsArgs a;
    a.w = w;
    a.q_prev = (i > 0) ? q->q(i - 1) : nullptr;
    a.q_cur = (i <= j) ? q->q(i) : nullptr;
    a.part_in = q->part + (size_t)((i + 1) & 1) * kRedBlocks;
    a.part_out = q->part + (size_t)(i & 1) * kRedBlocks;
    a.hess_prev = (i > 0) ? hcol + (i - 1) : nullptr;
    a.dt = dt;
    a.n = q->n;
    QP_CHECK(qp::launch_mgs_pass(ctx->stream, a, &ctx->stats));
  }
  return QP_OK;
}

// the two scratch vectors between which the unnormalised vectors of a folded or one-pass sweep ping-pong, on first use
int ensure_raw(qp_krylov* q) {
  if (q->raw[0]) return QP_OK;
  QP_CHECK(dev_alloc(&q->raw[0], (size_t)q->n));
  QP_CHECK(dev_alloc(&q->raw[1], (size_t)q->n));
  return QP_OK;
}

// the one-pass sweep's buffers (qp_krylov in engine.h says what they hold), on first use
int ensure_onepass(qp_krylov* q) {
  if (q->op_gram) return QP_OK;
  const int ldd = q->nvec;
  QP_CHECK(dev_alloc(&q->op_gram, (size_t)ldd * ldd));
  QP_CHECK(dev_alloc(&q->op_hhat, (size_t)ldd * ldd));
  QP_CHECK(dev_alloc(&q->op_part[0], (size_t)qp::op_part_slots(ldd) * kRedBlocks));
  QP_CHECK(dev_alloc(&q->op_part[1], (size_t)qp::op_part_slots(ldd) * kRedBlocks));
  QP_CHECK(dev_alloc(&q->op_svals, (size_t)ldd + 1));
  QP_CHECK(dev_alloc(&q->op_nu_dev, (size_t)ldd + 1));
  QP_HIP(hipHostMalloc((void**)&q->h_nu, sizeof(double) * (size_t)(ldd + 1), hipHostMallocMapped));
  QP_HIP(hipHostGetDevicePointer((void**)&q->nu_map, q->h_nu, 0));
  return QP_OK;
}

// Spin until the device has stored `seq` into *flag (coherent pinned memory): the ONE place where the host polls what a running
// kernel writes.  Never for good.  A flag that must come (`seen` null) is given timeout_s by the clock (looked at every 2^20
// polls); then the host falls back to the stream, looks once more, and fails if "`what` j" still has not announced itself.
// A flag that only lets the host start early (`seen` given) is given max_spins polls; running out of them is no error:
// *seen says whether the flag came, and the stream is left alone.
int wait_flag(qp_ctx* ctx, const unsigned* flag, unsigned seq, double timeout_s, const char* what, int j, bool* seen = nullptr,
              unsigned max_spins = 0) {
  const auto t_begin = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) {
      if (seen) *seen = true;
      return QP_OK;
    }
    if (seen ? spins >= max_spins
             : (spins & 0xfffffu) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > timeout_s)
      break;
    QP_CPU_RELAX();
  }
  if (!seen) QP_HIP(hipStreamSynchronize(ctx->stream));
  const bool there = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq;
  if (seen) *seen = there;
  return there || seen ? QP_OK : qp::fail(QP_E_INTERNAL, "%s %d never announced itself to the host", what, j);
}

}  // namespace

// arnoldi! with an optional normalisation of the start vector: beta_out != NULL means `psi` is
// not normalised; q_0 = psi / |psi| and *beta_out = |psi| (newton! :268-272 folded in, so that
// the persistent small-system kernel does it in the same launch).
//
// on_column != NULL: the host takes the columns as they arrive and calls on_column(j) once column j is
// in Hess -- the caller's work on the leading (j+1) x (j+1) block (newton!: its eigenvalues,
// src/newton.jl:297) overlaps the device's work on the later columns.  (Not on the persistent small sweep,
// whose columns arrive together: its caller goes through them afterwards.)
using ColumnHook = std::function<int(int)>;
constexpr double kOnepassNormDrift = 1e-4;   // |nu_i - 1| of a one-pass sweep's stored basis vectors beyond which the sweep is redone
constexpr double kColumnTimeout = 5.0;       // seconds the host polls for a column's flag before it falls back to the stream

namespace {

// What the host needs to know of an enqueued sweep to take its columns (collect_columns)
enum class Announce {
  stream_end,   // nobody waits for single columns: the sweep is complete when the stream is
  event,        // column j records col_events[j]
  flag,         // the kernel after column j stores the sweep's sequence number into col_flags[j]
};
struct SweepShape {
  Announce announce = Announce::stream_end;
  bool extended = false;     // m + 1 basis vectors, m + 1 rows of Hess: the last column has a norm and a kernel after it
  bool early_last = false;   // the last column also raises its early flag, once its coefficients (not yet its norm) are written
};

// The columns of an enqueued sweep, as they arrive in the pinned buffers: wait for column j, copy its rows into Hess, run the hook
// (for the last column already on its early flag, where armed: that hook is the one the device waits for, and its Hessenberg
// block does not contain the column's norm), stop at a breakdown (src/arnoldi.jl:91-95); then leave the stream drained unless the
// sweep announced itself to the end.  *m_out = number of columns kept.  A failed hook ends the sweep with the hook's status.
int collect_columns(qp_krylov* q, int m, const SweepShape& sw, double norm_min, qp_c128* Hess, int ldh, const ColumnHook* on_column,
                    int* m_out) {
  qp_ctx* ctx = q->ctx;
  const int ldd = q->nvec, dim = sw.extended ? m + 1 : m;
  const cplx* hh = reinterpret_cast<const cplx*>(q->h_hess);
  const double* hn = q->h_norms;
  auto copy_column = [&](int j, int rows) {
    for (int i = 0; i < rows; ++i) {
      const cplx v = hh[(size_t)j * ldd + i];
      Hess[(size_t)j * ldh + i] = qp_c128{v.real(), v.imag()};
    }
  };
  if (sw.announce == Announce::stream_end) QP_HIP(hipStreamSynchronize(ctx->stream));
  int m_eff = m, hook_rc = QP_OK;
  for (int j = 0; j < m; ++j) {
    const bool last = j + 1 == m;
    bool hooked = false;
    if (sw.early_last && last && on_column) {   // coefficients first, hook, then the norm
      bool early = false;
      QP_CHECK(wait_flag(ctx, q->col_flags + q->nvec + j, q->seq, 0.0, nullptr, j, &early, 1u << 24));
      if (early) {
        copy_column(j, j + 1);
        if ((hook_rc = (*on_column)(j)) != QP_OK) break;
        hooked = true;
      }
    }
    if (sw.announce == Announce::event) {
      QP_HIP(hipEventSynchronize(q->col_events[j]));
    } else if (sw.announce == Announce::flag) {
      if (last && !sw.extended)   // no kernel after the last column that could announce it
        QP_HIP(hipStreamSynchronize(ctx->stream));
      else
        QP_CHECK(wait_flag(ctx, q->col_flags + j, q->seq, kColumnTimeout, "Arnoldi column", j));
    }
    if (last) q->t_last_column = std::chrono::steady_clock::now();
    copy_column(j, std::min(j + 2, dim));
    if (on_column && !hooked && (hook_rc = (*on_column)(j)) != QP_OK) break;
    if ((!last || sw.extended) && hn[j] < norm_min) {   // dimensionality exhausted  :91-95
      m_eff = j + 1;
      break;
    }
  }
  // the columns after a breakdown or a failed hook are discarded: wait for them.  (A complete extended sweep of flags needs no wait:
  // its last column announced itself, and what the device still does -- normalising the last vector -- is consumed in stream order.)
  const bool announced_to_the_end = sw.announce == Announce::flag && sw.extended && m_eff == m && hook_rc == QP_OK;
  if (sw.announce != Announce::stream_end && !announced_to_the_end) QP_HIP(hipStreamSynchronize(ctx->stream));
  if (hook_rc != QP_OK) return hook_rc;
  *m_out = m_eff;
  return QP_OK;
}

// ---- the three ways to enqueue a sweep ----

// all m columns in one persistent single-workgroup launch (kernels_small.hip: arnoldi_small_kernel), then one download of the
// Hessenberg matrix and the norms into pinned memory; |psi| (normalize_start) arrives in norms slot ldd - 1, which is never a column's
int enqueue_small_sweep(qp_operator* op, qp_krylov* q, const qp::SmallPlan& plan, int m, const qp_state* psi, double dt, int extended,
                        double norm_min, bool normalize_start) {
  qp_ctx* ctx = op->ctx;
  const int ldd = q->nvec;
  QP_CHECK(operator_csr_mirror(op, false));
  qp::SmallArnoldiArgs a;
  a.n = q->n;
  a.lanes = plan.lanes;
  a.ent = plan.ent;
  a.rows_per_group = plan.rows_per_group;
  a.rowptr = op->m_rowptr;
  a.cols = op->m_cols;
  a.map = op->m_map;
  a.vals = op->A.vals;
  a.start = psi->d;
  a.Q = q->Q;
  a.hess = q->hess_dev;
  a.norms = q->norms_dev;
  a.ldd = ldd;
  a.m = m;
  a.extended = extended;
  a.dt = dt;
  a.norm_min = norm_min;
  a.normalize_start = normalize_start ? 1 : 0;     // the kernel also zero-fills hess / norms
  QP_CHECK(qp::launch_arnoldi_small(ctx->stream, a, &ctx->stats));
  q->gram_rows = 0;
  QP_HIP(hipMemcpyAsync(q->h_hess, q->hess_dev, (size_t)ldd * ldd * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
  QP_HIP(hipMemcpyAsync(q->h_norms, q->norms_dev, (size_t)ldd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  return QP_OK;
}

// Hessenberg entries and norms of the multi-launch and the one-pass sweep go straight into the pinned host buffers (nothing of
// an earlier sweep is in flight: every sweep ends with a synchronisation)
void clear_pinned_columns(qp_krylov* q) {
  std::memset(q->h_hess, 0, sizeof(double2) * (size_t)q->nvec * q->nvec);
  std::memset(q->h_norms, 0, sizeof(double) * (size_t)q->nvec);
}
void next_sequence_number(qp_krylov* q) { q->seq = q->seq + 1 == 0 ? 1 : q->seq + 1; }   // (0 is what the flags start with)

// The multi-launch sweep: mat-vec + projection per column.  Folded (stored operators, m > 1): "norm + scale" of column j is done by
// the mat-vec of column j + 1 (it scales its row sums by 1 / |q_j| and stores the normalised q_j as it goes; src/arnoldi.jl:89-96
// applied on the fly), and the unnormalised vectors ping-pong between two scratch vectors; plain: a norm kernel after every column.
// await_columns: the host will take the columns one by one -- a folded sweep then announces them through col_flags (the sweep gets a
// new sequence number), a plain one through events.  *sw says what was enqueued.
int enqueue_multilaunch_sweep(qp_operator* op, qp_krylov* q, int m, const qp_state* psi, double dt, bool extended, double norm_min,
                              double* beta_out, bool await_columns, SweepShape* sw) {
  qp_ctx* ctx = op->ctx;
  const int ldd = q->nvec;
  clear_pinned_columns(q);
  QP_HIP(hipMemsetAsync(q->ticket, 0, sizeof(unsigned), ctx->stream));
  QP_HIP(hipMemcpyAsync(q->q(0), psi->d, (size_t)q->n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));  // :79
  if (beta_out) {
    cplx n2;
    QP_CHECK(dot_sync(ctx, q->q(0), q->q(0), q->n, &n2));
    *beta_out = std::sqrt(n2.real());
    QP_CHECK(qp::launch_scal(ctx->stream, q->q(0), make_double2(1.0 / *beta_out, 0.0), q->n, &ctx->stats));
  }
  const bool fold = op->A.format != QP_FMT_MATFREE && m > 1;
  const bool flags = fold && await_columns;
  sw->announce = !await_columns ? Announce::stream_end : fold ? Announce::flag : Announce::event;
  sw->extended = extended;
  sw->early_last = false;
  if (fold) QP_CHECK(ensure_raw(q));
  if (flags) next_sequence_number(q);
  while (await_columns && (int)q->col_events.size() < m) {
    hipEvent_t e;
    QP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    q->col_events.push_back(e);
  }
  for (int j = 0; j < m; ++j) {
    const bool last = j + 1 == m;
    double2* hcol = q->hess_map + (size_t)j * ldd;
    double2* w = fold ? q->raw[(j + 1) & 1] : q->q(j + 1);   // where the column leaves its (unnormalised) new vector
    if (fold) {
      FoldArgs fa{q->part + (size_t)(j & 1) * kRedBlocks, j > 0 ? q->hess_map + (size_t)(j - 1) * ldd + j : nullptr,
                  j > 0 ? q->norms_map + (j - 1) : nullptr, norm_min, (flags && j > 0) ? q->col_flags_map + (j - 1) : nullptr,
                  q->seq};
      // The hook of the LAST column is the one the device waits for (the others run while it works on later columns):
      // its Hessenberg block does not contain the column's norm, so it may start as soon as the projection kernel has
      // solved for the coefficients -- while that kernel still streams the basis.
      if (flags && last && j > 0) {
        fa.early_flag = q->col_flags_map + q->nvec + j;
        fa.early_armed = &sw->early_last;
      }
      QP_CHECK(arnoldi_column(op, q, j, dt, hcol, j == 0 ? q->q(0) : q->raw[j & 1], w, j > 0 ? &fa : nullptr));
    } else {
      QP_CHECK(arnoldi_column(op, q, j, dt, hcol));
    }
    // norm + guarded scale of the new vector into the basis (:88-97).  A folded sweep leaves that to the next column's mat-vec: only
    // its last vector remains -- normalised here (extended), where the kernel also announces the last column, or handed over as it is
    if (fold ? (last && extended) : (!last || extended)) {
      QP_CHECK(qp::launch_norm_guard_scale(ctx->stream, q->q(j + 1), w, q->part + (size_t)((j + 1) & 1) * kRedBlocks, hcol + (j + 1),
                                           q->norms_map + j, dt, norm_min, q->n, flags ? q->col_flags_map + j : nullptr, q->seq,
                                           &ctx->stats));
    } else if (fold) {
      QP_HIP(hipMemcpyAsync(q->q(j + 1), w, (size_t)q->n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (sw->announce == Announce::event) QP_HIP(hipEventRecord(q->col_events[j], ctx->stream));
  }
  return QP_OK;
}

// The sweep that reads the basis once per column (knob arnoldi_onepass; kernels_onepass.hip says how): m + 1 column kernels, a
// single-workgroup solve after each; column j of the Hessenberg matrix reaches the pinned host buffer with the solve after
// column kernel j + 1 and announces itself through col_flags[j], like the folded sweep's.  The stored basis vectors have norm
// q->h_nu[i] (1 to rounding unless a projection cancelled nearly everything): the caller divides its combination coefficients by it.
int enqueue_onepass_sweep(qp_operator* op, qp_krylov* q, int m, const qp_state* psi, double dt, double* beta_out) {
  qp_ctx* ctx = op->ctx;
  const int ldd = q->nvec;
  QP_CHECK(ensure_onepass(q));
  QP_CHECK(ensure_raw(q));
  clear_pinned_columns(q);
  for (int i = 0; i <= ldd; ++i) q->h_nu[i] = 1.0;
  double s0 = 1.0;
  if (beta_out) {   // newton! :268-272: beta = |Psi|, q_0 = Psi / beta -- the first column kernel scales by 1 / beta
    cplx n2;
    QP_CHECK(dot_sync(ctx, psi->d, psi->d, q->n, &n2));
    *beta_out = std::sqrt(n2.real());
    s0 = 1.0 / *beta_out;
  }
  next_sequence_number(q);
  q->gram_rows = 0;            // (the low-synchronisation sweep's Gram rows do not describe this basis)
  q->nu_valid = true;
  const qp::ScopedRange mv_range(ctx->tun.roctx != 0 || qp::ranges_enabled_by_env(), "matrix-vector product");
  return qp::launch_arnoldi_onepass_sweep(ctx->stream, op->A, psi->d, s0, q->Q, q->n, q->raw, m, ldd, q->op_part, q->op_gram,
                                          q->op_hhat, q->op_svals, q->op_nu_dev, dt, q->hess_map, q->norms_map, q->nu_map,
                                          q->col_flags_map, q->seq, &ctx->stats);
}

// A whole one-pass sweep: always extended, its columns always awaited by flag (hook or not), no early flag.
int onepass_sweep(qp_operator* op, qp_krylov* q, int m, const qp_state* psi, double dt, double norm_min, qp_c128* Hess, int ldh,
                  int* m_out, double* beta_out, const ColumnHook* on_column) {
  QP_CHECK(enqueue_onepass_sweep(op, q, m, psi, dt, beta_out));
  QP_CHECK(collect_columns(q, m, SweepShape{Announce::flag, true, false}, norm_min, Hess, ldh, on_column, m_out));
  if (*m_out < m) {
    // the reference leaves the vector of a breakdown UNNORMALISED (src/arnoldi.jl:91-95 breaks before :96); the stored one was
    // scaled by s: its coefficient is to be divided by nu / h instead of nu
    const double h = q->h_norms[*m_out - 1];
    q->h_nu[*m_out] = h > 0.0 ? q->h_nu[*m_out] / h : 0.0;
  }
  return QP_OK;
}

// The one-pass sweep never applies H to the new basis vector itself: it carries a_{t+1} = s (H a_t - sum gamma_i q_i) forward by
// linearity and takes the scale from |a|^2 - sum |h|^2, which cancels when h_{t+1,t} << |a_t| -- the known error growth of
// pipelined Krylov sweeps.  The stored vectors' measured norms nu_i say when that happened: all conversions are exact in nu,
// but a nu far from 1 means the recurrence lost digits.
bool onepass_drifted(const qp_krylov* q, int m, int m_eff) {
  double drift = 0.0;
  for (int i = 0; i <= m_eff && i <= m; ++i)
    if (!(i == m_eff && m_eff < m)) drift = std::max(drift, std::fabs(q->h_nu[i] - 1.0));    // (the vector of a breakdown is unnormalised by design)
  return drift > kOnepassNormDrift;
}

enum class Sweep { small, onepass, multilaunch };

// small plan fits -> small; else one-pass wanted, allowed and fits -> one-pass; else multi-launch.  Allowed: only an extended
// low-synchronisation sweep for a caller that divides its combination coefficients by the stored vectors' norms (newton!).
// Wanted: by the knob, or by size -- basis + matrix beyond the Infinity Cache.
Sweep choose_sweep(const qp_operator* op, const qp_krylov* q, int m, bool extended, bool scaled_basis_ok, qp::SmallPlan* plan) {
  const qp_ctx* ctx = op->ctx;
  if (small_sweep_fits(op, q->n, m, plan)) return Sweep::small;
  const double sweep_bytes = 16.0 * (double)q->n * (m + 3) + (op->A.vals_r ? 12.0 : 20.0) * (double)op->A.stored;
  const bool wanted = ctx->tun.arnoldi_onepass >= 2 || (ctx->tun.arnoldi_onepass == 1 && sweep_bytes > 224.0 * 1024 * 1024);
  const bool allowed = extended && scaled_basis_ok && ctx->tun.arnoldi_mode == 1;
  if (wanted && allowed && qp::arnoldi_onepass_fits(op->A, m, q->nvec)) return Sweep::onepass;
  return Sweep::multilaunch;
}

}  // namespace

// does the persistent small-system kernel take an Arnoldi sweep of m columns on this operator (n rows), and with which plan?
// (Also behind qp_operator_small_plan.)
bool small_sweep_fits(const qp_operator* op, int64_t n, int m, qp::SmallPlan* plan) {
  const qp_ctx* ctx = op->ctx;
  if (!(ctx->tun.small_nnz > 0 && op->A.nnz <= (int64_t)ctx->tun.small_nnz * (qp::kSmallEptArnoldi / qp::kSmallEpt) &&
        n == op->A.nrows && qp::small_arnoldi_fits(n, m)))
    return false;
  const int64_t maxrow = operator_longest_row(op);
  // the plan of the 16-slot kernels where it exists (same lanes per row, hence the same rounding, as
  // before the 32-slot variants were added), the larger one only for systems that need it
  return qp::small_plan(n, maxrow, plan, qp::kSmallEpt) || qp::small_plan(n, maxrow, plan, qp::kSmallEptArnoldi);
}

static int arnoldi_impl(qp_operator* op, qp_krylov* q, int m, const qp_state* psi, double dt, int extended,
                        double norm_min, qp_c128* Hess, int ldh, int* m_out, double* beta_out,
                        const ColumnHook* on_column = nullptr, bool scaled_basis_ok = false) {
  QP_TRY
  if (!op || !q || !psi || !Hess || !m_out) return qp::fail(QP_E_BAD_ARG, "qp_arnoldi: NULL argument");
  const int dim = extended ? m + 1 : m;
  if (m < 1 || ldh < dim || q->nvec < m + 1) return qp::fail(QP_E_BAD_ARG, "qp_arnoldi: Hess/q too small for m=%d", m);
  if (op->A.nrows != op->A.ncols || psi->n != op->A.nrows || q->n != psi->n) return qp::fail(QP_E_BAD_ARG, "qp_arnoldi: shape mismatch");
  QP_CHECK(use(op->ctx));
  std::memset(Hess, 0, sizeof(qp_c128) * (size_t)ldh * ldh);                                      // :78
  q->nu_valid = false;   // (true only after a one-pass sweep that stands)
  qp::SmallPlan plan;
  Sweep sweep = choose_sweep(op, q, m, extended != 0, scaled_basis_ok, &plan);
  if (sweep == Sweep::onepass) {
    QP_CHECK(onepass_sweep(op, q, m, psi, dt, norm_min, Hess, ldh, m_out, beta_out, on_column));
    ++q->n_onepass;
    if (!onepass_drifted(q, m, *m_out) && op->ctx->tun.arnoldi_onepass != 3) return QP_OK;
    // drifted (or knob value 3): the sweep is done again in the two-pass form (the column hook is idempotent: it recomputes the
    // Ritz values of the leading blocks from the new columns)
    ++q->n_onepass_redone;
    q->nu_valid = false;
    std::memset(Hess, 0, sizeof(qp_c128) * (size_t)ldh * ldh);
    sweep = Sweep::multilaunch;
  }
  SweepShape sw;
  if (sweep == Sweep::small) {
    sw.extended = extended != 0;   // columns arrive together at the end of the stream: nothing to overlap a hook with
    QP_CHECK(enqueue_small_sweep(op, q, plan, m, psi, dt, extended, norm_min, beta_out != nullptr));
    QP_CHECK(collect_columns(q, m, sw, norm_min, Hess, ldh, nullptr, m_out));
    if (beta_out) *beta_out = q->h_norms[q->nvec - 1];
    return QP_OK;
  }
  // columns are awaited one by one only for a hook's sake
  QP_CHECK(enqueue_multilaunch_sweep(op, q, m, psi, dt, extended != 0, norm_min, beta_out, on_column != nullptr, &sw));
  return collect_columns(q, m, sw, norm_min, Hess, ldh, on_column, m_out);
  QP_CATCH
}

extern "C" {

int qp_arnoldi(qp_operator* op, qp_krylov* q, int m, const qp_state* psi, double dt, int extended, double norm_min,
               qp_c128* Hess, int ldh, int* m_out) {
  return arnoldi_impl(op, q, m, psi, dt, extended, norm_min, Hess, ldh, m_out, nullptr);
}

int qp_arnoldi_extend(qp_operator* op, qp_krylov* q, int m, double dt, double norm_min, qp_c128* Hess, int ldh,
                      int* extended_out) {
  QP_TRY
  if (!op || !q || !Hess) return qp::fail(QP_E_BAD_ARG, "qp_arnoldi_extend: NULL argument");
  if (m < 2 || ldh < m || q->nvec < m + 1) return qp::fail(QP_E_BAD_ARG, "qp_arnoldi_extend: Hess/q too small for m=%d", m);
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  if (extended_out) *extended_out = 0;
  cplx n2;
  QP_CHECK(dot_sync(ctx, q->q(m - 1), q->q(m - 1), q->n, &n2));
  const double h = std::sqrt(n2.real());                                   // src/arnoldi.jl:116
  if (h < norm_min) return QP_OK;                                          // :117
  Hess[(size_t)(m - 2) * ldh + (m - 1)] = qp_c128{dt * h, 0.0};            // :118
  const double inv = 1.0 / h;
  QP_CHECK(qp::launch_scal(ctx->stream, q->q(m - 1), make_double2(inv, 0.0), q->n, &ctx->stats));  // :119
  double2* hcol = q->hess_dev;  // scratch column
  QP_CHECK(arnoldi_column(op, q, m - 1, dt, hcol));                        // :120-124
  std::vector<cplx> hc(m);
  QP_HIP(hipMemcpyAsync(hc.data(), hcol, (size_t)m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
  QP_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < m; ++i) Hess[(size_t)(m - 1) * ldh + i] = qp_c128{hc[i].real(), hc[i].imag()};
  if (extended_out) *extended_out = 1;
  return QP_OK;
  QP_CATCH
}

// ---------------------------------------------------------------------------
// building blocks of a row-partitioned Arnoldi / Newton (the caller owns the collectives)
// ---------------------------------------------------------------------------
int qp_krylov_vec(qp_krylov* q, int i, qp_state** out) {
  QP_TRY
  if (!q || !out || i < 0 || i >= q->nvec) return qp::fail(QP_E_BAD_ARG, "qp_krylov_vec: bad arguments");
  return qp_state_wrap(q->ctx, q->q(i), q->n, out);
  QP_CATCH
}

int qp_krylov_multidot(qp_krylov* q, int j, qp_state* reduced) {
  QP_TRY
  if (!q || !reduced || j < 0 || j + 1 >= q->nvec || reduced->n < 2 * (j + 1))
    return qp::fail(QP_E_BAD_ARG, "qp_krylov_multidot: bad arguments");
  QP_CHECK(use(q->ctx));
  return qp::launch_mgs_multidot(q->ctx->stream, q->Q, q->n, j, q->q(j + 1), q->md_part, reduced->d, q->n, &q->ctx->stats);
  QP_CATCH
}

int qp_krylov_project(qp_krylov* q, int j, double dt, const qp_state* reduced, qp_state* hess_col,
                      qp_state* norm_partials) {
  QP_TRY
  if (!q || !reduced || !hess_col || !norm_partials || j < 0 || j + 1 >= q->nvec || reduced->n < 2 * (j + 1) ||
      hess_col->n < j + 1 || norm_partials->n < kRedBlocks)
    return qp::fail(QP_E_BAD_ARG, "qp_krylov_project: bad arguments");
  QP_CHECK(use(q->ctx));
  QP_CHECK(qp::launch_mgs_project(q->ctx->stream, q->Q, q->n, j, q->q(j + 1), reduced->d, q->gram, q->nvec, hess_col->d,
                                  q->mgs_coef, norm_partials->d, dt, q->n, &q->ctx->stats));
  // the solve has stored Gram row j: a basis whose columns 0 .. j all came this way continues in the low-synchronisation form
  if (q->gram_rows >= j) q->gram_rows = j + 1;
  return QP_OK;
  QP_CATCH
}

int qp_krylov_normalize(qp_krylov* q, int j, double dt, double norm_min, const qp_state* norm_partials,
                        qp_state* hess_norm) {
  QP_TRY
  if (!q || !norm_partials || !hess_norm || j < 0 || j + 1 >= q->nvec || norm_partials->n < kRedBlocks || hess_norm->n < 2)
    return qp::fail(QP_E_BAD_ARG, "qp_krylov_normalize: bad arguments");
  QP_CHECK(use(q->ctx));
  return qp::launch_norm_guard_scale(q->ctx->stream, q->q(j + 1), q->q(j + 1), norm_partials->d, hess_norm->d,
                                     reinterpret_cast<double*>(hess_norm->d + 1), dt, norm_min, q->n, nullptr, 0u, &q->ctx->stats);
  QP_CATCH
}

int qp_combine(qp_state* out, int use_out, qp_c128 s0, qp_krylov* q, int first, int m, const qp_c128* coefs,
               qp_state* norm_partials) {
  QP_TRY
  if (!out || !q || !coefs || first < 0 || m < 1 || first + m > q->nvec || out->n != q->n ||
      (norm_partials && norm_partials->n < kRedBlocks))
    return qp::fail(QP_E_BAD_ARG, "qp_combine: bad arguments");
  QP_CHECK(use(q->ctx));
  return qp::launch_combine_vecs(q->ctx->stream, out->d, use_out, d2(s0), q->q(first), q->n, m,
                                 reinterpret_cast<const double2*>(coefs), norm_partials ? norm_partials->d : nullptr,
                                 q->n, &q->ctx->stats);
  QP_CATCH
}

// ---------------------------------------------------------------------------
// Newton
// ---------------------------------------------------------------------------
int qp_newton_create(qp_ctx* ctx, int64_t n, int m_max, qp_newton** out) {
  QP_TRY
  if (!ctx || !out || n < 0) return qp::fail(QP_E_BAD_ARG, "qp_newton_create: bad arguments");
  if (m_max <= 2) return qp::fail(QP_E_M_MAX, "Newton propagation requires m_max > 2");          // src/newton.jl:38-40
  if (m_max >= n) {                                                                              // :41-46
    m_max = (int)n - 1;
    if (m_max <= 2) return qp::fail(QP_E_M_MAX, "Newton propagation requires state dimension > 2");
  }
  QP_CHECK(use(ctx));
  auto w = std::make_unique<qp_newton>();
  w->ctx = ctx;
  w->n = n;
  w->m_max = m_max;
  QP_CHECK(qp_krylov_create(ctx, n, m_max + 1, &w->q));
  QP_CHECK(dev_alloc(&w->v, (size_t)n));
  QP_CHECK(dev_alloc(&w->npart, (size_t)kRedBlocks));
  QP_HIP(hipHostMalloc((void**)&w->h_npart, kRedBlocks * sizeof(double2), hipHostMallocDefault));
  w->a.assign((size_t)10 * m_max + 1, cplx(0));      // :50-51
  w->leja.assign((size_t)10 * m_max + 1, cplx(0));
  *out = w.release();
  return QP_OK;
  QP_CATCH
}

int qp_newton_destroy(qp_newton* w) {
  QP_TRY
  if (!w) return QP_OK;
  (void)hipSetDevice(w->ctx->device);
  (void)hipStreamSynchronize(w->ctx->stream);
  qp_krylov_destroy(w->q);
  dev_release(w->v);
  dev_release(w->npart);
  host_release(w->h_npart);
  delete w;
  return QP_OK;
  QP_CATCH
}

int qp_newton_get_coeffs(const qp_newton* w, qp_c128* a, qp_c128* leja, int cap) {
  if (!w) return qp::fail(QP_E_BAD_ARG, "newton workspace is NULL");
  if (cap < w->n_a) return qp::fail(QP_E_BAD_ARG, "need room for %d coefficients", w->n_a);
  for (int i = 0; i < w->n_a; ++i) {
    if (a) a[i] = qp_c128{w->a[i].real(), w->a[i].imag()};
    if (leja) leja[i] = qp_c128{w->leja[i].real(), w->leja[i].imag()};
  }
  return QP_OK;
}

// m more Leja points from the Ritz values of this restart (src/newton.jl:306; prod_folded: the head of every candidate's product
// chain, where the hook built it while the columns arrived) and the Newton coefficients that go with them (:313-314)
static int newton_extend_points(qp_newton* w, std::vector<cplx>& ritz, int m, const qp::ScaledProd* prod_folded, int func_id,
                                qp_func_cb cb, void* user, bool ranges, int* n_leja, int* n_a, qp_newton_stats* st) {
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  if ((int)w->leja.size() < *n_leja + m) w->leja.resize((size_t)2 * (*n_leja + m), cplx(0));  // :105-110
  auto t0 = std::chrono::steady_clock::now();
  {
    const qp::ScopedRange leja_range(ranges, "get Leja points");
    qp::extend_leja(w->leja.data(), *n_leja, ritz.data(), (int)ritz.size(), m, prod_folded);
  }
  st->ms_leja += ms_since(t0);
  *n_leja += m;
  if ((int)w->a.size() < *n_leja) w->a.resize((size_t)2 * *n_leja, cplx(0));         // :187-192
  t0 = std::chrono::steady_clock::now();
  int rc;
  {
    const qp::ScopedRange coeff_range(ranges, "get Newton coeffs");
    rc = qp::extend_newton_coeffs(w->a.data(), *n_a, w->leja.data(), func_id, cb, user, *n_leja, w->radius);
  }
  st->ms_coeffs += ms_since(t0);
  if (rc == QP_E_DIVDIFF_UNDERFLOW) return qp::fail(rc, "Divided differences too small");
  if (rc != QP_OK) return qp::fail(rc, "extend_newton_coeffs failed (radius=%g)", w->radius);
  *n_a = *n_leja;
  return QP_OK;
}

// Psi = (accumulate ? Psi : 0) + sum_{i<m} P_i q_i  (:346-352)  and  v = sum_{i<=m} R_i q_i  (q_0 is the start vector of this
// sweep): one pass over the basis; fixed-size coefficient blocks, else one by one.  *norm_psi = |Psi| afterwards.
static int newton_update_states(qp_ctx* ctx, qp_newton* w, qp_state* psi, bool accumulate, int m, double* norm_psi) {
  const double2 *P = reinterpret_cast<const double2*>(w->P.data()), *R = reinterpret_cast<const double2*>(w->R.data());
  if (!qp::launch_combine2_vecs(ctx->stream, psi->d, accumulate ? 1 : 0, m, P, w->v, m + 1, R, w->q->q(0), w->n, w->npart, w->n,
                                &ctx->stats)) {
    QP_CHECK(qp::launch_combine_vecs(ctx->stream, psi->d, accumulate ? 1 : 0, make_double2(1.0, 0.0), w->q->q(0), w->n, m, P, w->npart,
                                     w->n, &ctx->stats));
    QP_CHECK(qp::launch_combine_vecs(ctx->stream, w->v, 0, make_double2(1.0, 0.0), w->q->q(0), w->n, m + 1, R, nullptr, w->n,
                                     &ctx->stats));
  }
  QP_HIP(hipMemcpyAsync(w->h_npart, w->npart, kRedBlocks * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
  QP_HIP(hipStreamSynchronize(ctx->stream));
  *norm_psi = std::sqrt(sum_partials(w->h_npart).real());
  return QP_OK;
}

int qp_newton_step(qp_newton* w, qp_operator* op, qp_state* psi, double dt, int func_id, qp_func_cb cb, void* user,
                   double norm_min, double relerr, int max_restarts, qp_newton_stats* stats) {
  QP_TRY
  if (!w || !op || !psi) return qp::fail(QP_E_BAD_ARG, "qp_newton_step: NULL argument");
  if (op->A.nrows != op->A.ncols || psi->n != op->A.nrows || w->n != psi->n) return qp::fail(QP_E_BAD_ARG, "qp_newton_step: shape mismatch");
  if (func_id == QP_FUNC_CALLBACK && !cb) return qp::fail(QP_E_BAD_ARG, "callback func is NULL");
  if (func_id < 0 || func_id > QP_FUNC_CALLBACK) return qp::fail(QP_E_BAD_ARG, "bad func_id");
  if (dt == 0.0) return qp::fail(QP_E_BAD_ARG, "dt must be non-zero");   // src/newton.jl:263
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  const bool ranges = ctx->tun.roctx != 0 || qp::ranges_enabled_by_env();
  const qp::ScopedRange step_range(ranges, "prop_step!");               // src/newton_propagator.jl:121
  const int m_max = w->m_max;
  int m = m_max;                                                        // :253
  std::fill(w->a.begin(), w->a.end(), cplx(0));                         // :254-255
  std::fill(w->leja.begin(), w->leja.end(), cplx(0));
  const int ldh = m_max + 1;
  std::vector<cplx>&Hess = w->Hess, &ritz = w->ritz;
  Hess.assign((size_t)ldh * ldh, cplx(0));
  int n_a = 0, n_leja = 0, s = 0;
  qp_newton_stats st{};   // filled as the step goes, handed out at its end
  qp_state vstate{ctx, w->v, w->n, false};
  // v = Psi / beta, beta = |Psi| (:268-272) is done by the first Arnoldi sweep itself (q_0)
  double beta = 0.0;
  const int onepass0 = w->q->n_onepass, redone0 = w->q->n_onepass_redone;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  while (true) {                                                                     // :274
    int m_req = m;
    auto t0 = now();
    // Ritz values of every leading block (:297), block j+1 as soon as column j has arrived -- on
    // the multi-launch path while the device is still orthogonalising the later columns
    ritz.assign((size_t)m_req * (m_req + 1) / 2, cplx(0));
    // ... and, from the second restart on, the head of every candidate's Leja product (the factors of
    // the Leja points of the earlier restarts, src/newton.jl:127-136)
    std::vector<qp::ScaledProd>& lprod = w->leja_prod;
    lprod.assign(ritz.size(), qp::ScaledProd{1.0, 0});
    double ms_eig_sweep = 0, ms_fold_sweep = 0;
    int blocks_done = 0;
    const ColumnHook eig_block = [&](int j) -> int {
      auto t1 = now();
      const qp::ScopedRange eig_range(ranges, "diagonalize_hessenberg_matrix");   // src/newton.jl:296
      const size_t off = (size_t)j * (j + 1) / 2;
      const int rc = qp::diagonalize_hessenberg_block(Hess.data(), ldh, j + 1, ritz.data() + off);
      ms_eig_sweep += ms_since(t1);
      if (rc == QP_OK && n_leja > 0) {
        t1 = now();
        for (int i = 0; i <= j; ++i) lprod[off + i] = qp::leja_fold_candidate(w->leja.data(), n_leja, ritz[off + i]);
        ms_fold_sweep += ms_since(t1);
      }
      blocks_done = j + 1;
      return rc == QP_OK ? QP_OK : qp::fail(QP_E_INTERNAL, "Hessenberg QR did not converge");
    };
    {
      const qp::ScopedRange arnoldi_range(ranges, "arnoldi!");                       // src/newton.jl:276
      QP_CHECK(arnoldi_impl(op, w->q, m_req, s == 0 ? psi : &vstate, dt, 1, norm_min,
                            reinterpret_cast<qp_c128*>(Hess.data()), ldh, &m, s == 0 ? &beta : nullptr,
                            ctx->tun.newton_pipeline ? &eig_block : nullptr, true));
    }
    st.ms_arnoldi += ms_since(t0) - ms_eig_sweep - ms_fold_sweep;
    st.ms_eig += ms_eig_sweep;
    st.ms_leja += ms_fold_sweep;
    st.n_matvec += m_req;
    if (m == 1 && s == 0) {                                                          // :289-295
      const cplx lam = beta * Hess[0];
      const cplx f = qp::eval_func(func_id, cb, user, lam);
      QP_CHECK(qp::launch_scal(ctx->stream, psi->d, d2(f), psi->n, &ctx->stats));
      break;
    }
    t0 = now();
    for (int j = blocks_done; j < m; ++j)   // persistent-kernel sweep, or the pipeline switched off
      QP_CHECK(eig_block(j));
    ritz.resize((size_t)m * (m + 1) / 2);
    const bool folded = n_leja > 0;   // (the products do not depend on m: valid also after a breakdown)
    st.ms_eig += ms_since(t0);
    if (s == 0) {                                                                    // :301-303, :67-70
      double rmax = 0;
      for (auto& z : ritz) rmax = std::max(rmax, std::abs(z));
      w->radius = 1.2 * rmax;
    }
    const int n_s = n_leja;                                                          // :307
    QP_CHECK(newton_extend_points(w, ritz, m, folded ? lprod.data() : nullptr, func_id, cb, user, ranges, &n_leja, &n_a, &st));
    // Newton polynomial in the extended Hessenberg matrix (:328-343), then the starting vector of the next restart (:356-367):
    // host algebra (host_numerics.cpp) that leaves the coefficients of Psi in P and those of v in R, in the stored basis
    if (ranges) qp::range_push("evaluate polynomial");                               // src/newton.jl:328 (closed after the update below)
    t0 = now();
    qp::newton_restart_poly(Hess.data(), ldh, m, w->a.data() + n_s, w->leja.data() + n_s, w->radius, beta, w->P, w->R, w->Rn);
    st.ms_poly += ms_since(t0);
    t0 = now();
    beta = qp::newton_restart_next(Hess.data(), ldh, m, w->leja[n_s + m - 1], w->radius, w->q->nu_valid ? w->q->h_nu : nullptr, w->P,
                                   w->R, w->Rn);
    st.ms_exposed += ms_since(w->q->t_last_column);
    QP_CHECK(newton_update_states(ctx, w, psi, s > 0, m, &st.norm_psi));
    if (ranges) qp::range_pop();
    st.ms_update += ms_since(t0);
    st.last_relerr = beta * std::abs(w->a[n_a - 1]) / (1 + st.norm_psi);              // :370
    if (st.last_relerr < relerr) break;
    s += 1;
    if (s > max_restarts) {                                                           // :375
      w->restarts = s;
      return qp::fail(QP_E_MAX_RESTARTS, "newton!: s=%d exceeds max_restarts=%d (relerr=%g)", s, max_restarts, st.last_relerr);
    }
  }
  w->restarts = s;
  w->n_leja = n_leja;
  w->n_a = n_a;
  ctx->stats.n_newton_steps++;
  ctx->stats.n_restarts += s;
  st.restarts = s;
  st.n_a = n_a;
  st.n_leja = n_leja;
  st.m_last = m;
  st.radius = w->radius;
  st.sweeps_onepass = w->q->n_onepass - onepass0;
  st.sweeps_onepass_redone = w->q->n_onepass_redone - redone0;
  if (stats) *stats = st;
  return QP_OK;
  QP_CATCH
}

}  // extern "C"

// ---------------------------------------------------------------------------
// SpectralRange
// ---------------------------------------------------------------------------
namespace {

// Ritz values of the leading m x m block of Hess into ev, and their extent: smallest and largest real part, largest |imaginary part|
struct RitzExtent {
  double lo, hi, im;
};
int ritz_extent(const std::vector<cplx>& Hess, int ldh, int m, std::vector<cplx>& ev, RitzExtent* x) {
  ev.assign(m, cplx(0));
  if (qp::diagonalize_hessenberg(Hess.data(), ldh, m, false, ev.data()) != QP_OK)
    return qp::fail(QP_E_INTERNAL, "Hessenberg QR did not converge");
  *x = RitzExtent{ev[0].real(), ev[0].real(), std::fabs(ev[0].imag())};
  for (auto& z : ev) {
    x->lo = std::min(x->lo, z.real());
    x->hi = std::max(x->hi, z.real());
    x->im = std::max(x->im, std::fabs(z.imag()));
  }
  return QP_OK;
}

}  // namespace

extern "C" {

int qp_ritzvals(qp_operator* op, const qp_state* state, int m_min, int m_max, double prec, double norm_min,
                qp_c128* out, int* n_out) {
  QP_TRY
  if (!op || !state || !out || !n_out) return qp::fail(QP_E_BAD_ARG, "qp_ritzvals: NULL argument");
  if (m_max <= m_min) return qp::fail(QP_E_BAD_ARG, "m_max=%d must be larger than m_min=%d", m_max, m_min);  // src/specrad.jl:171-173
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  int m = std::max(5, std::min(m_min, m_max - 1));                         // :174
  if (m_max < m) return qp::fail(QP_E_BAD_ARG, "m_max=%d too small (need >= %d)", m_max, m);
  const int ldh = m_max;
  std::vector<cplx> Hess((size_t)ldh * ldh, cplx(0));
  qp_c128* H = reinterpret_cast<qp_c128*>(Hess.data());
  qp_krylov* q = nullptr;
  QP_CHECK(qp_krylov_create(ctx, state->n, m_max + 1, &q));
  std::unique_ptr<qp_krylov, int (*)(qp_krylov*)> guard(q, qp_krylov_destroy);
  std::vector<cplx> ev;
  RitzExtent x0, x;
  int m0 = m - 1;
  QP_CHECK(qp_arnoldi(op, q, m0, state, 1.0, 0, norm_min, H, ldh, &m0));  // :182
  QP_CHECK(ritz_extent(Hess, ldh, m0, ev, &x0));
  if (m0 == m - 1) {
    int ext = 0;
    QP_CHECK(qp_arnoldi_extend(op, q, m, 1.0, norm_min, H, ldh, &ext));  // :190
    QP_CHECK(ritz_extent(Hess, ldh, m, ev, &x));
    double er_lo = (x0.lo != 0.0) ? std::fabs(1.0 - x.lo / x0.lo) : 0.0;
    double er_hi = (x0.hi != 0.0) ? std::fabs(1.0 - x.hi / x0.hi) : 0.0;
    double ei = (x0.im != 0.0) ? std::fabs(1.0 - x.im / x0.im) : 0.0;
    while ((er_lo > prec) || (er_hi > prec) || ((x0.im > 1e-14) && ei > prec)) {   // :198
      x0 = x;
      m = m + 1;
      // quirk kept: the reference discards extend_arnoldi!'s return value, so Krylov
      // exhaustion is never detected here (:204-205)
      QP_CHECK(qp_arnoldi_extend(op, q, m, 1.0, norm_min, H, ldh, &ext));
      QP_CHECK(ritz_extent(Hess, ldh, m, ev, &x));
      er_lo = std::fabs(1.0 - (x.lo / x0.lo));   // (quirk kept: unguarded divisions inside the loop, :209-211)
      er_hi = std::fabs(1.0 - (x.hi / x0.hi));
      ei = std::fabs(1.0 - (x.im / x0.im));
      if (m == m_max) break;                                                     // :213-216
    }
  }
  *n_out = (int)ev.size();
  for (size_t i = 0; i < ev.size(); ++i) out[i] = qp_c128{ev[i].real(), ev[i].imag()};
  return QP_OK;
  QP_CATCH
}

int qp_specrange_arnoldi(qp_operator* op, const qp_state* state, int m_min, int m_max, double prec, double norm_min,
                         int enlarge, double* E_min, double* E_max) {
  QP_TRY
  if (!E_min || !E_max) return qp::fail(QP_E_BAD_ARG, "qp_specrange_arnoldi: NULL output");
  m_min = std::max(5, std::min(m_min, m_max - 1));                              // src/specrad.jl:97
  std::vector<qp_c128> R((size_t)std::max(m_max, 8));
  int n = 0;
  QP_CHECK(qp_ritzvals(op, state, m_min, m_max, prec, norm_min, R.data(), &n));
  double lo = R[0].re, hi = R[n - 1].re;                                        // :103-104
  if (enlarge && n > 1) {                                                        // :105-110
    lo = 2 * lo - R[1].re;
    hi = 2 * hi - R[n - 2].re;
  }
  *E_min = lo;
  *E_max = hi;
  return QP_OK;
  QP_CATCH
}

}  // extern "C"
