// C ABI of libqprop_hip.so, the part every other engine unit stands on: error plumbing, contexts and their tuning knobs,
// status names, matrices (canonical host CSR), states, host registration and BLAS-1.  Operators: engine_operator.hip.
// Device work is stream-ordered, with host synchronisation only where a scalar is needed on the host.
#include <mutex>
#include <atomic>

#include "engine.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
namespace qp {
// the context knobs by name (qp_tuning_set / qp_ctx_tuning_set / _get)
int* tuning_field(Tuning& t, const char* key) {
  struct Entry {
    const char* name;
    int Tuning::*field;
  };
  static const Entry table[] = {
      {"rbcsr_variant", &Tuning::rbcsr_variant},
      {"arnoldi_mode", &Tuning::arnoldi_mode},   {"arnoldi_onepass", &Tuning::arnoldi_onepass},   {"split_mode", &Tuning::split_mode},
            {"arnoldi_fuse_dots", &Tuning::arnoldi_fuse_dots},   {"lattice_fill", &Tuning::lattice_fill},   {"sparse_controls", &Tuning::sparse_controls},
      {"liouville_fused_n", &Tuning::liouville_fused_n}, {"liouville_tile32_n", &Tuning::liouville_tile32_n}, {"liouville_tile32_min_n", &Tuning::liouville_tile32_min_n}, {"real_vals", &Tuning::real_vals},
      {"stencil", &Tuning::stencil}, {"block_map", &Tuning::block_map},             {"acc_defer", &Tuning::acc_defer},
      {"cheby_graph", &Tuning::cheby_graph},     {"small_nnz", &Tuning::small_nnz},
      {"roctx", &Tuning::roctx}, 
      {"colblock", &Tuning::colblock}, {"cb_log2w", &Tuning::cb_log2w},
      {"dense_auto", &Tuning::dense_auto},       {"dense_panel_mfma", &Tuning::dense_panel_mfma},
      {"newton_pipeline", &Tuning::newton_pipeline}, 
      {"spmm_nt", &Tuning::spmm_nt},             {"spmm_rows", &Tuning::spmm_rows},
      {"spmm_strip", &Tuning::spmm_strip},       {"spmm_rw", &Tuning::spmm_rw},
      {"hrb_walk", &Tuning::hrb_walk},           {"walk_waves", &Tuning::walk_waves},
      {"walk_min_blocks", &Tuning::walk_min_blocks}, {"walk_dbg", &Tuning::walk_dbg}, {"walk_nt", &Tuning::walk_nt}, {"value_dict", &Tuning::value_dict}, {"walk_pair", &Tuning::walk_pair}, {"split_spin_log2", &Tuning::split_spin_log2}, {"split_dbg", &Tuning::split_dbg},
  };
  for (const Entry& e : table)
    if (std::strcmp(e.name, key) == 0) return &(t.*(e.field));
  return nullptr;
}

int device_cu_count() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 256;
  }
  int n = cached[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    n = 256;
  }
  cached[dev].store(n, std::memory_order_relaxed);
  return n;
}

static thread_local std::string g_last_error;
void set_error(const char* msg) { g_last_error = msg ? msg : ""; }
int fail(int status, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return status;
}
}  // namespace qp

// ---------------------------------------------------------------------------
// misc
// ---------------------------------------------------------------------------
extern "C" {

const char* qp_last_error(void) { return qp::g_last_error.c_str(); }

const char* qp_status_name(int s) {
  switch (s) {
    case QP_OK: return "QP_OK";
    case QP_E_BAD_ARG: return "QP_E_BAD_ARG";
    case QP_E_HIP: return "QP_E_HIP";
    case QP_E_DT_MISMATCH: return "QP_E_DT_MISMATCH";
    case QP_E_TOO_FEW_COEFFS: return "QP_E_TOO_FEW_COEFFS";
    case QP_E_NORMALIZATION: return "QP_E_NORMALIZATION";
    case QP_E_MAX_RESTARTS: return "QP_E_MAX_RESTARTS";
    case QP_E_DIVDIFF_UNDERFLOW: return "QP_E_DIVDIFF_UNDERFLOW";
    case QP_E_NO_DEVICE: return "QP_E_NO_DEVICE";
    case QP_E_ALLOC: return "QP_E_ALLOC";
    case QP_E_INTERNAL: return "QP_E_INTERNAL";
    case QP_E_M_MAX: return "QP_E_M_MAX";
    case QP_E_RCCL: return "QP_E_RCCL";
    default: return "QP_E_UNKNOWN";
  }
}

int qp_version(void) { return 100; }

}  // extern "C"

// defaults that new contexts start from (qp_tuning_set); a context's own copy is qp_ctx::tun
static std::mutex g_tuning_mutex;
static qp::Tuning g_tuning_defaults;

// Settings that change RESULTS (walk_dbg bit 1: the edge blocks of the strip walk are skipped) or force a failure
// (split_dbg: the boundary launches of a split term do not signal, every waiting wavefront runs into the time-out) exist for
// measurements and for the time-out test only: a release build refuses them; `make dev` (-DQP_DEVELOPER) builds the flavour
// that takes them (lib/libqprop_hip_dev.so, loaded with QPROP_HIP_LIB).
static int tuning_value_allowed(const char* key, int value) {
#ifndef QP_DEVELOPER
  if ((std::strcmp(key, "walk_dbg") == 0 && (value & 2)) || (std::strcmp(key, "split_dbg") == 0 && value != 0))
    return qp::fail(QP_E_BAD_ARG, "%s = %d is a developer-build setting (csrc: make dev; it changes results or forces a time-out)", key, value);
#endif
  (void)key;
  (void)value;
  return QP_OK;
}

extern "C" {

/* 1 for the developer flavour of the library (-DQP_DEVELOPER), 0 for the release build */
int qp_developer_build(void) {
#ifdef QP_DEVELOPER
  return 1;
#else
  return 0;
#endif
}

int qp_tuning_set(const char* key, int value) {
  if (!key) return qp::fail(QP_E_BAD_ARG, "key is NULL");
  QP_CHECK(tuning_value_allowed(key, value));
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  int* f = qp::tuning_field(g_tuning_defaults, key);
  if (!f) return qp::fail(QP_E_BAD_ARG, "unknown tuning key %s", key);
  *f = value;
  return QP_OK;
}

int qp_ctx_tuning_set(qp_ctx* ctx, const char* key, int value) {
  if (!ctx || !key) return qp::fail(QP_E_BAD_ARG, "qp_ctx_tuning_set: NULL argument");
  QP_CHECK(tuning_value_allowed(key, value));
  int* f = qp::tuning_field(ctx->tun, key);
  if (!f) return qp::fail(QP_E_BAD_ARG, "unknown tuning key %s", key);
  *f = value;
  return QP_OK;
}

int qp_ctx_tuning_get(qp_ctx* ctx, const char* key, int* value_out) {
  if (!ctx || !key || !value_out) return qp::fail(QP_E_BAD_ARG, "qp_ctx_tuning_get: NULL argument");
  const int* f = qp::tuning_field(ctx->tun, key);
  if (!f) return qp::fail(QP_E_BAD_ARG, "unknown tuning key %s", key);
  *value_out = *f;
  return QP_OK;
}

int qp_device_count(int* n_out) {
  QP_TRY
  if (!n_out) return qp::fail(QP_E_BAD_ARG, "n_out is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *n_out = n;
  return QP_OK;
  QP_CATCH
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
int qp_ctx_create(int device, void* stream, qp_ctx** out) {
  QP_TRY
  if (!out) return qp::fail(QP_E_BAD_ARG, "qp_ctx_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return qp::fail(QP_E_NO_DEVICE,
                    "no HIP device visible (%s): libqprop_hip has no CPU fallback for the prop_step! path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  }
  if (device < 0 || device >= n) return qp::fail(QP_E_BAD_ARG, "device %d out of range [0,%d)", device, n);
  QP_HIP(hipSetDevice(device));
  auto ctx = std::make_unique<qp_ctx>();
  ctx->device = device;
  {
    std::lock_guard<std::mutex> lock(g_tuning_mutex);
    ctx->tun = g_tuning_defaults;
  }
  if (stream == QP_STREAM_NULL) {
    ctx->stream = nullptr;   // HIP's null stream
  } else if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    QP_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  QP_HIP(hipEventCreate(&ctx->ev0));
  QP_HIP(hipEventCreate(&ctx->ev1));
  QP_CHECK(dev_alloc(&ctx->d_part, kRedBlocks));
  QP_HIP(hipHostMalloc((void**)&ctx->h_part, kRedBlocks * sizeof(double2), hipHostMallocDefault));
  *out = ctx.release();
  return QP_OK;
  QP_CATCH
}

int qp_ctx_destroy(qp_ctx* ctx) {
  QP_TRY
  if (!ctx || ctx->closed) return QP_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->d_part) (void)hipFree(ctx->d_part);
  if (ctx->h_part) (void)hipHostFree(ctx->h_part);
  for (int k = 0; k < 2; ++k) {
    if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
    if (ctx->stage_ev[k]) (void)hipEventDestroy(ctx->stage_ev[k]);
    ctx->stage[k] = nullptr;
    ctx->stage_ev[k] = nullptr;
  }
  ctx->stage_bytes = 0;
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  // the record stays (a few dozen bytes): child handles destroyed later still find their device in it
  ctx->d_part = nullptr;
  ctx->h_part = nullptr;
  ctx->ev0 = ctx->ev1 = nullptr;
  ctx->stream = nullptr;      // what a late child destroy synchronises: the null stream
  ctx->own_stream = false;
  ctx->closed = true;
  return QP_OK;
  QP_CATCH
}

int qp_sync(qp_ctx* ctx) {
  QP_TRY
  if (!ctx) return qp::fail(QP_E_BAD_ARG, "ctx is NULL");
  QP_CHECK(use(ctx));
  QP_HIP(hipStreamSynchronize(ctx->stream));
  return QP_OK;
  QP_CATCH
}

int qp_stats_get(qp_ctx* ctx, qp_stats* out) {
  if (!ctx || !out) return qp::fail(QP_E_BAD_ARG, "qp_stats_get: NULL argument");
  out->n_matvec = ctx->stats.n_matvec;
  out->n_cheby_steps = ctx->stats.n_cheby_steps;
  out->n_newton_steps = ctx->stats.n_newton_steps;
  out->n_restarts = ctx->stats.n_restarts;
  out->n_kernel_launches = ctx->stats.n_launch;
  out->spmv_bytes = ctx->stats.spmv_bytes;
  out->n_graph_launches = ctx->stats.n_graph_launch;
  out->n_pair_launches = ctx->stats.n_pair_launch;
  return QP_OK;
}

int qp_stats_reset(qp_ctx* ctx) {
  if (!ctx) return qp::fail(QP_E_BAD_ARG, "ctx is NULL");
  ctx->stats = Stats();
  return QP_OK;
}

int qp_timer_begin(qp_ctx* ctx) {
  QP_TRY
  if (!ctx) return qp::fail(QP_E_BAD_ARG, "ctx is NULL");
  QP_CHECK(use(ctx));
  QP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  return QP_OK;
  QP_CATCH
}

int qp_timer_end(qp_ctx* ctx, double* elapsed_ms_out) {
  QP_TRY
  if (!ctx || !elapsed_ms_out) return qp::fail(QP_E_BAD_ARG, "qp_timer_end: NULL argument");
  QP_CHECK(use(ctx));
  QP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  QP_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0;
  QP_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *elapsed_ms_out = ms;
  return QP_OK;
  QP_CATCH
}

// ---------------------------------------------------------------------------
// matrices: canonicalise to host CSR (bit-exact index work)
// ---------------------------------------------------------------------------
int qp_matrix_create(qp_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* ptr,
                     const int64_t* idx, const void* vals, int val_dtype, int layout, int index_base,
                     int format, qp_matrix** out) {
  QP_TRY
  (void)format;
  if (!ctx || !out || !ptr || (nnz > 0 && (!idx || !vals)))
    return qp::fail(QP_E_BAD_ARG, "qp_matrix_create: NULL argument");
  if (nrows < 0 || ncols < 0 || nnz < 0 || ncols > INT32_MAX)   // columns are int32 on the device
    return qp::fail(QP_E_BAD_ARG, "qp_matrix_create: bad shape %lld x %lld, nnz %lld", (long long)nrows,
                    (long long)ncols, (long long)nnz);
  if (index_base != 0 && index_base != 1) return qp::fail(QP_E_BAD_ARG, "index_base must be 0 or 1");
  if (val_dtype != QP_VAL_C128 && val_dtype != QP_VAL_F64) return qp::fail(QP_E_BAD_ARG, "bad val_dtype");
  auto m = std::make_unique<qp_matrix>();
  m->ctx = ctx;
  m->nrows = nrows;
  m->ncols = ncols;
  m->nnz = nnz;
  m->rowptr.resize(nrows + 1);
  m->col.resize(nnz);
  m->vals.resize(nnz);
  qp::HostVec<qp_c128> cv;
  const qp_c128* v128 = nullptr;
  if (val_dtype == QP_VAL_F64) {
    cv.resize(nnz);
    const double* r = static_cast<const double*>(vals);
    parallel_rows(nnz, [&](int64_t p0, int64_t p1) {
      for (int64_t p = p0; p < p1; ++p) cv[p] = qp_c128{r[p], 0.0};
    }, (int64_t)1 << 20);
    v128 = cv.data();
  } else {
    v128 = static_cast<const qp_c128*>(vals);
  }
  if (layout == QP_LAYOUT_CSC) {
    if (ptr[ncols] - index_base != nnz) return qp::fail(QP_E_BAD_ARG, "colptr[end] does not match nnz");
    int st = qp::csc_to_csr(nrows, ncols, ptr, idx, v128, index_base, m->rowptr.data(), m->col.data(),
                            reinterpret_cast<qp_c128*>(m->vals.data()));
    if (st != QP_OK)
      return qp::fail(st, "qp_matrix_create: colptr must start at the index base, be monotone and end at nnz, and every "
                          "row index must lie in [base, base + nrows)");
  } else if (layout == QP_LAYOUT_CSR) {
    if (ptr[nrows] - index_base != nnz) return qp::fail(QP_E_BAD_ARG, "rowptr[end] does not match nnz");
    if (ptr[0] != index_base) return qp::fail(QP_E_BAD_ARG, "rowptr[0] must equal the index base (%d)", index_base);
    // rows in chunks on the host threads (N = 2^24: 5 GB of index and value arrays; one thread took 1.5 s): the copy with its range
    // checks, then per row the canonical form -- columns ascending (stable: duplicates keep their order and are summed later)
    std::atomic<int64_t> bad_row{-1}, bad_col{-1};
    parallel_rows(nrows + 1, [&](int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1; ++r) m->rowptr[r] = ptr[r] - index_base;
    });
    parallel_rows(nrows, [&](int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1; ++r)
        if (m->rowptr[r + 1] < m->rowptr[r] || m->rowptr[r] < 0 || m->rowptr[r + 1] > nnz) {
          int64_t none = -1;
          bad_row.compare_exchange_strong(none, r);
          return;
        }
    });
    if (bad_row.load() >= 0) return qp::fail(QP_E_BAD_ARG, "rowptr not monotone at row %lld", (long long)bad_row.load());
    parallel_rows(nrows, [&](int64_t r0, int64_t r1) {
      std::vector<std::pair<int32_t, cplx>> tmp;
      for (int64_t r = r0; r < r1; ++r) {
        const int64_t a = m->rowptr[r], b = m->rowptr[r + 1];
        bool sorted = true;
        for (int64_t p = a; p < b; ++p) {
          const int64_t c = idx[p] - index_base;
          if (c < 0 || c >= ncols) {
            int64_t none = -1;
            bad_col.compare_exchange_strong(none, p);
            return;
          }
          m->col[p] = (int32_t)c;
          m->vals[p] = cplx(v128[p].re, v128[p].im);
          if (p > a && m->col[p] < m->col[p - 1]) sorted = false;
        }
        if (sorted) continue;
        tmp.resize((size_t)(b - a));
        for (int64_t p = a; p < b; ++p) tmp[(size_t)(p - a)] = {m->col[p], m->vals[p]};
        std::stable_sort(tmp.begin(), tmp.end(), [](auto& x, auto& y) { return x.first < y.first; });
        for (int64_t p = a; p < b; ++p) { m->col[p] = tmp[(size_t)(p - a)].first; m->vals[p] = tmp[(size_t)(p - a)].second; }
      }
    });
    if (bad_col.load() >= 0) return qp::fail(QP_E_BAD_ARG, "column index out of range at %lld", (long long)bad_col.load());
  } else {
    return qp::fail(QP_E_BAD_ARG, "bad layout");
  }
  *out = m.release();
  return QP_OK;
  QP_CATCH
}

int qp_matrix_destroy(qp_matrix* m) {
  delete m;
  return QP_OK;
}

int qp_matrix_info(const qp_matrix* m, int64_t* nrows, int64_t* ncols, int64_t* nnz, int* format,
                   int64_t* stored_nnz) {
  if (!m) return qp::fail(QP_E_BAD_ARG, "matrix is NULL");
  if (nrows) *nrows = m->nrows;
  if (ncols) *ncols = m->ncols;
  if (nnz) *nnz = m->nnz;
  if (format) *format = QP_FMT_CSR;
  if (stored_nnz) *stored_nnz = m->nnz;
  return QP_OK;
}

int qp_matrix_get_csr(const qp_matrix* m, int64_t* rowptr, int32_t* col, qp_c128* vals) {
  if (!m || !rowptr || !col || !vals) return qp::fail(QP_E_BAD_ARG, "qp_matrix_get_csr: NULL argument");
  std::memcpy(rowptr, m->rowptr.data(), (m->nrows + 1) * sizeof(int64_t));
  std::memcpy(col, m->col.data(), m->nnz * sizeof(int32_t));
  std::memcpy(vals, m->vals.data(), m->nnz * sizeof(qp_c128));
  return QP_OK;
}

// ---------------------------------------------------------------------------
// states and BLAS-1
// ---------------------------------------------------------------------------
int qp_state_create(qp_ctx* ctx, int64_t n, qp_state** out) {
  QP_TRY
  if (!ctx || !out || n < 0) return qp::fail(QP_E_BAD_ARG, "qp_state_create: bad arguments");
  QP_CHECK(use(ctx));
  auto s = std::make_unique<qp_state>();
  s->ctx = ctx;
  s->n = n;
  s->own = true;
  QP_CHECK(dev_alloc(&s->d, (size_t)n));
  QP_HIP(hipMemsetAsync(s->d, 0, (size_t)n * sizeof(double2), ctx->stream));
  *out = s.release();
  return QP_OK;
  QP_CATCH
}

int qp_state_wrap(qp_ctx* ctx, void* device_ptr, int64_t n, qp_state** out) {
  QP_TRY
  if (!ctx || !out || !device_ptr || n < 0) return qp::fail(QP_E_BAD_ARG, "qp_state_wrap: bad arguments");
  if ((uintptr_t)device_ptr % 16 != 0) return qp::fail(QP_E_BAD_ARG, "device pointer must be 16-byte aligned");
  auto s = std::make_unique<qp_state>();
  s->ctx = ctx;
  s->d = static_cast<double2*>(device_ptr);
  s->n = n;
  s->own = false;
  *out = s.release();
  return QP_OK;
  QP_CATCH
}

int qp_state_destroy(qp_state* s) {
  QP_TRY
  if (!s) return QP_OK;
  if (s->own) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    (void)hipFree(s->d);
  }
  delete s;
  return QP_OK;
  QP_CATCH
}

int qp_state_upload(qp_state* s, const qp_c128* host) {
  QP_TRY
  if (!s || !host) return qp::fail(QP_E_BAD_ARG, "qp_state_upload: NULL argument");
  QP_CHECK(use(s->ctx));
  QP_HIP(hipMemcpyAsync(s->d, host, (size_t)s->n * sizeof(double2), hipMemcpyHostToDevice, s->ctx->stream));
  QP_HIP(hipStreamSynchronize(s->ctx->stream));
  return QP_OK;
  QP_CATCH
}

int qp_state_download(const qp_state* s, qp_c128* host) {
  QP_TRY
  if (!s || !host) return qp::fail(QP_E_BAD_ARG, "qp_state_download: NULL argument");
  QP_CHECK(use(s->ctx));
  QP_HIP(hipMemcpyAsync(host, s->d, (size_t)s->n * sizeof(double2), hipMemcpyDeviceToHost, s->ctx->stream));
  QP_HIP(hipStreamSynchronize(s->ctx->stream));
  return QP_OK;
  QP_CATCH
}

int qp_host_register(void* host, size_t bytes) {
  QP_TRY
  if (!host || bytes == 0) return qp::fail(QP_E_BAD_ARG, "qp_host_register: NULL / empty array");
  // portable: the registration holds for every device / context of the process, so it may be undone from
  // any thread (a garbage collector's finalizer thread included), whichever device is current there
  QP_HIP(hipHostRegister(host, bytes, hipHostRegisterPortable));
  return QP_OK;
  QP_CATCH
}

int qp_host_unregister(void* host) {
  QP_TRY
  if (!host) return qp::fail(QP_E_BAD_ARG, "qp_host_unregister: NULL");
  QP_HIP(hipHostUnregister(host));
  return QP_OK;
  QP_CATCH
}

void* qp_state_ptr(const qp_state* s) { return s ? s->d : nullptr; }
int64_t qp_state_len(const qp_state* s) { return s ? s->n : -1; }

int qp_copy(qp_state* dst, const qp_state* src) {
  QP_TRY
  if (!dst || !src || dst->n != src->n) return qp::fail(QP_E_BAD_ARG, "qp_copy: length mismatch");
  QP_CHECK(use(dst->ctx));
  if (dst->d != src->d)
    QP_HIP(hipMemcpyAsync(dst->d, src->d, (size_t)dst->n * sizeof(double2), hipMemcpyDeviceToDevice, dst->ctx->stream));
  return QP_OK;
  QP_CATCH
}

int qp_scal(qp_state* x, qp_c128 alpha) {
  QP_TRY
  if (!x) return qp::fail(QP_E_BAD_ARG, "state is NULL");
  QP_CHECK(use(x->ctx));
  return qp::launch_scal(x->ctx->stream, x->d, d2(alpha), x->n, &x->ctx->stats);
  QP_CATCH
}

int qp_axpy(qp_c128 alpha, const qp_state* x, qp_state* y) {
  QP_TRY
  if (!x || !y || x->n != y->n) return qp::fail(QP_E_BAD_ARG, "qp_axpy: length mismatch");
  QP_CHECK(use(y->ctx));
  return qp::launch_axpy(y->ctx->stream, d2(alpha), x->d, y->d, y->n, &y->ctx->stats);
  QP_CATCH
}

int qp_fill(qp_state* x, qp_c128 alpha) {
  QP_TRY
  if (!x) return qp::fail(QP_E_BAD_ARG, "state is NULL");
  QP_CHECK(use(x->ctx));
  return qp::launch_fill(x->ctx->stream, x->d, d2(alpha), x->n, &x->ctx->stats);
  QP_CATCH
}

int qp_dot(const qp_state* x, const qp_state* y, qp_c128* out) {
  QP_TRY
  if (!x || !y || !out || x->n != y->n) return qp::fail(QP_E_BAD_ARG, "qp_dot: bad arguments");
  QP_CHECK(use(x->ctx));
  cplx r;
  QP_CHECK(dot_sync(x->ctx, x->d, y->d, x->n, &r));
  *out = qp_c128{r.real(), r.imag()};
  return QP_OK;
  QP_CATCH
}

int qp_norm(const qp_state* x, double* out) {
  QP_TRY
  if (!x || !out) return qp::fail(QP_E_BAD_ARG, "qp_norm: bad arguments");
  QP_CHECK(use(x->ctx));
  cplx r;
  QP_CHECK(dot_sync(x->ctx, x->d, x->d, x->n, &r));
  *out = std::sqrt(r.real());
  return QP_OK;
  QP_CATCH
}

int qp_mul(qp_operator* op, const qp_state* x, qp_state* y, qp_c128 alpha, qp_c128 beta) {
  QP_TRY
  if (!op || !x || !y) return qp::fail(QP_E_BAD_ARG, "qp_mul: NULL argument");
  if (x->n != op->A.ncols || y->n != op->A.nrows)
    return qp::fail(QP_E_BAD_ARG, "qp_mul: shape mismatch (op %lld x %lld, x %lld, y %lld)", (long long)op->A.nrows,
                    (long long)op->A.ncols, (long long)x->n, (long long)y->n);
  if (x->d == y->d) return qp::fail(QP_E_BAD_ARG, "qp_mul: x and y must not alias");
  QP_CHECK(use(op->ctx));
  qp::PlainEpi e;
  e.y = y->d;
  e.alpha = d2(alpha);
  e.beta = d2(beta);
  e.beta_zero = (beta.re == 0.0 && beta.im == 0.0);
  return qp::launch_spmv_plain(op->ctx->stream, op->A, x->d, e, &op->ctx->stats);
  QP_CATCH
}

int qp_dot_op(const qp_state* x, qp_operator* op, const qp_state* y, qp_state* tmp, qp_c128* out) {
  QP_TRY
  if (!x || !op || !y || !tmp || !out) return qp::fail(QP_E_BAD_ARG, "qp_dot_op: NULL argument");
  QP_CHECK(qp_mul(op, y, tmp, qp_c128{1, 0}, qp_c128{0, 0}));
  return qp_dot(x, tmp, out);
  QP_CATCH
}

}  // extern "C"
