// Operators of the C ABI (the lazy sum of include/qprop.h): creation, the device build, evaluate! (operator_refresh), the
// *_info getters and qp_operator_get_csr.  A thin device layer: WHAT the arrays hold is computed by the pure-host layout unit
// (operator_layout.h) and by the pure-host planning unit (operator_plans.h, through engine_plans.hip); this file uploads the results, phase by phase.
#include <atomic>

#include "engine_host.h"

// ---------------------------------------------------------------------------
// Operator: union pattern + value planes in HBM
// ---------------------------------------------------------------------------
static int operator_free_device(qp_operator* op) {
  DevMatrix& A = op->A;
  for (auto& p : op->planes) dev_release(p);
  op->planes.clear();
  dev_release(op->planes_dev);
  dev_release(op->combined);
  dev_release(op->support);
  dev_release(op->support_vals);
  dev_release(op->base);
  op->sparse_from = -1;
  op->n_support = 0;
  op->base_valid = false;
  dev_release(op->real_vals);
  op->real_of = nullptr;
  A.vals = nullptr;
  A.vals_r = nullptr;
  dev_release(A.bptr);
  dev_release(A.rowptr);
  dev_release(A.cols);
  dev_release(A.cmeta);
  dev_release(A.lptr);
  dev_release(A.lcols);
  dev_release(A.lcmeta);
  dev_release(A.lpos);
  dev_release(op->walk.edge_map);
  op->walk = qp::WalkPlan();
  dev_release(op->walk2.edge_map);
  op->walk2 = qp::WalkPlan();
  A.walk = nullptr;
  dev_release(op->cb.segptr);
  dev_release(op->cb.rowoff);
  dev_release(op->cb.cols);
  dev_release(op->cb.map);
  dev_release(op->cb.vals);
  dev_release(op->cb.vals_r);
  op->cb = qp::ColBlockPlan();
  A.cb = nullptr;
  for (auto& p : op->cv_tplanes) dev_release(p);
  op->cv_tplanes.clear();
  dev_release(op->cv_tplanes_dev);
  dev_release(op->cv_tab_comb);
  dev_release(op->cv.codes);
  dev_release(op->cv.tptr);
  dev_release(op->cv.tab_r);
  op->cv = qp::CodedVals();
  A.cv = nullptr;
  dev_release(op->m_rowptr);
  dev_release(op->m_cols);
  dev_release(op->m_map);
  dev_release(op->m_vals);
  dev_release(op->m_order);
  op->m_order_valid = false;
  dev_release(op->m_tiles.tiles);
  dev_release(op->m_tiles.rest);
  dev_release(op->m_tiles.tab);
  op->m_tiles = qp::SpmmTiles();
  op->m_epoch = 0;
  return QP_OK;
}

static int operator_free(qp_operator* op) {
  if (!op) return QP_OK;
  (void)hipSetDevice(op->ctx->device);
  (void)hipStreamSynchronize(op->ctx->stream);
  if (op->mf_free) op->mf_free(op);
  operator_free_device(op);
  delete op;
  return QP_OK;
}


// ---- the device build, phase by phase: compute with the layout unit, upload ------------------------------------------
// CSR layouts (QP_FMT_DENSE: the same arrays with a complete pattern, vals[r ncols + c])
static int build_csr_arrays(qp_operator* op) {
  DevMatrix& A = op->A;
  const int64_t nnz = op->u_rowptr[A.nrows];
  A.stored = nnz;
  QP_CHECK(dev_upload(&A.rowptr, op->u_rowptr.data(), op->u_rowptr.size()));
  QP_CHECK(dev_upload(&A.cols, op->u_col.data(), (size_t)nnz));
  double mean = A.nrows > 0 ? (double)nnz / (double)A.nrows : 1.0;
  int T = 2;
  while (T < 64 && T < mean) T *= 2;
  A.lanes_per_row = T;
  return QP_OK;
}

// row-block layouts: pointers, column sections and -- Hermitian-packed -- the lower sections, transposed positions, walk plan
static int build_row_blocks(qp_operator* op, BuildTrace& trace) {
  const qp::Tuning& tun = op->ctx->tun;
  DevMatrix& A = op->A;
  HostLayout& Lh = op->layout;
  const auto& ur = op->u_rowptr;
  const auto& uc = op->u_col;
  block_pointers(A.nrows, ur, uc, Lh);
  A.stored = Lh.stored;
  A.lstored = Lh.lstored;
  trace.mark("  block widths and pointers");
  std::vector<char> cbytes;
  encode_upper_sections(A.nrows, A.ncols, ur, uc, Lh, tun.stencil != 0, tun.block_map != 0, cbytes);
  A.colbytes = (int64_t)cbytes.size();
  QP_CHECK(dev_upload(reinterpret_cast<char**>(&A.cols), cbytes.data(), cbytes.size()));
  QP_CHECK(dev_upload(&A.cmeta, Lh.cmeta.data(), Lh.cmeta.size()));
  QP_CHECK(dev_upload(&A.bptr, Lh.bptr.data(), Lh.bptr.size()));
  trace.mark("  upper column sections + upload");
  if (Lh.format != QP_FMT_HRB) return QP_OK;
  if (Lh.stored >= (int64_t)INT32_MAX) return qp::fail(QP_E_BAD_ARG, "Hermitian-packed format needs < 2^31 stored values per GPU");
  qp::HostVec<int32_t> lpos;
  transposed_positions(A.nrows, ur, uc, Lh, lpos);
  std::vector<char> lbytes;
  encode_lower_sections(A.nrows, A.ncols, ur, uc, Lh, lpos, tun.stencil != 0, tun.block_map != 0, lbytes);
  A.lcolbytes = (int64_t)lbytes.size();
  QP_CHECK(dev_upload(&A.lptr, Lh.lptr.data(), Lh.lptr.size()));
  QP_CHECK(dev_alloc(reinterpret_cast<char**>(&A.lcols), std::max<size_t>(lbytes.size(), 16)));
  if (!lbytes.empty()) QP_HIP(hipMemcpy(A.lcols, lbytes.data(), lbytes.size(), hipMemcpyHostToDevice));
  QP_CHECK(dev_upload(&A.lcmeta, Lh.lcmeta.data(), Lh.lcmeta.size()));
  QP_CHECK(dev_upload(&A.lpos, lpos.data(), lpos.size()));
  trace.mark("  lower sections (positions, stencils) + upload");
  QP_CHECK(build_walk_plan(op));
  trace.mark("  strip-walk plan");
  return QP_OK;
}

constexpr size_t kStageBytes = (size_t)64 << 20;

// a large plane: units in chunks of 64 MiB, written in device order into one of two pinned buffers by the host threads while
// the other buffer's chunk is on its way to the device (one pageable 2.4 GB copy after a 2.4 GB fill took 0.42 s at N = 2^24)
static int upload_plane_staged(qp_operator* op, const PlaneView& pv, double2* dp) {
  qp_ctx* ctx = op->ctx;
  const DevMatrix& A = op->A;
  const HostLayout& Lh = op->layout;
  const auto& ur = op->u_rowptr;
  if (ctx->stage_bytes < kStageBytes) {
    for (int k = 0; k < 2; ++k) {
      if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
      ctx->stage[k] = nullptr;
      QP_HIP(hipHostMalloc(&ctx->stage[k], kStageBytes, hipHostMallocDefault));
      if (!ctx->stage_ev[k]) QP_HIP(hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
    }
    ctx->stage_bytes = kStageBytes;
  }
  const int64_t cap = (int64_t)(kStageBytes / sizeof(cplx)), nunits = (A.nrows + kRB - 1) / kRB;
  int which = 0;
  bool used[2] = {false, false};
  for (int64_t u0 = 0; u0 < nunits;) {
    const int64_t u1 = chunk_end(Lh, A.nrows, ur, nunits, u0, cap);
    const int64_t p0 = unit_pos(Lh, A.nrows, ur, u0), p1 = unit_pos(Lh, A.nrows, ur, u1);
    if (p1 - p0 > cap) return qp::fail(QP_E_BAD_ARG, "operator build: a 64-row block of %lld stored values exceeds the staging buffer", (long long)(p1 - p0));
    cplx* buf = static_cast<cplx*>(ctx->stage[which]);
    if (used[which]) QP_HIP(hipEventSynchronize(ctx->stage_ev[which]));
    plane_device_order(Lh, ur, op->u_col, pv, u0 * kRB, std::min(A.nrows, u1 * kRB), p0, p1, buf, (int64_t)1 << 18, 1024);
    if (p1 > p0) QP_HIP(hipMemcpyAsync(dp + p0, buf, (size_t)(p1 - p0) * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QP_HIP(hipEventRecord(ctx->stage_ev[which], ctx->stream));
    used[which] = true;
    which ^= 1;
    u0 = u1;
  }
  const int64_t pend = unit_pos(Lh, A.nrows, ur, nunits);      // (the slack behind the last block: zeros)
  if (A.stored > pend) QP_HIP(hipMemsetAsync(dp + pend, 0, (size_t)(A.stored - pend) * sizeof(double2), ctx->stream));
  QP_HIP(hipStreamSynchronize(ctx->stream));
  return QP_OK;
}

// any other plane: the whole of it in device order in `hplane` (max(stored, 1) values), one pageable copy
static int upload_plane_pageable(qp_operator* op, const PlaneView& pv, double2* dp, cplx* hplane) {
  const DevMatrix& A = op->A;
  plane_device_order(op->layout, op->u_rowptr, op->u_col, pv, 0, A.nrows, 0, std::max<int64_t>(A.stored, 1), hplane, (int64_t)1 << 20, (int64_t)1 << 16);
  QP_HIP(hipMemcpy(dp, hplane, (size_t)A.stored * sizeof(double2), hipMemcpyHostToDevice));
  return QP_OK;
}

static int build_value_planes(qp_operator* op, const Planes& planes_csr) {
  DevMatrix& A = op->A;
  const int nops = (int)planes_csr.size();
  op->planes_real = planes_all_real(planes_csr);
  // (raw storage: a std::vector would zero its gigabytes serially before the threaded fill does it again)
  std::unique_ptr<cplx, void (*)(void*)> hplane(nullptr, std::free);
  for (int l = 0; l < nops; ++l) {
    double2* dp = nullptr;
    QP_CHECK(dev_alloc(&dp, (size_t)A.stored));
    op->planes.push_back(dp);
    // (a plane that may belong to the sparse suffix stays whole on the host side: one copy)
    if (!sparse_candidate(nops, op->ncoeffs, A.stored, l) && (size_t)A.stored * sizeof(cplx) >= 4 * kStageBytes) {
      QP_CHECK(upload_plane_staged(op, planes_csr[l], dp));
      continue;
    }
    const size_t hplane_n = (size_t)std::max<int64_t>(A.stored, 1);
    if (!hplane) hplane.reset(static_cast<cplx*>(std::malloc(hplane_n * sizeof(cplx))));
    if (!hplane) return qp::fail(QP_E_ALLOC, "out of host memory building the operator (%zu bytes)", hplane_n * sizeof(cplx));
    QP_CHECK(upload_plane_pageable(op, planes_csr[l], dp, hplane.get()));
  }
  hplane.reset();
  const SparseControls sc = find_sparse_controls(op->layout, A.nrows, A.stored, op->u_rowptr, op->u_col, planes_csr, op->ncoeffs, qp::kCoefBlock);
  if (sc.sparse_from >= 0) {
    QP_CHECK(dev_upload(&op->support, sc.support.data(), sc.support.size()));
    QP_CHECK(dev_upload(&op->support_vals, sc.support_vals.data(), sc.support_vals.size()));
    op->sparse_from = sc.sparse_from;
    op->n_support = (int64_t)sc.support.size();
  }
  QP_CHECK(dev_upload(&op->planes_dev, op->planes.data(), (size_t)nops));
  A.vals = op->planes[0];
  return QP_OK;
}

// Value-dictionary mirror (device.h: CodedVals) of a row-block operator, where the layout unit finds one worth having
static int build_coded_values(qp_operator* op, const Planes& planes_csr) {
  DevMatrix& A = op->A;
  ValueDict vd;
  build_value_dict(op->ctx->tun.value_dict != 0, A.nrows, A.nblocks, A.stored, op->planes_real, op->layout, op->u_rowptr, planes_csr, vd);
  op->cv_reason = vd.reason;
  if (vd.reason != 0) return QP_OK;
  qp::CodedVals& C = op->cv;
  C.ntab = vd.ntab;
  C.ntables = vd.ntables;
  QP_CHECK(dev_upload(&C.codes, vd.codes.data(), vd.codes.size()));
  QP_CHECK(dev_upload(&C.tptr, vd.tptr.data(), vd.tptr.size()));
  for (const auto& col : vd.tab) {
    double2* dp = nullptr;
    QP_CHECK(dev_upload(&dp, col.data(), col.size()));
    op->cv_tplanes.push_back(dp);
  }
  QP_CHECK(dev_upload(&op->cv_tplanes_dev, op->cv_tplanes.data(), op->cv_tplanes.size()));
  C.tab = op->cv_tplanes[0];
  C.valid = 1;
  A.cv = &op->cv;
  return QP_OK;
}

// Build every device array of `op` for `format` from the union pattern (op->u_rowptr / u_col) and the per-term values given in
// union-CSR order.  Timed: format conversion, encoding and upload are host work at qp_operator_create (and once more if a complex
// coefficient forces a Hermitian-packed operator back to plain row blocks); qp_operator_build_info reports it
static int operator_build_device(qp_operator* op, int format, const Planes& planes_csr) {
  const auto t0 = std::chrono::steady_clock::now();
  BuildTrace trace;
  op->A.nblocks = (op->A.nrows + kRB - 1) / kRB;
  op->A.format = format;
  op->layout = HostLayout();
  op->layout.format = format;
  int rc = qp::csr_layout(format) ? build_csr_arrays(op) : build_row_blocks(op, trace);
  if (rc == QP_OK) rc = build_value_planes(op, planes_csr);
  trace.mark("  value planes in device order + upload");
  if (rc == QP_OK) rc = build_colblock(op);
  trace.mark("  column-block plan");
  if (rc == QP_OK && !(op->cb.valid && op->ctx->tun.colblock != 0)) rc = build_coded_values(op, planes_csr);
  trace.mark("  value dictionary");
  op->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  op->build_ms_total += op->build_ms;
  op->n_builds++;
  return rc;
}

// current per-term values (device planes) back in union-CSR order: download a plane, gather through the value map
static int operator_download_planes(qp_operator* op, Planes& planes_csr) {
  const DevMatrix& A = op->A;
  const int64_t nnz = op->u_rowptr[A.nrows];
  QP_HIP(hipStreamSynchronize(op->ctx->stream));
  std::vector<int64_t> map;
  csr_value_map(op->layout, A.nrows, op->u_rowptr, op->u_col, map);
  std::vector<cplx> hv((size_t)std::max<int64_t>(A.stored, 1));
  planes_csr.clear();
  planes_csr.resize(op->planes.size());
  for (size_t l = 0; l < op->planes.size(); ++l) {
    QP_HIP(hipMemcpy(hv.data(), op->planes[l], (size_t)A.stored * sizeof(double2), hipMemcpyDeviceToHost));
    auto& out = planes_csr[l].make_own((size_t)nnz);
    for (int64_t p = 0; p < nnz; ++p) out[p] = map[p] >= 0 ? hv[(size_t)map[p]] : std::conj(hv[(size_t)(-map[p] - 1)]);
  }
  return QP_OK;
}

static int pick_format(qp_operator* op, int requested, bool hermitian, int* fmt) {
  *fmt = choose_format(op, requested, hermitian);
  if (*fmt < 0) return qp::fail(QP_E_BAD_ARG, "QP_FMT_HRB requested but the operator terms are not exactly Hermitian");
  return QP_OK;
}

// back to the union pattern as it was before the lattice completion (ur_orig / uc_orig), and the terms' values in it
static void take_completion_back(qp_operator* op, const std::vector<TermCsr>& terms, bool canonical, qp::HostVec<int64_t>& ur_orig,
                                 qp::HostVec<int32_t>& uc_orig, Planes& planes_csr) {
  op->u_rowptr.swap(ur_orig);
  op->u_col.swap(uc_orig);
  ur_orig.clear();
  uc_orig.clear();
  op->n_lattice_fill = 0;
  for (auto& pv : planes_csr) pv.clear();
  op->A.nnz = op->u_rowptr[op->A.nrows];
  scatter_terms(terms, canonical, op->A.nrows, op->u_rowptr, op->u_col, planes_csr);
}

extern "C" {

int qp_operator_create(qp_ctx* ctx, qp_matrix* const* ops, int nops, int ncoeffs, int format,
                       qp_operator** out) {
  QP_TRY
  if (!ctx || !ops || !out || nops < 1 || ncoeffs < 0 || ncoeffs > nops)
    return qp::fail(QP_E_BAD_ARG, "qp_operator_create: bad arguments");
  for (int l = 0; l < nops; ++l) {
    if (!ops[l]) return qp::fail(QP_E_BAD_ARG, "ops[%d] is NULL", l);
    if (ops[l]->nrows != ops[0]->nrows || ops[l]->ncols != ops[0]->ncols)
      return qp::fail(QP_E_BAD_ARG, "ops[%d] shape differs from ops[0]", l);
  }
  if (format < QP_FMT_AUTO || (format > QP_FMT_HRB && format != QP_FMT_DENSE)) return qp::fail(QP_E_BAD_ARG, "bad device format %d", format);
  QP_CHECK(use(ctx));
  std::unique_ptr<qp_operator, int (*)(qp_operator*)> op(new qp_operator(), operator_free);
  op->ctx = ctx;
  op->A.tun = &ctx->tun;
  op->nops = nops;
  op->ncoeffs = ncoeffs;
  op->coeffs.assign(ncoeffs, cplx(1.0));
  const int64_t nrows = ops[0]->nrows, ncols = ops[0]->ncols;
  op->A.nrows = nrows;
  op->A.ncols = ncols;

  const auto t_create = std::chrono::steady_clock::now();
  BuildTrace trace;
  // ---- union sparsity pattern (sorted merge per row) ----
  auto& ur = op->u_rowptr;
  auto& uc = op->u_col;
  std::vector<TermCsr> terms;
  for (int l = 0; l < nops; ++l) terms.push_back(TermCsr{ops[l]->rowptr, ops[l]->col, ops[l]->vals});
  const bool canonical = union_pattern(terms, nrows, ur, uc);
  trace.mark("union pattern");
  // ---- a dense generator (QP_FMT_DENSE): requested, or AUTO with at least kDenseMinDensityPct % of the positions stored.
  // The pattern is made complete (the missing positions become explicit zeros, counted like the lattice completion's), so
  // that the CSR-ordered value array IS the row-major dense matrix and the dense kernels need no index at all.
  bool dense = false;
  {
    const double positions = (double)nrows * (double)ncols;
    if (format == QP_FMT_DENSE) {
      if (positions > (double)INT32_MAX) return qp::fail(QP_E_BAD_ARG, "QP_FMT_DENSE: %lld x %lld positions exceed the 2^31 limit", (long long)nrows, (long long)ncols);
      dense = nrows > 0 && ncols > 0;
    } else if (format == QP_FMT_AUTO && ctx->tun.dense_auto && nrows > 0 && ncols > 0 && positions <= 1073741824.0) {
      dense = 100.0 * (double)ur[nrows] >= (double)qp::kDenseMinDensityPct * positions;
    }
  }
  if (dense) {
    const int64_t before = ur[nrows];
    dense_complete(nrows, ncols, ur, uc);
    op->n_lattice_fill = ur[nrows] - before;
  }
  // Lattice completion (explicit zeros) is for operators that END UP Hermitian-packed with a strip-walk plan; whether this
  // one does is known only after the Hermitian check and the format choice below, which need the values.  So: complete
  // tentatively, keep the original pattern, and take the completion back if the operator turns out non-Hermitian, is laid
  // out otherwise, or has no plan after all (a non-Hermitian lattice-shaped Liouvillian kept up to 12 % stored
  // zeros for nothing -- more bytes per mat-vec, and 0 * Inf = NaN where the reference has no entry).
  qp::HostVec<int64_t> ur_orig;
  qp::HostVec<int32_t> uc_orig;
  if (!dense && (format == QP_FMT_AUTO || format == QP_FMT_HRB)) {
    const int64_t before = ur[nrows];
    lattice_fill(plan_knobs(ctx->tun), nrows, ncols, ur, uc, &ur_orig, &uc_orig);      // (ur_orig / uc_orig stay empty when nothing was completed)
    op->n_lattice_fill = ur[nrows] - before;
    if (op->n_lattice_fill == 0) {
      ur_orig.clear();
      uc_orig.clear();
    }
  }

  trace.mark("lattice completion");
  // ---- per-term values in union order (duplicates within a row are summed, as Julia's sparse() does) ----
  Planes planes_csr((size_t)nops);
  op->A.nnz = ur[nrows];
  scatter_terms(terms, canonical, nrows, ur, uc, planes_csr);
  trace.mark("value planes in union order");
  bool hermitian = !dense && (ncols >= nrows) && (format == QP_FMT_AUTO || format == QP_FMT_HRB);
  for (int l = 0; hermitian && l < nops; ++l) hermitian = csr_is_hermitian(nrows, ur, uc, planes_csr[l]);
  op->hermitian_planes = hermitian;
  trace.mark("Hermitian check");
  int fmt = QP_FMT_DENSE;
  if (!dense) QP_CHECK(pick_format(op.get(), format, hermitian, &fmt));
  trace.mark("format choice");
  if (!ur_orig.empty() && fmt != QP_FMT_HRB) {   // (a lattice completion happened;) not Hermitian, or not packed: the zeros would buy nothing
    take_completion_back(op.get(), terms, canonical, ur_orig, uc_orig, planes_csr);
    QP_CHECK(pick_format(op.get(), format, hermitian, &fmt));
  }
  QP_CHECK(operator_build_device(op.get(), fmt, planes_csr));
  trace.mark("device build (layout, encodings, uploads, plans)");
  if (!ur_orig.empty() && !op->walk.valid) {     // packed, completed, and still no plan: build once more without the zeros
    QP_CHECK(operator_free_device(op.get()));
    take_completion_back(op.get(), terms, canonical, ur_orig, uc_orig, planes_csr);
    QP_CHECK(pick_format(op.get(), format, hermitian, &fmt));
    QP_CHECK(operator_build_device(op.get(), fmt, planes_csr));
  }
  planes_csr.clear();
  // the whole host side of the creation (union pattern, lattice completion, value planes, Hermitian check, format choice)
  // belongs to what qp_operator_build_info reports for the first build
  op->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create).count();
  op->build_ms_total = op->build_ms;
  qp_operator* raw = op.release();
  std::vector<qp_c128> ones(ncoeffs, qp_c128{1.0, 0.0});
  int rc = qp_operator_set_coeffs(raw, ones.data(), ncoeffs);
  if (rc != QP_OK) {
    operator_free(raw);
    return rc;
  }
  *out = raw;
  return QP_OK;
  QP_CATCH
}


// evaluate!: the current values from the planes and the coefficients
static int operator_refresh(qp_operator* op) {
  qp_ctx* ctx = op->ctx;
  op->vals_epoch++;
  if (op->A.format == QP_FMT_MATFREE) return op->mf_refresh(op);
  const int drift = op->nops - op->ncoeffs;  // src/generators.jl:635
  std::vector<double2> eff(op->nops);
  bool all_one = true, all_real = true;
  for (int l = 0; l < op->nops; ++l) {
    cplx c = op->scale;
    if (l >= drift) c *= op->coeffs[l - drift];
    eff[l] = d2(c);
    if (!(c == cplx(1.0))) all_one = false;
    if (c.imag() != 0.0) all_real = false;
  }
  if (op->A.format == QP_FMT_HRB && !all_real) {
    // a complex combination of Hermitian terms is not Hermitian: leave the packed format
    // (slow path, once): re-lay the planes out as full row-block CSR
    Planes planes_csr;
    QP_CHECK(operator_download_planes(op, planes_csr));
    operator_free_device(op);
    const int fmt = choose_format(op, QP_FMT_AUTO, false);
    QP_CHECK(operator_build_device(op, fmt, planes_csr));
    op->n_relayouts++;
  }
  // real terms with real coefficients: the mat-vec kernels stream a real copy (8 instead of 16
  // bytes per value); everything else keeps reading the complex array
  const bool want_real = op->ctx->tun.real_vals && op->planes_real && all_real && op->A.stored > 0;
  if (want_real && !op->real_vals) QP_CHECK(dev_alloc(&op->real_vals, (size_t)op->A.stored));
  if (op->sparse_from > 0 && ctx->tun.sparse_controls && !(op->nops == 1 && all_one)) {
    // only the sparse trailing control terms' positions are rewritten (qp_operator::sparse_from)
    const int sf = op->sparse_from;
    bool same = op->base_valid && op->base_real == want_real && (int)op->base_eff.size() == sf;
    for (int l = 0; same && l < sf; ++l) same = (eff[l].x == op->base_eff[(size_t)l].x && eff[l].y == op->base_eff[(size_t)l].y);
    if (!same) {
      if (!op->base) QP_CHECK(dev_alloc(&op->base, (size_t)op->A.stored));
      if (!op->combined) QP_CHECK(dev_alloc(&op->combined, (size_t)op->A.stored));
      QP_CHECK(qp::launch_combine_planes(ctx->stream, op->base, op->planes_dev, eff.data(), sf, op->A.stored, nullptr, &ctx->stats));
      QP_HIP(hipMemcpyAsync(op->combined, op->base, (size_t)op->A.stored * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
      op->base_eff.assign(eff.begin(), eff.begin() + sf);
      op->base_valid = true;
      op->base_real = want_real;
    }
    QP_CHECK(qp::launch_sparse_planes_update(ctx->stream, op->combined, op->base, op->support, op->n_support, op->support_vals,
                                             op->nops - sf, eff.data() + sf, (same && want_real) ? op->real_vals : nullptr,
                                             &ctx->stats));
    if (!same && want_real) QP_CHECK(qp::launch_real_part(ctx->stream, op->real_vals, op->combined, op->A.stored, &ctx->stats));
    op->A.vals = op->combined;
    op->real_of = nullptr;
    op->last_refresh_sparse = true;
  } else if (op->nops == 1 && all_one) {
    op->last_refresh_sparse = false;
    op->base_valid = false;   // (`combined` is not what the sparse update left: the next sparse update rebuilds its base)
    op->A.vals = op->planes[0];
    if (want_real && op->real_of != op->A.vals) {   // a plane never changes: extract once
      QP_CHECK(qp::launch_real_part(ctx->stream, op->real_vals, op->A.vals, op->A.stored, &ctx->stats));
      op->real_of = op->A.vals;
    }
  } else {
    // the full combination rewrites `combined` with THESE coefficients everywhere: whatever the sparse update's base was
    // built for no longer describes it (knob sparse_controls switched off and on again on a live operator)
    op->base_valid = false;
    op->last_refresh_sparse = false;
    if (!op->combined) QP_CHECK(dev_alloc(&op->combined, (size_t)op->A.stored));
    QP_CHECK(qp::launch_combine_planes(ctx->stream, op->combined, op->planes_dev, eff.data(), op->nops, op->A.stored,
                                       want_real ? op->real_vals : nullptr, &ctx->stats));
    op->A.vals = op->combined;
    op->real_of = nullptr;
  }
  op->A.vals_r = want_real ? op->real_vals : nullptr;
  if (op->cv.valid) {   // the value-dictionary mirror: the same combination on the table entries instead of the stored positions
    qp::CodedVals& C = op->cv;
    if (want_real && !C.tab_r) QP_CHECK(dev_alloc(&C.tab_r, (size_t)C.ntab));
    if (op->nops == 1 && all_one) {
      C.tab = op->cv_tplanes[0];
      if (want_real) QP_CHECK(qp::launch_real_part(ctx->stream, C.tab_r, C.tab, C.ntab, &ctx->stats));
    } else {
      if (!op->cv_tab_comb) QP_CHECK(dev_alloc(&op->cv_tab_comb, (size_t)C.ntab));
      QP_CHECK(qp::launch_combine_planes(ctx->stream, op->cv_tab_comb, op->cv_tplanes_dev, eff.data(), op->nops, C.ntab,
                                         want_real ? C.tab_r : nullptr, &ctx->stats));
      C.tab = op->cv_tab_comb;
    }
    C.use_real = want_real ? 1 : 0;
  }
  if (op->cb.valid) {   // the column-blocked mirror follows the values (one gather pass per evaluate!)
    if (want_real && !op->cb.vals_r) QP_CHECK(dev_alloc(&op->cb.vals_r, (size_t)op->cb.nnz));
    op->cb.use_real = want_real ? 1 : 0;
    QP_CHECK(qp::launch_colblock_gather(ctx->stream, op->cb, op->A.vals, &ctx->stats));
  }
  return QP_OK;
}

int qp_operator_set_coeffs(qp_operator* op, const qp_c128* coeffs, int ncoeffs) {
  QP_TRY
  if (!op || (ncoeffs > 0 && !coeffs)) return qp::fail(QP_E_BAD_ARG, "qp_operator_set_coeffs: NULL argument");
  if (ncoeffs != op->ncoeffs) return qp::fail(QP_E_BAD_ARG, "expected %d coefficients, got %d", op->ncoeffs, ncoeffs);
  QP_CHECK(use(op->ctx));
  for (int i = 0; i < ncoeffs; ++i) op->coeffs[i] = cx(coeffs[i]);
  return operator_refresh(op);
  QP_CATCH
}

int qp_operator_set_scale(qp_operator* op, qp_c128 scale) {
  QP_TRY
  if (!op) return qp::fail(QP_E_BAD_ARG, "operator is NULL");
  QP_CHECK(use(op->ctx));
  op->scale = cx(scale);
  return operator_refresh(op);
  QP_CATCH
}

int qp_operator_destroy(qp_operator* op) {
  QP_TRY
  return operator_free(op);
  QP_CATCH
}

int qp_operator_info(const qp_operator* op, int64_t* nrows, int64_t* ncols, int64_t* nnz, int* format) {
  if (!op) return qp::fail(QP_E_BAD_ARG, "operator is NULL");
  if (nrows) *nrows = op->A.nrows;
  if (ncols) *ncols = op->A.ncols;
  if (nnz) *nnz = op->A.nnz;
  if (format) *format = op->A.format;
  return QP_OK;
}

int qp_operator_layout_info(const qp_operator* op, int64_t out[5]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_layout_info: NULL argument");
  for (int i = 0; i < 5; ++i) out[i] = 0;
  const DevMatrix& A = op->A;
  out[4] = A.stored;
  if (qp::csr_layout(A.format) || A.format == QP_FMT_MATFREE) return QP_OK;
  const HostLayout& Lh = op->layout;
  out[0] = A.nblocks;
  int64_t idx_bytes = A.colbytes + A.lcolbytes;
  for (int64_t b = 0; b < A.nblocks; ++b) {
    if ((Lh.cmeta[b] & 3) == qp::kColStencil) out[1]++;
    if (A.format == QP_FMT_HRB) {
      if ((Lh.lcmeta[b] & 3) == qp::kColStencil) out[2]++;
      else idx_bytes += (Lh.lptr[b + 1] - Lh.lptr[b]) * (int64_t)sizeof(int32_t);
    }
  }
  out[3] = idx_bytes;
  return QP_OK;
}

/* how the column sections of the row blocks are encoded: out[0..3] = upper (or only) sections as int32 columns / int16 distances
   / stencil (one distance per slot) / block map (one column block per slot + a byte per entry); out[4..7] = the same for the lower
   sections of a Hermitian-packed operator */
int qp_operator_encoding_info(const qp_operator* op, int64_t out[8]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_encoding_info: NULL argument");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  const DevMatrix& A = op->A;
  if (qp::csr_layout(A.format) || A.format == QP_FMT_MATFREE) return QP_OK;
  const HostLayout& Lh = op->layout;
  for (int64_t b = 0; b < A.nblocks; ++b) {
    out[(int)(Lh.cmeta[b] & 3)]++;
    if (A.format == QP_FMT_HRB) out[4 + (int)(Lh.lcmeta[b] & 3)]++;
  }
  return QP_OK;
}

/* the value-dictionary mirror (device.h: CodedVals): out[0] = 1 when the mat-vec reads it, out[1] = table entries, out[2] = distinct
   tables, out[3] = bytes a term streams for the values through it (codes + tables), out[4] = bytes of the value plane it replaces,
   out[5] = why there is none (0: there is one, 1: not a plain row-block operator, 2: a block with more than 256 distinct values,
   3: no saving, 4: knob value_dict off, 5: column-blocked mirror in use) */
int qp_operator_value_encoding_info(const qp_operator* op, int64_t out[6]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_value_encoding_info: NULL argument");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  const qp::CodedVals& C = op->cv;
  const bool on = C.valid && op->ctx->tun.value_dict != 0;
  out[0] = on ? 1 : 0;
  out[1] = C.ntab;
  out[2] = C.ntables;
  out[3] = C.valid ? op->A.stored + (C.use_real ? 8 : 16) * C.ntab : 0;
  out[4] = (op->A.vals_r ? 8 : 16) * op->A.stored;
  out[5] = on ? 0 : (C.valid ? 4 : (op->cb.valid ? 5 : (op->cv_reason ? op->cv_reason : 1)));
  return QP_OK;
}

int qp_operator_build_info(const qp_operator* op, double out[4]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_build_info: NULL argument");
  out[0] = op->build_ms;
  out[1] = op->build_ms_total;
  out[2] = (double)op->n_relayouts;
  out[3] = (double)op->A.format;
  return QP_OK;
}

int qp_lattice_fill_host(int64_t nrows, int64_t ncols, const int64_t* rowptr, const int32_t* col, int min_blocks,
                         int64_t* rowptr_out, int32_t* col_out, int64_t cap, int64_t* nnz_out) {
  QP_TRY
  if (!rowptr || !col || !rowptr_out || !col_out || !nnz_out || nrows < 0 || ncols < 0 || rowptr[0] != 0)
    return qp::fail(QP_E_BAD_ARG, "qp_lattice_fill_host: bad arguments");
  qp::HostVec<int64_t> ur(rowptr, rowptr + nrows + 1);
  qp::HostVec<int32_t> uc(col, col + rowptr[nrows]);
  PlanKnobs knobs;
  knobs.lattice_fill = 1;
  knobs.walk_min_blocks = min_blocks;
  lattice_fill(knobs, nrows, ncols, ur, uc);
  *nnz_out = ur[nrows];
  if (ur[nrows] > cap) return qp::fail(QP_E_BAD_ARG, "qp_lattice_fill_host: col_out holds %lld entries, %lld needed", (long long)cap, (long long)ur[nrows]);
  std::memcpy(rowptr_out, ur.data(), ur.size() * sizeof(int64_t));
  std::memcpy(col_out, uc.data(), uc.size() * sizeof(int32_t));
  return QP_OK;
  QP_CATCH
}

int qp_operator_fill_info(const qp_operator* op, int64_t* n_filled) {
  if (!op || !n_filled) return qp::fail(QP_E_BAD_ARG, "qp_operator_fill_info: NULL argument");
  *n_filled = op->n_lattice_fill;
  return QP_OK;
}

int qp_operator_walk_info(const qp_operator* op, int64_t out[8]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_walk_info: NULL argument");
  const qp::WalkPlan& P = op->walk;
  const qp::Tuning& tun = op->ctx->tun;
  // "has one" = the fused term of a whole-operator cheby! takes the walk under the context's current knobs
  const bool on = P.valid && op->A.walk == &op->walk && tun.hrb_walk && (tun.rbcsr_variant & 31) == 15 &&
                  P.R1 - P.W0 >= tun.walk_min_blocks;
  out[0] = on ? 1 : 0;
  out[1] = on ? P.nn : 0;
  out[2] = on ? P.K : 0;
  out[3] = on ? P.z0 : 0;
  out[4] = on ? P.g : 0;
  out[5] = on ? P.W0 : 0;
  out[6] = on ? P.R1 : 0;
  out[7] = on ? P.n_edge : 0;
  return QP_OK;
}

int qp_operator_evaluate_info(const qp_operator* op, int64_t out[3]) {
  QP_TRY
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_evaluate_info: NULL argument");
  out[0] = op->sparse_from;
  out[1] = op->sparse_from > 0 ? op->n_support : 0;
  out[2] = op->last_refresh_sparse ? 1 : 0;
  return QP_OK;
  QP_CATCH
}

int qp_operator_walk_reason(const qp_operator* op, int* code, char* text, size_t text_len) {
  QP_TRY
  if (!op || !code) return qp::fail(QP_E_BAD_ARG, "qp_operator_walk_reason: NULL argument");
  int c = QP_WALK_OK;
  std::string why;
  const qp::WalkPlan& P = op->walk;
  const qp::Tuning& tun = op->ctx->tun;
  if (op->A.format != QP_FMT_HRB) {
    if (op->A.format == QP_FMT_MATFREE || op->A.format == QP_FMT_DENSE) {
      c = QP_WALK_NOT_PACKED;
      why = "a dense / matrix-free operator has no sparse lattice to walk";
    } else if (!op->hermitian_planes) {
      c = QP_WALK_NOT_HERMITIAN;
      why = "a term of the operator is not exactly Hermitian (or a format other than AUTO / HRB was requested): no Hermitian-packed layout";
    } else if (op->n_relayouts > 0) {
      c = QP_WALK_COMPLEX_COEFF;
      why = "a complex coefficient took the Hermitian-packed operator back to plain row blocks (qp_operator_build_info: re-layouts)";
    } else {
      c = QP_WALK_NOT_PACKED;
      why = "Hermitian, but not laid out Hermitian-packed (transposed entries too far apart for the L2, irregular row blocks, or padding)";
    }
  } else if (!P.valid) {
    c = op->walk_reason != QP_WALK_OK ? op->walk_reason : (int)QP_WALK_NO_UNIFORM_RUN;
    why = op->walk_reason_text;
  } else if (!tun.hrb_walk) {
    c = QP_WALK_DISABLED;
    why = "knob hrb_walk is 0";
  } else if (P.R1 - P.W0 < tun.walk_min_blocks || P.R1 - P.W0 < P.S) {
    c = QP_WALK_TOO_FEW_BLOCKS;
    char buf[160];
    std::snprintf(buf, sizeof buf, "%lld walkable row blocks, knob walk_min_blocks is %d: the per-block kernel runs (as fast at this size)",
                  (long long)(P.R1 - P.W0), tun.walk_min_blocks);
    why = buf;
  }
  *code = c;
  if (text && text_len > 0) {
    std::strncpy(text, why.c_str(), text_len - 1);
    text[text_len - 1] = '\0';
  }
  return QP_OK;
  QP_CATCH
}

/* column-blocked mirror (device.h: ColBlockPlan): out = {1 if the operator has one, column blocks, log2 of the columns per
   block, rows per tile, entries of the longest segment, tiles}; *line_share (nullable) = the sampled share of gathers that
   pull a 128-byte line of their own -- what the decision was taken on (0 when it never came to sampling) */
int qp_operator_colblock_info(const qp_operator* op, int64_t out[6], double* line_share) {
  QP_TRY
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_colblock_info: NULL argument");
  out[0] = op->cb.valid;
  out[1] = op->cb.P;
  out[2] = op->cb.log2w;
  out[3] = 64 * op->cb.rpt;
  out[4] = op->cb.max_seg;
  out[5] = op->cb.ntiles;
  if (line_share) *line_share = op->cb_line_share;
  return QP_OK;
  QP_CATCH
}

int qp_operator_walk_long(const qp_operator* op, int64_t* glong) {
  if (!op || !glong) return qp::fail(QP_E_BAD_ARG, "qp_operator_walk_long: NULL argument");
  *glong = (op->walk.valid && op->A.walk == &op->walk && op->walk.xl) ? op->walk.glong : 0;
  return QP_OK;
}

/* the whole stencil shape of the walk plan: {near distances, far reach K, diagonal entry, long pairs, diagonal far neighbours
   (1: the far distances of step m are m g - 1, m g, m g + 1), strip step g, shorter long distance, longest distance}; zeros
   without a plan */
int qp_operator_walk_shape(const qp_operator* op, int64_t out[8]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_walk_shape: NULL argument");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (!(op->walk.valid && op->A.walk == &op->walk)) return QP_OK;
  const qp::WalkPlan& P = op->walk;
  out[0] = P.nn;
  out[1] = P.K;
  out[2] = P.z0;
  out[3] = P.xl;
  out[4] = P.fd;
  out[5] = P.g;
  out[6] = P.xl == 2 ? P.glong1 : 0;
  out[7] = P.xl ? P.glong : 0;
  return QP_OK;
}

int qp_operator_walk_long_pairs(const qp_operator* op, int64_t out[2]) {
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_walk_long_pairs: NULL argument");
  const bool on = op->walk.valid && op->A.walk == &op->walk;
  out[0] = (on && op->walk.xl == 2) ? op->walk.glong1 : (on && op->walk.xl == 1) ? op->walk.glong : 0;
  out[1] = (on && op->walk.xl == 2) ? op->walk.glong : 0;
  return QP_OK;
}

int qp_operator_spmm_tiles(qp_operator* op, int batch, int64_t out[6]) {
  QP_TRY
  if (!op || !out || batch < 1) return qp::fail(QP_E_BAD_ARG, "qp_operator_spmm_tiles: bad arguments");
  if (op->A.format == QP_FMT_MATFREE) return qp::fail(QP_E_BAD_ARG, "a matrix-free operator has no stored entries");
  QP_CHECK(use(op->ctx));
  for (int k = 0; k < 6; ++k) out[k] = 0;
  if (qp::spmm_uses_rows_kernel(op->ctx->tun, batch) && op->ctx->tun.spmm_rw < 0) {
    const qp::SpmmTiles* P = nullptr;
    QP_CHECK(operator_spmm_tiles(op, &P));
    if (P) {
      out[0] = 1;
      out[1] = P->ntiles;
      out[2] = P->nrest;
      out[3] = P->g;
      out[4] = P->shape.K;
      out[5] = P->shape.NN;
    }
  }
  return QP_OK;
  QP_CATCH
}

int qp_operator_spmm_walk(qp_operator* op, int batch, int64_t out[2]) {
  QP_TRY
  if (!op || !out || batch < 1) return qp::fail(QP_E_BAD_ARG, "qp_operator_spmm_walk: bad arguments");
  if (op->A.format == QP_FMT_MATFREE) return qp::fail(QP_E_BAD_ARG, "a matrix-free operator has no stored entries");
  QP_CHECK(use(op->ctx));
  out[0] = out[1] = 0;
  if (qp::spmm_uses_rows_kernel(op->ctx->tun, batch)) {
    const int32_t* order = nullptr;
    QP_CHECK(operator_spmm_order(op, batch, &order));
    out[0] = order ? op->m_order_g : 0;
    out[1] = order ? op->m_order_sw : 0;
  }
  return QP_OK;
  QP_CATCH
}

// download the *device* copy (current combined values and indices) back as canonical CSR
int qp_operator_get_csr(qp_operator* op, int64_t* rowptr, int32_t* col, qp_c128* vals) {
  QP_TRY
  if (!op || !rowptr || !col || !vals) return qp::fail(QP_E_BAD_ARG, "qp_operator_get_csr: NULL argument");
  if (op->A.format == QP_FMT_MATFREE) return qp::fail(QP_E_BAD_ARG, "a matrix-free operator has no stored entries");
  QP_CHECK(use(op->ctx));
  const DevMatrix& A = op->A;
  const auto& ur = op->u_rowptr;
  QP_HIP(hipStreamSynchronize(op->ctx->stream));
  std::vector<cplx> hv((size_t)std::max<int64_t>(A.stored, 1));
  QP_HIP(hipMemcpy(hv.data(), A.vals, (size_t)A.stored * sizeof(double2), hipMemcpyDeviceToHost));
  if (op->cv.valid && op->ctx->tun.value_dict != 0) {
    // the values the mat-vec really reads: table[tptr[block] + code], decoded back into the plane's positions (the
    // reconstruction is exact: tests compare it with what was passed in)
    const qp::CodedVals& C = op->cv;
    std::vector<uint8_t> codes((size_t)A.stored);
    std::vector<int64_t> tptr((size_t)A.nblocks);
    std::vector<cplx> tab((size_t)C.ntab);
    QP_HIP(hipMemcpy(codes.data(), C.codes, codes.size(), hipMemcpyDeviceToHost));
    QP_HIP(hipMemcpy(tptr.data(), C.tptr, tptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    QP_HIP(hipMemcpy(tab.data(), C.tab, tab.size() * sizeof(double2), hipMemcpyDeviceToHost));
    decode_value_dict(op->layout, A.nblocks, codes, tptr, tab, hv);
  }
  if (qp::csr_layout(A.format)) {
    std::vector<int64_t> rp(A.nrows + 1);
    std::vector<int32_t> hc((size_t)std::max<int64_t>(A.nnz, 1));
    QP_HIP(hipMemcpy(rp.data(), A.rowptr, rp.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    QP_HIP(hipMemcpy(hc.data(), A.cols, (size_t)A.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::memcpy(rowptr, rp.data(), rp.size() * sizeof(int64_t));
    std::memcpy(col, hc.data(), (size_t)A.nnz * sizeof(int32_t));
    std::memcpy(vals, hv.data(), (size_t)A.nnz * sizeof(qp_c128));
    return QP_OK;
  }
  std::vector<int64_t> bptr(A.nblocks + 1), cmeta((size_t)A.nblocks), lptr, lcmeta;
  std::vector<char> cbytes((size_t)std::max<int64_t>(A.colbytes, 1)), lbytes;
  QP_HIP(hipMemcpy(bptr.data(), A.bptr, bptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  QP_HIP(hipMemcpy(cmeta.data(), A.cmeta, cmeta.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  QP_HIP(hipMemcpy(cbytes.data(), A.cols, (size_t)A.colbytes, hipMemcpyDeviceToHost));
  std::vector<int32_t> lp;
  if (A.format == QP_FMT_HRB) {
    lptr.resize(A.nblocks + 1);
    lcmeta.resize((size_t)A.nblocks);
    lbytes.resize((size_t)std::max<int64_t>(A.lcolbytes, 1));
    lp.resize((size_t)std::max<int64_t>(A.lstored, 1));
    QP_HIP(hipMemcpy(lptr.data(), A.lptr, lptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    QP_HIP(hipMemcpy(lcmeta.data(), A.lcmeta, lcmeta.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (A.lcolbytes > 0) QP_HIP(hipMemcpy(lbytes.data(), A.lcols, (size_t)A.lcolbytes, hipMemcpyDeviceToHost));
    QP_HIP(hipMemcpy(lp.data(), A.lpos, lp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  for (int64_t r = 0; r <= A.nrows; ++r) rowptr[r] = ur[r];
  for (int64_t r = 0; r < A.nrows; ++r) {
    const int64_t nl = (A.format == QP_FMT_HRB) ? op->layout.nlow[r] : 0;
    for (int64_t k = 0; k < ur[r + 1] - ur[r]; ++k) {
      cplx v;
      int64_t c;
      if (k >= nl) {
        c = decode_col(cbytes, cmeta, A.nrows, r, k - nl);
        v = hv[rb_val_pos(bptr, r, k - nl)];
      } else {
        c = decode_col(lbytes, lcmeta, A.nrows, r, k, true);
        const bool stencil = (lcmeta[r / kRB] & 3) == qp::kColStencil;
        v = std::conj(hv[stencil ? decode_lower_stencil_pos(lbytes, lcmeta, A.nrows, r, k) : lp[rb_quad_pos(lptr, r, k)]]);
      }
      col[ur[r] + k] = (int32_t)c;
      vals[ur[r] + k] = qp_c128{v.real(), v.imag()};
    }
  }
  return QP_OK;
  QP_CATCH
}

}  // extern "C"

// CSR-ordered mirror of the operator for the batched (SpMM) path and the persistent
// small-system kernels, built lazily
int operator_csr_mirror(qp_operator* op, bool gather) {
  if (op->A.format == QP_FMT_MATFREE) return qp::fail(QP_E_BAD_ARG, "a matrix-free operator has no stored entries");
  qp_ctx* ctx = op->ctx;
  const DevMatrix& A = op->A;
  const auto& ur = op->u_rowptr;
  const auto& uc = op->u_col;
  const int64_t nnz = A.nnz;
  if (!op->m_rowptr) {
    std::vector<int64_t> map;
    csr_value_map(op->layout, A.nrows, ur, uc, map);
    QP_CHECK(dev_upload(&op->m_rowptr, ur.data(), ur.size()));
    QP_CHECK(dev_upload(&op->m_cols, uc.data(), (size_t)nnz));
    QP_CHECK(dev_upload(&op->m_map, map.data(), (size_t)nnz));
    QP_CHECK(dev_alloc(&op->m_vals, (size_t)nnz));
    op->m_epoch = 0;
  }
  if (gather && op->m_epoch != op->vals_epoch) {
    QP_CHECK(qp::launch_gather_csr_vals(ctx->stream, op->m_vals, A.vals, op->m_map, nnz, &ctx->stats));
    op->m_epoch = op->vals_epoch;
  }
  return QP_OK;
}
