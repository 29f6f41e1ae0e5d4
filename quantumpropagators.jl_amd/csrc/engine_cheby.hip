// cheby!: one step, batched states, one fused term (plain and boundary/interior split),
// and the propagate step loop.
#include "engine.h"

int split_timed_out(const qp_split* sp) {
  if (sp && sp->timeout_host && __atomic_load_n(sp->timeout_host, __ATOMIC_RELAXED) != 0)
    return qp::fail(QP_E_INTERNAL, "an interior launch of an earlier term timed out waiting for its boundary launch: "
                                   "the state of this partitioned cheby! is not valid");
  return QP_OK;
}

void set_defer(qp::ChebyEpi& e, const qp_acc_defer* d) {
  if (!d) return;
  e.acc_skip = d->skip ? 1 : 0;
  e.n_defer = d->skip ? 0 : d->n_defer;
  e.a_d1 = d->a_d1;
  e.a_d2 = d->a_d2;
}

// the epilogue of one fused term from its operands and scalars; a term that skips the accumulator (defer->skip) carries none
static qp::ChebyEpi cheby_epi(const double2* xloc, const double2* v0, double2* vout, const double2* acc_in, double2* acc_out,
                              double2 c, double beta, double a_prev, double a, double2 phase, int apply_phase,
                              const qp_acc_defer* defer) {
  const bool skip = defer && defer->skip;
  qp::ChebyEpi e;
  e.xloc = xloc;
  e.v0 = v0;
  e.vout = vout;
  e.acc_in = skip ? nullptr : acc_in;
  e.acc_out = skip ? nullptr : acc_out;
  e.c = c;
  e.beta = beta;
  e.a_prev = a_prev;
  e.a = a;
  e.phase = phase;
  e.apply_phase = apply_phase;
  e.check_partials = nullptr;
  set_defer(e, defer);
  return e;
}

// the term arguments of the C ABI (qp_cheby_term, qp_cheby_term_split; `who`: the entry point's name): checked, then as an epilogue
static int cheby_term_args(const char* who, const qp_operator* op, const qp_state* x, int64_t xoff, const qp_state* v0,
                           qp_state* vout, const qp_state* acc_in, qp_state* acc_out, qp_c128 c, double beta, double a_prev,
                           double a, qp_c128 phase, const qp_acc_defer* defer, qp::ChebyEpi* e) {
  if (defer && !defer->skip && (defer->n_defer < 0 || defer->n_defer > 2 || (defer->n_defer > 0 && !v0 && (defer->n_defer == 2 || !acc_in))))
    return qp::fail(QP_E_BAD_ARG, "%s: deferred accumulation needs v0", who);
  const int64_t nr = op->A.nrows;
  if (x->n != op->A.ncols || xoff < 0 || xoff + nr > x->n) return qp::fail(QP_E_BAD_ARG, "%s: x shape / offset mismatch", who);
  if ((v0 && v0->n != nr) || (vout && vout->n != nr) || (acc_in && acc_in->n != nr) || (acc_out && acc_out->n != nr))
    return qp::fail(QP_E_BAD_ARG, "%s: local vector length mismatch", who);
  *e = cheby_epi(x->d + xoff, v0 ? v0->d : nullptr, vout ? vout->d : nullptr, acc_in ? acc_in->d : nullptr,
                 acc_out ? acc_out->d : nullptr, d2(c), beta, a_prev, a, d2(phase), !(phase.re == 1.0 && phase.im == 0.0), defer);
  return QP_OK;
}

// Does a whole-operator cheby! of `op` take the two-term strip walk (kernels_walk2.hip) under the context's knobs?  The rule:
// walk_geometry.cpp, for an operator whose whole-operator term is the one-term walk of its own plan.
// Which of the two rules fired names the cut of the pair launches (walk_geometry.h: Walk2Rule).
static qp::Walk2Rule walk2_rule(const qp_operator* op) {
  const qp::Tuning& tun = op->ctx->tun;
  if (!(tun.hrb_walk && (tun.rbcsr_variant & 31) == 15 && op->A.walk == &op->walk)) return qp::kWalk2None;
  return qp::walk2_rule(op->walk, op->walk2, qp::walk_matrix(op->A), qp::walk_knobs(tun), qp::device_cu_count());
}
static bool walk2_wanted(const qp_operator* op) { return walk2_rule(op) != qp::kWalk2None; }

// the launches of one cheby! call (src/cheby.jl:171-211): n_coeffs - 1 fused mat-vec + term kernels in the order and with the
// vectors ChebySequence (cheby_plan.h) names, and, when the result does not land in Psi's buffer, one copy.
// `launch_term(x, e)` issues one term: the single-state step's mat-vec kernel, or the panel kernels of the batched step (`panel`:
// element = (row, state); never in pairs, no check_normalization).
template <class LaunchTerm>
static int cheby_step_launches(qp_cheby* w, qp_operator* op, qp_state* psi, const double* a, int n_coeffs, const ChebyScalars& sc,
                               bool check_normalization, bool panel, LaunchTerm&& launch_term) {
  qp_ctx* ctx = op->ctx;
  const DevMatrix& A = op->A;
  double2* const buf[kChebySlots] = {nullptr, psi->d, w->bufA, w->bufC, w->bufD, w->acc};   // (ChebySlot)
  auto epi = [&](const ChebyTerm& t) {
    return cheby_epi(buf[(int)t.x], buf[(int)t.v0], buf[(int)t.vout], buf[(int)t.acc_in], buf[(int)t.acc_out], d2(sc.c * t.c_scale),
                     sc.beta, t.a_prev, t.a, d2(sc.phase), t.apply_phase, t.defer);
  };
  // (qp_cheby_step allocated the two vectors of a step in pairs)
  const qp::Walk2Rule pair_rule = walk2_rule(op);
  const bool pairs = ChebySequence::pairs_possible(n_coeffs, check_normalization, panel) && w->bufC && w->bufD && pair_rule != qp::kWalk2None;
  ChebySequence seq(a, n_coeffs, ctx->tun.acc_defer != 0, pairs, check_normalization, panel);
  ChebyLaunch L;
  while (seq.next(&L)) {
    if (L.pair) {
      // terms m and m + 1 in one pass over the values: y = v_m, z = v_{m+1}
      const qp::ChebyEpi e1 = epi(L.t[0]), e2 = epi(L.t[1]);
      bool launched = false;
      const qp::ScopedRange mv_range(ctx->tun.roctx != 0 || qp::ranges_enabled_by_env(), "matrix-vector product");
      QP_CHECK(qp::launch_hrb_walk2_cheby(ctx->stream, A, op->walk2, e1.xloc, e1, e2, ctx->tun, pair_rule, &launched));
      if (!launched) {   // not taken after all (the kernel's LDS opt-in was refused): this and every later term as one-term launches
        seq.refuse();
        continue;
      }
      // term m + 1 of the blocks outside the two-term region: they read y of their neighbours, which the launch above wrote
      if (ctx->tun.walk_dbg & qp::kWalkDbgPairFollowUpPerBlock) {      // (A/B: the per-block kernel over the edge list as a row set)
        qp::RowSet rs;
        rs.block_map = op->walk2.edge_map;
        rs.nmap = op->walk2.n_edge;
        rs.count = false;
        QP_CHECK(qp::launch_spmv_cheby(ctx->stream, A, e2.xloc, e2, &ctx->stats, &rs));
      } else {
        QP_CHECK(qp::launch_hrb_walk2_edge_cheby(ctx->stream, A, op->walk2, e2.xloc, e2));
        ctx->stats.n_launch++;
      }
      ctx->stats.n_launch++;
      ctx->stats.n_pair_launch++;
      ctx->stats.n_matvec += 2;
      ctx->stats.spmv_bytes += 2.0 * (20.0 * (double)A.nnz + 4.0 * (double)(A.nrows + 1) + 80.0 * (double)A.nrows);
      continue;
    }
    qp::ChebyEpi e = epi(L.t[0]);
    e.check_partials = L.t[0].check ? w->chk_part : nullptr;
    QP_CHECK(launch_term(e.xloc, e));
    if (e.check_partials)
      QP_CHECK(qp::launch_reduce_triples(ctx->stream, w->chk_part, qp::spmv_grid_size(A), w->chk_out + 3 * (L.m - 1), &ctx->stats));
  }
  if (seq.result() != ChebySlot::Psi)
    QP_HIP(hipMemcpyAsync(psi->d, buf[(int)seq.result()], (size_t)psi->n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
  return QP_OK;
}

// does the persistent small-system kernel take a Chebychev time grid of this operator, and with which plan?  (Also behind
// qp_operator_small_plan; the gate on plain numbers: cheby_plan.h.)
bool cheby_small_fits(const qp_operator* op, qp::SmallPlan* plan) {
  const int small_nnz = op->ctx->tun.small_nnz;
  return cheby_small_candidate(op->A.nnz, op->nops, small_nnz) &&
         cheby_small_gate(op->A.nnz, op->nops, op->A.nrows, operator_longest_row(op), small_nnz, plan);
}

// the argument checks every cheby! entry point shares, in the reference's words (`dt` nullable: no time step to compare)
static int cheby_step_args(const double* dt, double wrk_dt, int n_coeffs, double Delta) {
  if (dt && !cheby_dt_matches(*dt, wrk_dt)) return qp::fail(QP_E_DT_MISMATCH, "wrk was initialized for dt=%g, not dt=abs(%g)", wrk_dt, *dt);
  if (n_coeffs < 2) return qp::fail(QP_E_TOO_FEW_COEFFS, "Need at least 2 Chebychev coefficients");
  if (!(Delta > 0)) return qp::fail(QP_E_BAD_ARG, "Delta must be positive");
  return QP_OK;
}

// Launch-bound systems (a term takes less than its launch): the step of `launch` as a hipGraph, replayed while the key --
// everything a launch argument is derived from -- stays the same; the second identical call in a row records it.  *done = false:
// nothing was issued (the caller launches the step itself).  Never for a matrix-free operator: the key knows an operator by its
// stored arrays (all NULL there), and the owner's launch picks its kernel on the host from the CURRENT coefficients
// (engine_pauli.hip: real-only paths, diagonal vector real or complex) -- a captured step would replay another operator's, or an
// earlier coefficient set's, launches
template <class Launch>
static int cheby_step_graph(qp_cheby* w, qp_operator* op, qp_state* psi, const double* a, int n_coeffs, double Delta, double E_min,
                            double dt, Launch&& launch, bool* done) {
  qp_ctx* ctx = op->ctx;
  const DevMatrix& A = op->A;
  *done = false;
  if (!ctx->tun.cheby_graph || A.format == QP_FMT_MATFREE || ctx->stream == nullptr || ctx->stream == hipStreamLegacy) return QP_OK;
  qp_cheby::GraphKey key;
  key.vals = A.vals_r ? (const void*)A.vals_r : (const void*)A.vals;
  key.cols = A.cols;
  key.rowptr = qp::csr_layout(A.format) ? (const void*)A.rowptr : (const void*)A.bptr;
  key.psi = psi->d;
  key.format = A.format;
  // every knob that selects a kernel or a launch shape of the step's terms
  key.variant = ((((ctx->tun.rbcsr_variant * 2) * 16 + 8) * 2 + (ctx->tun.hrb_walk ? 1 : 0)) * 8 +
                 (ctx->tun.walk_nt & 7)) * 4096 + (ctx->tun.walk_waves & 4095);
  key.variant = key.variant * 2 + (ctx->tun.value_dict ? 1 : 0);      // (coded / plain row-block kernel)
  key.variant = key.variant * 2 + (walk2_wanted(op) ? 1 : 0);         // (terms in pairs)
  key.pair = (int)walk2_rule(op) * 128 + (ctx->tun.walk_dbg & 127);   // (... with which cut, follow-up kernel and edge steps)
  key.n_coeffs = n_coeffs;
  key.dt = dt;
  key.Delta = Delta;
  key.E_min = E_min;
  uint64_t h = 1469598103934665603ull;   // FNV-1a over the coefficient bits
  for (int i = 0; i < n_coeffs; ++i) {
    uint64_t bits;
    std::memcpy(&bits, &a[i], 8);
    h = (h ^ bits) * 1099511628211ull;
  }
  key.a_hash = h;
  if (!(w->gexec && key == w->gkey)) {
    if (!(key == w->gpending && (int64_t)spmv_grid_size(A) <= ctx->tun.cheby_graph)) {
      w->gpending = key;
      return QP_OK;
    }
    // second identical call in a row: record it
    hipGraph_t graph = nullptr;
    const Stats before = ctx->stats;
    QP_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const int rc = launch();
    w->gstats = Stats();
    w->gstats.n_matvec = ctx->stats.n_matvec - before.n_matvec;
    w->gstats.n_launch = ctx->stats.n_launch - before.n_launch;
    w->gstats.spmv_bytes = ctx->stats.spmv_bytes - before.spmv_bytes;
    ctx->stats = before;
    const hipError_t ec = hipStreamEndCapture(ctx->stream, &graph);
    if (rc != QP_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    QP_HIP(ec);
    if (w->gexec) {
      (void)hipGraphExecDestroy(w->gexec);
      w->gexec = nullptr;
    }
    const hipError_t ei = hipGraphInstantiate(&w->gexec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    QP_HIP(ei);
    w->gkey = key;
  }
  QP_HIP(hipGraphLaunch(w->gexec, ctx->stream));
  ctx->stats.n_graph_launch++;
  ctx->stats.n_matvec += w->gstats.n_matvec;
  ctx->stats.n_launch += w->gstats.n_launch;
  ctx->stats.spmv_bytes += w->gstats.spmv_bytes;
  *done = true;
  return QP_OK;
}

extern "C" {

// ---------------------------------------------------------------------------
// Chebyshev
// ---------------------------------------------------------------------------
int qp_cheby_create(qp_ctx* ctx, int64_t n, qp_cheby** out) {
  QP_TRY
  if (!ctx || !out || n < 0) return qp::fail(QP_E_BAD_ARG, "qp_cheby_create: bad arguments");
  QP_CHECK(use(ctx));
  auto w = std::make_unique<qp_cheby>();
  w->ctx = ctx;
  w->n = n;
  QP_CHECK(dev_alloc(&w->bufA, (size_t)n));
  QP_CHECK(dev_alloc(&w->acc, (size_t)n));
  *out = w.release();
  return QP_OK;
  QP_CATCH
}

int qp_cheby_destroy(qp_cheby* w) {
  QP_TRY
  if (!w) return QP_OK;
  (void)hipSetDevice(w->ctx->device);
  (void)hipStreamSynchronize(w->ctx->stream);
  if (w->bufA) (void)hipFree(w->bufA);
  if (w->bufC) (void)hipFree(w->bufC);
  if (w->bufD) (void)hipFree(w->bufD);
  if (w->acc) (void)hipFree(w->acc);
  if (w->chk_part) (void)hipFree(w->chk_part);
  if (w->chk_out) (void)hipFree(w->chk_out);
  if (w->gexec) (void)hipGraphExecDestroy(w->gexec);
  delete w;
  return QP_OK;
  QP_CATCH
}

int qp_acc_schedule_host(const double* a, int n_coeffs, qp_acc_defer* out) {
  if (!a || !out || n_coeffs < 2) return qp::fail(QP_E_BAD_ARG, "qp_acc_schedule_host: bad arguments");
  acc_schedule(a, n_coeffs, true, out);
  return QP_OK;
}

int qp_cheby_term(qp_operator* op, const qp_state* x, int64_t xoff, const qp_state* v0, qp_state* vout,
                  const qp_state* acc_in, qp_state* acc_out, qp_c128 c, double beta, double a_prev, double a,
                  qp_c128 phase, const qp_acc_defer* defer) {
  QP_TRY
  const bool skip = defer && defer->skip;
  if (!op || !x || (!acc_out && !skip)) return qp::fail(QP_E_BAD_ARG, "qp_cheby_term: NULL argument");
  qp::ChebyEpi e;
  QP_CHECK(cheby_term_args("qp_cheby_term", op, x, xoff, v0, vout, acc_in, acc_out, c, beta, a_prev, a, phase, defer, &e));
  auto overlaps = [&](const qp_state* s) { return s && s->d < x->d + x->n && x->d < s->d + s->n; };
  if (overlaps(vout) || overlaps(acc_out)) return qp::fail(QP_E_BAD_ARG, "qp_cheby_term: outputs must not overlap the gathered x");
  QP_CHECK(use(op->ctx));
  return qp::launch_spmv_cheby(op->ctx->stream, op->A, x->d, e, &op->ctx->stats);
  QP_CATCH
}

int qp_operator_walk2_info(const qp_operator* op, int64_t out[8]) {
  QP_TRY
  if (!op || !out) return qp::fail(QP_E_BAD_ARG, "qp_operator_walk2_info: NULL argument");
  const qp::Walk2Rule rule = walk2_rule(op);
  const bool on = rule != qp::kWalk2None;
  // the cut the launcher gets (kernels_walk2.hip: launch_hrb_walk2_cheby): rows of a chunk that form z, chunks per strip step,
  // z steps per wavefront, segments per strip column
  const qp::Walk2Cut C = qp::walk2_cut_of(rule, op->walk2, qp::walk_matrix(op->A), qp::walk_knobs(op->ctx->tun), qp::device_cu_count());
  out[0] = on ? 1 : 0;
  out[1] = on ? op->walk2.W0 : 0;
  out[2] = on ? op->walk2.R1 : 0;
  out[3] = on ? op->walk2.n_edge : 0;
  out[4] = C.G.W;
  out[5] = C.G.S2;
  out[6] = C.G.L;
  out[7] = C.G.nseg;
  return QP_OK;
  QP_CATCH
}

int qp_operator_small_plan(const qp_operator* op, int kind, int m, int64_t out[4]) {
  QP_TRY
  if (!op || !out || (kind != 0 && kind != 1) || (kind == 1 && m < 1)) return qp::fail(QP_E_BAD_ARG, "qp_operator_small_plan: bad arguments");
  qp::SmallPlan p;
  const bool taken = kind == 0 ? cheby_small_fits(op, &p) : small_sweep_fits(op, op->A.nrows, m, &p);
  out[0] = taken ? 1 : 0;
  out[1] = taken ? p.lanes : 0;
  out[2] = taken ? p.ent : 0;
  out[3] = taken ? p.rows_per_group : 0;
  return QP_OK;
  QP_CATCH
}

int qp_cheby_step(qp_cheby* w, qp_operator* op, qp_state* psi, const double* a, int n_coeffs, double Delta,
                  double E_min, double dt, double wrk_dt, double limit, int check_normalization) {
  QP_TRY
  if (!w || !op || !psi || !a) return qp::fail(QP_E_BAD_ARG, "qp_cheby_step: NULL argument");
  if (op->A.nrows != op->A.ncols || psi->n != op->A.nrows || w->n != psi->n)
    return qp::fail(QP_E_BAD_ARG, "qp_cheby_step: shape mismatch");
  QP_CHECK(cheby_step_args(&dt, wrk_dt, n_coeffs, Delta));
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  const qp::ScopedRange step_range(ctx->tun.roctx != 0 || qp::ranges_enabled_by_env(), "prop_step!");   // src/cheby_propagator.jl:349
  const ChebyScalars sc(Delta, E_min, dt);
  const int nterms = n_coeffs - 1;
  const DevMatrix& A = op->A;
  auto launch_term = [&](const double2* x, const qp::ChebyEpi& e) -> int {
    const qp::ScopedRange mv_range(ctx->tun.roctx != 0 || qp::ranges_enabled_by_env(), "matrix-vector product");   // src/cheby.jl:175, :189
    return qp::launch_spmv_cheby(ctx->stream, A, x, e, &ctx->stats);
  };
  const int nwg = qp::spmv_grid_size(A);
  if (check_normalization) {
    if (w->chk_wg < nwg) {
      if (w->chk_part) QP_HIP(hipFree(w->chk_part));
      QP_CHECK(dev_alloc(&w->chk_part, (size_t)3 * nwg));
      w->chk_wg = nwg;
    }
    if (w->chk_terms < nterms) {
      if (w->chk_out) QP_HIP(hipFree(w->chk_out));
      QP_CHECK(dev_alloc(&w->chk_out, (size_t)3 * nterms));
      w->chk_terms = nterms;
    }
  }
  // the two-term strip walk rotates four term vectors: the two beyond Psi's and bufA are allocated on first use (here, not inside a
  // stream capture)
  if (ChebySequence::pairs_possible(n_coeffs, check_normalization != 0, false) && !w->bufC && walk2_wanted(op)) {
    QP_CHECK(dev_alloc(&w->bufC, (size_t)w->n));
    QP_CHECK(dev_alloc(&w->bufD, (size_t)w->n));
  }
  auto launches = [&] { return cheby_step_launches(w, op, psi, a, n_coeffs, sc, check_normalization != 0, false, launch_term); };
  bool done = false;
  if (!check_normalization) QP_CHECK(cheby_step_graph(w, op, psi, a, n_coeffs, Delta, E_min, dt, launches, &done));
  if (!done) QP_CHECK(launches());
  ctx->stats.n_cheby_steps++;
  if (check_normalization && nterms >= 2) {
    std::vector<double> h((size_t)3 * nterms);
    QP_HIP(hipMemcpyAsync(h.data(), w->chk_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QP_HIP(hipStreamSynchronize(ctx->stream));
    if (const int bad = cheby_normalization_verdict(h.data(), nterms, limit)) {
      w->bad_term = bad;
      return qp::fail(QP_E_NORMALIZATION, "Incorrect normalization (E_min=%g, Delta=%g) in term %d", E_min, Delta, bad);
    }
  }
  return QP_OK;
  QP_CATCH
}

// ---------------------------------------------------------------------------
// batched states (BASELINE configs[4]): panel X[i*b + s]
// ---------------------------------------------------------------------------
int qp_cheby_step_batched(qp_cheby* w, qp_operator* op, qp_state* psi, int batch, const double* a, int n_coeffs,
                          double Delta, double E_min, double dt, double wrk_dt) {
  QP_TRY
  if (!w || !op || !psi || !a || batch < 1) return qp::fail(QP_E_BAD_ARG, "qp_cheby_step_batched: bad arguments");
  const int64_t n = op->A.nrows;
  if (op->A.nrows != op->A.ncols || psi->n != n * batch || w->n != psi->n)
    return qp::fail(QP_E_BAD_ARG, "qp_cheby_step_batched: shape mismatch (operator %lld, batch %d, panel %lld)",
                    (long long)n, batch, (long long)psi->n);
  QP_CHECK(cheby_step_args(&dt, wrk_dt, n_coeffs, Delta));
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  // a dense operator (QP_FMT_DENSE): H X on the fp64 matrix cores (csrc/kernels_dense.hip), straight from the operator's own
  // value array; knob dense_panel_mfma 0 sends it through the sparse panel kernels like any CSR operator (A/B)
  const bool dense = op->A.format == QP_FMT_DENSE && ctx->tun.dense_panel_mfma != 0 && (op->A.vals || op->A.vals_r);
  if (!dense) QP_CHECK(operator_csr_mirror(op));
  // kernel choice (knob spmm_rows): the wave-per-row kernel for wide panels, else the state-tiled kernel
  const bool rows_kernel = !dense && qp::spmm_uses_rows_kernel(ctx->tun, batch);
  const int32_t* order = nullptr;   // row walk of the wave-per-row kernel
  const qp::SpmmTiles* tiles = nullptr;   // LDS-staged tiles of a lattice operator's interior rows (knob spmm_rw -1, the default)
  if (rows_kernel && ctx->tun.spmm_rw < 0) QP_CHECK(operator_spmm_tiles(op, &tiles));
  if (rows_kernel && !tiles) QP_CHECK(operator_spmm_order(op, batch, &order));

  // the term loop and buffer rotation of qp_cheby_step, element = (row, state)
  auto launch_term = [&](const double2* x, const qp::ChebyEpi& e) -> int {
    if (dense) return qp::launch_dense_zgemm_cheby(ctx->stream, op->A, x, batch, e, &ctx->stats);
    if (tiles)
      return qp::launch_spmm_tile_cheby(ctx->stream, op->m_rowptr, op->m_cols, op->m_vals, x, n, op->A.nnz, batch, e, ctx->tun,
                                        *tiles, &ctx->stats);
    return qp::launch_spmm_cheby(ctx->stream, op->m_rowptr, op->m_cols, op->m_vals, x, n, op->A.nnz, batch, e, ctx->tun,
                                 rows_kernel, order, &ctx->stats);
  };
  QP_CHECK(cheby_step_launches(w, op, psi, a, n_coeffs, ChebyScalars(Delta, E_min, dt), false, true, launch_term));
  ctx->stats.n_cheby_steps++;
  return QP_OK;
  QP_CATCH
}

// ---------------------------------------------------------------------------
// boundary / interior split of one fused term (overlap of the multi-GPU exchange)
// ---------------------------------------------------------------------------
int qp_split_create(qp_operator* op, const int64_t* send_rows, int64_t nsend, qp_split** out) {
  QP_TRY
  if (!op || !out || nsend < 0 || (nsend > 0 && !send_rows)) return qp::fail(QP_E_BAD_ARG, "qp_split_create: bad arguments");
  const DevMatrix& A = op->A;
  if (A.format != QP_FMT_RBCSR && A.format != QP_FMT_HRB)
    return qp::fail(QP_E_BAD_ARG, "qp_split_create needs a row-block device format (got %d)", A.format);
  QP_CHECK(use(op->ctx));
  // the partition itself is plain data (cheby_plan.h: plan_split); the interior as a strip walk where the operator has a plan
  const qp::WalkPlan* P = (A.walk && A.walk->valid && A.format == QP_FMT_HRB) ? A.walk : nullptr;
  const SplitWalk pw = P ? SplitWalk{1, P->K, P->fd, P->g, P->glong, P->W0, P->R1} : SplitWalk();
  SplitPlan plan;
  QP_CHECK(plan_split(A.nrows, op->u_rowptr.data(), op->u_col.data(), send_rows, nsend, qp::kThreads / 64, pw, &plan));
  auto sp = std::make_unique<qp_split>();
  sp->op = op;
  sp->device = op->ctx->device;
  sp->n_boundary = (int64_t)plan.boundary.size();
  sp->n_interior = (int64_t)plan.interior.size();
  sp->nsend = nsend;
  sp->wait_from_wg = plan.wait_from_wg;
  sp->n_waiting_wg = plan.n_waiting_wg;
  QP_CHECK(dev_upload(&sp->bmap_boundary, plan.boundary.data(), plan.boundary.size()));
  QP_CHECK(dev_upload(&sp->bmap_interior, plan.interior.data(), plan.interior.size()));
  QP_CHECK(dev_upload(&sp->mirror, plan.mirror.data(), plan.mirror.size()));
  QP_HIP(hipEventCreateWithFlags(&sp->ev_b, hipEventDisableTiming));
  QP_HIP(hipEventCreateWithFlags(&sp->ev_i, hipEventDisableTiming));
  QP_CHECK(dev_alloc(&sp->counter, 2));
  QP_HIP(hipMemset(sp->counter, 0, 2 * sizeof(unsigned)));
  QP_HIP(hipHostMalloc((void**)&sp->timeout_host, sizeof(unsigned), hipHostMallocMapped));
  *sp->timeout_host = 0;
  QP_HIP(hipHostGetDevicePointer((void**)&sp->timeout_dev, sp->timeout_host, 0));
  if (plan.walk) {
    qp::WalkPlan W = *A.walk;
    W.W0 = plan.W0;
    W.R1 = plan.R1;
    W.n_edge = (int64_t)plan.edge.size();
    QP_CHECK(dev_upload(&W.edge_map, plan.edge.data(), plan.edge.size()));
    sp->walk = W;
  }
  *out = sp.release();
  return QP_OK;
  QP_CATCH
}

int qp_split_destroy(qp_split* sp) {
  QP_TRY
  if (!sp) return QP_OK;
  (void)hipSetDevice(sp->device);
  (void)hipDeviceSynchronize();
  if (sp->bmap_boundary) (void)hipFree(sp->bmap_boundary);
  if (sp->bmap_interior) (void)hipFree(sp->bmap_interior);
  if (sp->mirror) (void)hipFree(sp->mirror);
  if (sp->walk.edge_map) (void)hipFree(sp->walk.edge_map);
  if (sp->counter) (void)hipFree(sp->counter);
  if (sp->timeout_host) (void)hipHostFree(sp->timeout_host);
  if (sp->ev_b) (void)hipEventDestroy(sp->ev_b);
  if (sp->ev_i) (void)hipEventDestroy(sp->ev_i);
  delete sp;
  return QP_OK;
  QP_CATCH
}

int qp_split_info(const qp_split* sp, int64_t* n_boundary_blocks, int64_t* n_interior_blocks) {
  if (!sp) return qp::fail(QP_E_BAD_ARG, "split is NULL");
  if (n_boundary_blocks) *n_boundary_blocks = sp->n_boundary;
  if (n_interior_blocks) *n_interior_blocks = sp->n_interior;
  return QP_OK;
}

int qp_split_walk_info(const qp_split* sp, int64_t out[4]) {
  if (!sp || !out) return qp::fail(QP_E_BAD_ARG, "qp_split_walk_info: NULL argument");
  out[0] = sp->walk.valid ? 1 : 0;
  out[1] = sp->walk.valid ? sp->walk.W0 : 0;
  out[2] = sp->walk.valid ? sp->walk.R1 : 0;
  out[3] = sp->walk.valid ? sp->walk.n_edge : 0;
  return QP_OK;
}

/* synchronises the device; returns QP_E_INTERNAL if an in-launch wait ever timed out */
int qp_split_check(qp_split* sp) {
  QP_TRY
  if (!sp) return qp::fail(QP_E_BAD_ARG, "split is NULL");
  QP_HIP(hipSetDevice(sp->device));
  QP_HIP(hipDeviceSynchronize());
  return split_timed_out(sp);
  QP_CATCH
}

int qp_cheby_term_split(qp_operator* op, qp_split* sp, void* boundary_stream, int first, const qp_state* x,
                        int64_t xoff, const qp_state* v0, qp_state* vout, const qp_state* acc_in, qp_state* acc_out,
                        qp_state* slab, qp_c128 c, double beta, double a_prev, double a, qp_c128 phase,
                        const qp_acc_defer* defer) {
  QP_TRY
  const bool skip = defer && defer->skip;
  if (!op || !sp || sp->op != op || !boundary_stream || !x || (!acc_out && !skip))
    return qp::fail(QP_E_BAD_ARG, "qp_cheby_term_split: bad arguments");
  qp::ChebyEpi e;
  QP_CHECK(cheby_term_args("qp_cheby_term_split", op, x, xoff, v0, vout, acc_in, acc_out, c, beta, a_prev, a, phase, defer, &e));
  if (slab && slab->n < sp->nsend) return qp::fail(QP_E_BAD_ARG, "qp_cheby_term_split: slab too small");
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  hipStream_t S_c = ctx->stream, S_x = (hipStream_t)boundary_stream;
  // (the term is counted as ONE mat-vec: by its interior launch, or by the boundary launch where there is no interior block)
  qp::RowSet rb{sp->bmap_boundary, sp->n_boundary, sp->n_interior == 0};
  qp::RowSet ri{sp->bmap_interior, sp->n_interior, true};
  if (sp->walk.valid) {   // lattice operator: the interior as a strip walk; CUs beyond the edge workgroups' stay free (knob) for
    ri.walk = &sp->walk;  // the boundary launch and the collective's kernel that run beside it
    ri.reserve_cu = qp::kWalkReserveCu;
  }
  QP_CHECK(split_timed_out(sp));
  // knob split_mode: 1 = in-launch counter hand-off, 0 = events on both streams, 2 (default) = the counter
  // where it is safe by construction: the polling workgroups hold their CU slots while the boundary launch
  // they wait for may sit behind a collective that depends on other ranks, so they must be few enough to
  // leave room for that launch and the collective's kernel on every CU (at most one per CU here)
  const int mode = op->ctx->tun.split_mode;
  const bool flag_mode = mode == 1 || (mode == 2 && sp->n_waiting_wg <= 256);
  if (first && flag_mode) {
    // the caller joined both streams: restart the signal counter (keeps it far from wrap)
    QP_HIP(hipMemsetAsync(sp->counter, 0, sizeof(unsigned), S_c));
    sp->signals_issued = 0;
    QP_HIP(hipEventRecord(sp->ev_i, S_c));
    QP_HIP(hipStreamWaitEvent(S_x, sp->ev_i, 0));
  }
  if (!first) {
    // boundary(m) overwrites rows that interior(m-1) gathered from, and vice versa.  The side
    // stream takes a queue-level event wait (its idle time is hidden); the main stream either
    // does the same (mode 0) or lets only the adjacent workgroups of the interior launch poll
    // the boundary launch's completion counter (mode 1: no idle gap between interior launches)
    QP_HIP(hipStreamWaitEvent(S_x, sp->ev_i, 0));
    if (!flag_mode) QP_HIP(hipStreamWaitEvent(S_c, sp->ev_b, 0));
  }
  if (flag_mode) {
    ri.sync.wait = sp->counter;
    ri.sync.wait_target = sp->signals_issued;      // every boundary workgroup launched so far
    ri.sync.wait_from_wg = sp->wait_from_wg;
    ri.sync.timeout_flag = sp->timeout_dev;
    ri.sync.spin_limit = 1u << std::min(std::max(op->ctx->tun.split_spin_log2, 4), 31);
#ifdef QP_DEVELOPER
    rb.sync.signal = (op->ctx->tun.split_dbg & 1) ? nullptr : sp->counter;   // (time-out test: the boundary launch does not signal)
#else
    rb.sync.signal = sp->counter;
#endif
    sp->signals_issued += (unsigned)((sp->n_boundary + qp::kThreads / 64 - 1) / (qp::kThreads / 64));
  }
  qp::ChebyEpi eb = e;
  if (slab && vout) {   // the slab carries the new term vector (what the next term gathers)
    eb.mirror = sp->mirror;
    eb.slab = slab->d;
  }
  if (sp->n_boundary > 0) QP_CHECK(qp::launch_spmv_cheby(S_x, op->A, x->d, eb, &ctx->stats, &rb));
  if (!flag_mode) QP_HIP(hipEventRecord(sp->ev_b, S_x));
  if (sp->n_interior > 0) QP_CHECK(qp::launch_spmv_cheby(S_c, op->A, x->d, e, &ctx->stats, &ri));
  QP_HIP(hipEventRecord(sp->ev_i, S_c));
  return QP_OK;
  QP_CATCH
}

// ---------------------------------------------------------------------------
// propagate step loop (src/propagate.jl:283-344)
// ---------------------------------------------------------------------------
// Small systems: the whole time grid in one persistent single-workgroup launch
// (kernels_small.hip: cheby_propagate_small_kernel).  Same arguments as qp_propagate, method 0.
static int propagate_cheby_small(qp_operator* op, qp_state* psi, const qp_prop_spec* spec, const qp::SmallPlan& plan,
                                 const double* dts,
                                 const qp_c128* coeff_table, int ncoeffs, int nsteps, qp_operator* const* observables,
                                 int nobs, qp_c128* expvals_out, qp_c128* states_out) {
  qp_ctx* ctx = op->ctx;
  qp_cheby* w = spec->cheby;
  const int64_t n = psi->n;
  const size_t rows = (size_t)nsteps + 1;
  if (!w || !spec->a) return qp::fail(QP_E_BAD_ARG, "qp_propagate: NULL Chebychev workspace");
  if (op->A.nrows != op->A.ncols || n != op->A.nrows || w->n != n) return qp::fail(QP_E_BAD_ARG, "qp_propagate: shape mismatch");
  QP_CHECK(cheby_step_args(nullptr, spec->wrk_dt, spec->n_coeffs, spec->Delta));
  for (int k = 0; k < nsteps; ++k) {
    QP_CHECK(cheby_step_args(&dts[k], spec->wrk_dt, spec->n_coeffs, spec->Delta));
    if ((dts[k] > 0) != (dts[0] > 0)) return qp::fail(QP_E_BAD_ARG, "qp_propagate: time steps change sign");
  }
  QP_CHECK(operator_csr_mirror(op));
  for (int o = 0; o < nobs; ++o) QP_CHECK(operator_csr_mirror(observables[o]));
  const ChebyScalars sc(spec->Delta, spec->E_min, dts[0]);

  qp::SmallArgs a;
  a.n = n;
  a.nnz = op->A.nnz;
  a.lanes = plan.lanes;
  a.ent = plan.ent;
  a.rows_per_group = plan.rows_per_group;
  a.obs_lanes = plan.obs_lanes;
  a.rowptr = op->m_rowptr;
  a.cols = op->m_cols;
  a.map = op->m_map;
  a.planes = op->planes_dev;
  a.nops = op->nops;
  a.ncoeffs = ncoeffs;
  a.scale = d2(op->scale);
  a.nsteps = nsteps;
  a.n_coeffs = spec->n_coeffs;
  a.c = d2(sc.c);
  a.beta = sc.beta;
  a.phase = d2(sc.phase);
  a.psi = psi->d;
  a.nobs = nobs;
  a.check = spec->check_normalization ? 1 : 0;
  a.limit = spec->limit;

  // one staging buffer: [table | a | obs descriptors | fail | expvals | work | states]
  std::vector<void*> owned;
  struct Free {
    std::vector<void*>& v;
    ~Free() {
      for (void* p : v) (void)hipFree(p);
    }
  } guard{owned};
  auto upload = [&](const void* src, size_t bytes, void** out) -> int {
    void* d = nullptr;
    QP_HIP(hipMalloc(&d, std::max<size_t>(bytes, 16)));
    owned.push_back(d);
    if (src && bytes) QP_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *out = d;
    return QP_OK;
  };
  void* p = nullptr;
  QP_CHECK(upload(coeff_table, sizeof(qp_c128) * (size_t)nsteps * ncoeffs, &p));
  a.table = static_cast<const double2*>(p);
  QP_CHECK(upload(spec->a, sizeof(double) * (size_t)spec->n_coeffs, &p));
  a.a = static_cast<const double*>(p);
  std::vector<qp::SmallObs> hobs((size_t)nobs);
  for (int o = 0; o < nobs; ++o) hobs[o] = qp::SmallObs{observables[o]->m_rowptr, observables[o]->m_cols, observables[o]->m_vals};
  QP_CHECK(upload(hobs.data(), sizeof(qp::SmallObs) * (size_t)nobs, &p));
  a.obs = static_cast<const qp::SmallObs*>(p);
  QP_CHECK(upload(nullptr, sizeof(int) * 4, &p));
  a.fail = static_cast<int*>(p);
  QP_HIP(hipMemsetAsync(a.fail, 0, sizeof(int) * 4, ctx->stream));
  QP_CHECK(upload(nullptr, sizeof(double2) * rows * (size_t)nobs, &p));
  a.expvals = static_cast<double2*>(p);
  if (states_out) {
    QP_CHECK(upload(nullptr, sizeof(double2) * rows * (size_t)n, &p));
    a.states = static_cast<double2*>(p);
  }
  QP_CHECK(qp::launch_cheby_propagate_small(ctx->stream, a, &ctx->stats));
  ctx->stats.n_cheby_steps += nsteps;
  int fail[4] = {0, 0, 0, 0};
  QP_HIP(hipMemcpyAsync(fail, a.fail, sizeof(fail), hipMemcpyDeviceToHost, ctx->stream));
  if (nobs > 0)
    QP_HIP(hipMemcpyAsync(expvals_out, a.expvals, sizeof(double2) * rows * (size_t)nobs, hipMemcpyDeviceToHost, ctx->stream));
  if (states_out)
    QP_HIP(hipMemcpyAsync(states_out, a.states, sizeof(double2) * rows * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  QP_HIP(hipStreamSynchronize(ctx->stream));
  // leave the operator as the step-by-step loop would: holding the last interval's values
  if (ncoeffs > 0) QP_CHECK(qp_operator_set_coeffs(op, coeff_table + (size_t)(nsteps - 1) * ncoeffs, ncoeffs));
  if (fail[0])
    return qp::fail(QP_E_NORMALIZATION, "Incorrect normalization (E_min=%g, Delta=%g) in step %d, term %d", spec->E_min,
                    spec->Delta, fail[1] + 1, fail[2] + 1);
  return QP_OK;
}

int qp_propagate(qp_operator* op, qp_state* psi, const qp_prop_spec* spec, const double* dts,
                 const qp_c128* coeff_table, int ncoeffs, int nsteps, qp_operator* const* observables, int nobs,
                 qp_c128* expvals_out, qp_c128* states_out) {
  QP_TRY
  if (!op || !psi || !spec || !dts || nsteps < 0 || nobs < 0 || (nobs > 0 && (!observables || !expvals_out)))
    return qp::fail(QP_E_BAD_ARG, "qp_propagate: bad arguments");
  if (ncoeffs != op->ncoeffs || (ncoeffs > 0 && nsteps > 0 && !coeff_table))
    return qp::fail(QP_E_BAD_ARG, "qp_propagate: expected %d coefficients per step", op->ncoeffs);
  if (spec->method != 0 && spec->method != 1) return qp::fail(QP_E_BAD_ARG, "qp_propagate: bad method");
  for (int o = 0; o < nobs; ++o)
    if (!observables[o] || observables[o]->A.nrows != psi->n || observables[o]->A.ncols != psi->n)
      return qp::fail(QP_E_BAD_ARG, "qp_propagate: observable %d has the wrong shape", o);
  qp_ctx* ctx = op->ctx;
  QP_CHECK(use(ctx));
  const int64_t n = psi->n;
  const size_t rows = (size_t)nsteps + 1;
  if (spec->method == 0 && nsteps > 0) {
    qp::SmallPlan plan;
    if (cheby_small_fits(op, &plan))
      return propagate_cheby_small(op, psi, spec, plan, dts, coeff_table, ncoeffs, nsteps, observables, nobs,
                                   expvals_out, states_out);
  }
  // device staging, released at the end: observable partials and the state history
  double2* d_part = nullptr;
  double2* d_tmp = nullptr;
  double2* d_states = nullptr;
  struct Free {
    double2 *&a, *&b, *&c;
    ~Free() {
      if (a) (void)hipFree(a);
      if (b) (void)hipFree(b);
      if (c) (void)hipFree(c);
    }
  } guard{d_part, d_tmp, d_states};
  if (nobs > 0) {
    QP_CHECK(dev_alloc(&d_part, rows * nobs * kRedBlocks));
    QP_CHECK(dev_alloc(&d_tmp, (size_t)n));
  }
  if (states_out) QP_CHECK(dev_alloc(&d_states, rows * (size_t)n));
  auto record = [&](size_t row) -> int {
    for (int o = 0; o < nobs; ++o) {   // <psi|O|psi> = dot(psi, O psi)
      qp::PlainEpi e;
      e.y = d_tmp;
      e.alpha = make_double2(1.0, 0.0);
      e.beta = make_double2(0.0, 0.0);
      e.beta_zero = 1;
      QP_CHECK(qp::launch_spmv_plain(ctx->stream, observables[o]->A, psi->d, e, &ctx->stats));
      QP_CHECK(qp::launch_dot_partials(ctx->stream, psi->d, d_tmp, d_part + (row * nobs + o) * kRedBlocks, n, &ctx->stats));
    }
    if (d_states)
      QP_HIP(hipMemcpyAsync(d_states + row * (size_t)n, psi->d, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
    return QP_OK;
  };
  QP_CHECK(record(0));
  for (int k = 0; k < nsteps; ++k) {
    if (ncoeffs > 0) QP_CHECK(qp_operator_set_coeffs(op, coeff_table + (size_t)k * ncoeffs, ncoeffs));
    if (spec->method == 0) {
      const int rc = qp_cheby_step(spec->cheby, op, psi, spec->a, spec->n_coeffs, spec->Delta, spec->E_min, dts[k],
                                   spec->wrk_dt, spec->limit, spec->check_normalization);
      if (rc == QP_E_NORMALIZATION)   // name the step as well, in the words of the persistent kernel's report (propagate_cheby_small)
        return qp::fail(rc, "Incorrect normalization (E_min=%g, Delta=%g) in step %d, term %d", spec->E_min, spec->Delta, k + 1,
                        spec->cheby->bad_term);
      QP_CHECK(rc);
    } else {
      QP_CHECK(qp_newton_step(spec->newton, op, psi, dts[k], spec->func_id, spec->cb, spec->user, spec->norm_min,
                              spec->relerr, spec->max_restarts, nullptr));
    }
    QP_CHECK(record((size_t)k + 1));
  }
  if (nobs > 0) {
    std::vector<cplx> hp(rows * nobs * kRedBlocks);
    QP_HIP(hipMemcpyAsync(hp.data(), d_part, hp.size() * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QP_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < rows * nobs; ++i) {
      const cplx v = sum_partials(reinterpret_cast<const double2*>(hp.data() + i * kRedBlocks));
      expvals_out[i] = qp_c128{v.real(), v.imag()};
    }
  }
  if (states_out) {
    QP_HIP(hipMemcpyAsync(states_out, d_states, rows * (size_t)n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QP_HIP(hipStreamSynchronize(ctx->stream));
  }
  return QP_OK;
  QP_CATCH
}

}  // extern "C"
