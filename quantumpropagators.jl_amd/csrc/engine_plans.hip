// Device layer of the plans that decide HOW an operator runs.  The decisions -- device format, strip-walk plans, column-blocked
// mirror, the batched path's row order and LDS tiles -- are made on plain host data by the pure-host planning unit
// (operator_plans.h); each function here releases the old device arrays, calls the planner with the operator's pattern, the
// context's knobs and the device's CU count, uploads what came back and sets the operator's fields.
// Called from qp_operator_create / operator_build_device (engine_operator.hip) and, lazily, from the batched step (engine_cheby.hip).
#include "engine_host.h"

int choose_format(qp_operator* op, int requested, bool hermitian) {
  return choose_format(union_pattern_of(op), requested, hermitian, plan_knobs(op->ctx->tun));
}

int build_walk_plan(qp_operator* op) {
  dev_release(op->walk.edge_map);
  dev_release(op->walk2.edge_map);
  op->A.walk = nullptr;
  const WalkPlans R = plan_walk(union_pattern_of(op), op->layout);
  op->walk_reason = R.reason;
  op->walk_reason_text = R.text;
  op->walk = R.one;
  op->walk2 = R.two;
  if (op->walk.valid) {
    QP_CHECK(dev_upload(&op->walk.edge_map, R.edge.data(), R.edge.size()));
    op->A.walk = &op->walk;
  }
  if (op->walk2.valid) QP_CHECK(dev_upload(&op->walk2.edge_map, R.edge2.data(), R.edge2.size()));
  return QP_OK;
}

int build_colblock(qp_operator* op) {
  op->A.cb = nullptr;
  const ColBlockHost R = plan_colblock(union_pattern_of(op), op->layout, plan_knobs(op->ctx->tun), qp::device_cu_count());
  if (R.line_share >= 0.0) op->cb_line_share = R.line_share;
  if (!R.shape.valid) return QP_OK;
  qp::ColBlockPlan& C = op->cb;
  QP_CHECK(dev_upload(&C.segptr, R.segptr.data(), R.segptr.size()));
  QP_CHECK(dev_upload(&C.rowoff, R.rowoff.data(), R.rowoff.size()));
  QP_CHECK(dev_upload(&C.cols, R.cols.data(), R.cols.size()));
  QP_CHECK(dev_upload(&C.map, R.map.data(), R.map.size()));
  QP_CHECK(dev_alloc(&C.vals, (size_t)R.shape.nnz));
  static_cast<qp::ColBlockShape&>(C) = R.shape;
  op->A.cb = &op->cb;
  return QP_OK;
}

int operator_spmm_order(qp_operator* op, int batch, const int32_t** order_out) {
  const int knob = op->ctx->tun.spmm_strip;
  if (op->m_order_valid && op->m_order_batch == batch && op->m_order_knob == knob) {
    *order_out = op->m_order;
    return QP_OK;
  }
  dev_release(op->m_order);
  op->m_order_valid = true;
  op->m_order_batch = batch;
  op->m_order_knob = knob;
  op->m_order_g = op->m_order_sw = 0;
  *order_out = nullptr;
  const SpmmOrder R = plan_spmm_order(union_pattern_of(op), batch, knob);
  if (R.order.empty()) return QP_OK;
  QP_CHECK(dev_upload(&op->m_order, R.order.data(), R.order.size()));
  op->m_order_g = R.g;
  op->m_order_sw = R.sw;
  *order_out = op->m_order;
  return QP_OK;
}

int operator_spmm_tiles(qp_operator* op, const qp::SpmmTiles** out) {
  qp::SpmmTiles& P = op->m_tiles;
  const int knob = op->ctx->tun.spmm_strip;
  *out = nullptr;
  if (!P.built || P.knob != knob) {
    dev_release(P.tiles);
    dev_release(P.rest);
    dev_release(P.tab);
    P = qp::SpmmTiles();
    P.built = true;
    P.knob = knob;
    const SpmmTilesHost R = plan_spmm_tiles(union_pattern_of(op), knob);
    P.shape = R.shape;
    P.g = R.g;
    P.sw = R.sw;
    if (!R.tiles.empty()) {
      const SpmmTileTable tab = spmm_tile_table(R.shape, R.g);
      P.T = tab.T;
      QP_CHECK(dev_upload(&P.tab, tab.tab.data(), tab.tab.size()));
      QP_CHECK(dev_upload(&P.tiles, R.tiles.data(), R.tiles.size()));
      if (!R.rest.empty()) QP_CHECK(dev_upload(&P.rest, R.rest.data(), R.rest.size()));
      P.ntiles = (int64_t)R.tiles.size();
      P.nrest = (int64_t)R.rest.size();
      P.valid = 1;
    }
  }
  if (P.valid) *out = &P;
  return QP_OK;
}
