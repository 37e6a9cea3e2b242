// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): pin_to_plane /
// pin_to_circle -- the tables (ms_set_pins), the enforcement program on X (k_pin_enforce) and the project lane's
// gradient pass (k_pin_grad).  The one-tile interpreter records both (CK_PIN_ENFORCE, CK_PIN_GRAD); MS_EXEC_PINS=0: both flush it
// first and run as launches of their own.  The launch counters count program runs either way.
namespace {

inline bool pins_set(const ms_ctx* c) { return c->pin_lane >= 0; }
inline bool pins_project(const ms_ctx* c) { return c->pin_lane == MS_PIN_LANE_PROJECT && c->pin_grad.n_grad + c->pin_grad.n_avg > 0; }

// run the enforcement program on X (what every caller then sees moved: the state of x is stale)
int pin_enforce_run(ms_ctx* c) {
  if (!pins_set(c) || c->pin_enf.n_stages == 0) return MS_OK;
  PinEnforceArgs a = c->pin_enf;
  a.x = c->buf[MS_BUF_X];
  HIPCHK(c, launch_pin_enforce(a, c->stream, c->exec_pins));  // (a record of the pack, or a launch behind a flush)
  ++c->pin_enforce_launches;
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
  return MS_OK;
}

// project lane: remove the pin rows from G (and from GC with the volume row) after the gradient pass, and correct
// tile0's <g,gC> / <gC,gC> partials by the change at the touched rows (before the fold takes them)
int pin_grad_run(ms_ctx* c, bool volrow) {
  if (!pins_project(c)) return MS_OK;
  PinGradArgs a = c->pin_grad;
  a.x = c->buf[MS_BUF_X];
  a.g = c->buf[MS_BUF_G];
  a.gc = volrow ? c->buf[MS_BUF_GC] : nullptr;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile = c->tile0;
  HIPCHK(c, launch_pin_grad(a, c->stream, c->exec_pins));
  ++c->pin_grad_launches;
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_pins(ms_ctx* c, int n_params, const double* params, int n_stages, const int32_t* stage_kind,
                const int32_t* stage_param, const int32_t* stage_off, const int32_t* item_row,
                const int32_t* item_arg, int lane, int n_grad, const int32_t* grad_row, const int32_t* grad_kind,
                const int32_t* grad_param, int n_avg, const int32_t* avg_param, const int32_t* avg_off,
                const int32_t* avg_row) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_set_pins: pin constraints are single-shard only");
  if (int rc = drop_table(c, c->d_pins)) return rc;
  c->pin_enf = PinEnforceArgs{};
  c->pin_grad = PinGradArgs{};
  c->pin_lane = -1;
  if (!params) return MS_OK;
  if (n_params <= 0 || n_stages < 0 || n_grad < 0 || n_avg < 0 || (n_stages > 0 && (!stage_kind || !stage_param || !stage_off)) ||
      (lane != MS_PIN_LANE_SKIP && lane != MS_PIN_LANE_PROJECT))
    return fail(c, MS_ERR_INVALID, "ms_set_pins: bad argument");
  if (lane != MS_PIN_LANE_PROJECT) n_grad = n_avg = 0;  // (the skip lane has no gradient tables)
  if ((n_grad > 0 && (!grad_row || !grad_kind || !grad_param)) || (n_avg > 0 && (!avg_param || !avg_off || !avg_row)))
    return fail(c, MS_ERR_INVALID, "ms_set_pins: missing gradient table");
  // offsets first: they size everything below
  for (int s = 0; s < n_stages; ++s)
    if (stage_off[s] < 0 || stage_off[s + 1] < stage_off[s]) return fail(c, MS_ERR_INVALID, "ms_set_pins: stage offsets");
  for (int s = 0; s < n_avg; ++s)
    if (avg_off[s] < 0 || avg_off[s + 1] <= avg_off[s]) return fail(c, MS_ERR_INVALID, "ms_set_pins: support offsets");
  const int nv = c->til.nv;
  const int n_items = n_stages > 0 ? stage_off[n_stages] : 0;
  const int n_avg_rows = n_avg > 0 ? avg_off[n_avg] : 0;
  if (n_items > 0 && (!item_row || !item_arg)) return fail(c, MS_ERR_INVALID, "ms_set_pins: missing item table");
  // validate everything the kernels index with, and map external rows to the library's order
  auto row_ok = [&](int r) { return r >= 0 && r < nv; };
  std::vector<int32_t> irow(n_items), grow(n_grad), arow(n_avg_rows);
  if (n_stages > 0 && stage_off[0] != 0) return fail(c, MS_ERR_INVALID, "ms_set_pins: stage_off[0] != 0");
  for (int s = 0; s < n_stages; ++s) {
    if (stage_off[s + 1] < stage_off[s]) return fail(c, MS_ERR_INVALID, "ms_set_pins: stage offsets decrease");
    const int k = stage_kind[s];
    if (k < MS_PIN_STAGE_FIXED || k > MS_PIN_STAGE_CIRCLE_GROUP) return fail(c, MS_ERR_INVALID, "ms_set_pins: stage kind");
    if (k != MS_PIN_STAGE_FIXED && (stage_param[s] < 0 || stage_param[s] >= n_params || stage_off[s + 1] == stage_off[s]))
      return fail(c, MS_ERR_INVALID, "ms_set_pins: group stage parameter / members");
    for (int i = stage_off[s]; i < stage_off[s + 1]; ++i)
      if (k == MS_PIN_STAGE_FIXED && ((item_arg[i] & 0xffffff) >= n_params || (item_arg[i] >> 24) > MS_PIN_OP_CIRCLE || item_arg[i] < 0))
        return fail(c, MS_ERR_INVALID, "ms_set_pins: op parameter row");
  }
  for (int i = 0; i < n_items; ++i) {
    if (!row_ok(item_row[i])) return fail(c, MS_ERR_INVALID, "ms_set_pins: item row out of range");
    irow[i] = c->til.iperm[item_row[i]];
  }
  std::vector<int32_t> touch;
  std::vector<char> seen(lane == MS_PIN_LANE_PROJECT ? nv : 0, 0);
  auto note = [&](int32_t r) {
    if (!seen[r]) {
      seen[r] = 1;
      touch.push_back(r);
    }
  };
  if (lane == MS_PIN_LANE_PROJECT) {
    for (int k = 0; k < n_grad; ++k) {
      if (!row_ok(grad_row[k]) || grad_param[k] < 0 || grad_param[k] >= n_params || grad_kind[k] < 0 || grad_kind[k] > MS_PIN_GRAD_RADIAL)
        return fail(c, MS_ERR_INVALID, "ms_set_pins: gradient row");
      grow[k] = c->til.iperm[grad_row[k]];
      if (seen[grow[k]]) return fail(c, MS_ERR_INVALID, "ms_set_pins: a gradient row appears twice");
      note(grow[k]);
    }
    if (n_avg > 0 && avg_off[0] != 0) return fail(c, MS_ERR_INVALID, "ms_set_pins: avg_off[0] != 0");
    for (int s = 0; s < n_avg; ++s) {
      if (avg_off[s + 1] <= avg_off[s] || avg_param[s] < 0 || avg_param[s] >= n_params)
        return fail(c, MS_ERR_INVALID, "ms_set_pins: support table");
    }
    for (int i = 0; i < n_avg_rows; ++i) {
      if (!row_ok(avg_row[i])) return fail(c, MS_ERR_INVALID, "ms_set_pins: support row out of range");
      arow[i] = c->til.iperm[avg_row[i]];
      note(arow[i]);
    }
  }
  // one allocation (ms_table_blob.h): params, then the int tables (an offset table without a stage / support is one 0)
  TableBlob b;
  const auto h_prm = b.f64(7 * (size_t)n_params, params);
  const auto h_sk = b.i32(n_stages, stage_kind), h_sp = b.i32(n_stages, stage_param);
  const auto h_so = n_stages > 0 ? b.i32(n_stages + 1, stage_off) : b.i32(1);
  const auto h_ir = b.i32(irow), h_ia = b.i32(n_items, item_arg);
  const auto h_gr = b.i32(grow), h_gk = b.i32(n_grad, grad_kind), h_gp = b.i32(n_grad, grad_param);
  const auto h_ap = b.i32(n_avg, avg_param);
  const auto h_ao = n_avg > 0 ? b.i32(n_avg + 1, avg_off) : b.i32(1);
  const auto h_ar = b.i32(arow), h_t = b.i32(touch);
  if (int rc = upload_table(c, b, &c->d_pins)) return rc;
  PinEnforceArgs& e = c->pin_enf;
  e.params = b.at(c->d_pins, h_prm);
  e.n_stages = n_stages;
  e.stage_kind = b.at(c->d_pins, h_sk);
  e.stage_param = b.at(c->d_pins, h_sp);
  e.stage_off = b.at(c->d_pins, h_so);
  e.item_row = b.at(c->d_pins, h_ir);
  e.item_arg = b.at(c->d_pins, h_ia);
  PinGradArgs& g = c->pin_grad;
  g.params = e.params;
  g.n_grad = n_grad;
  g.grad_row = b.at(c->d_pins, h_gr);
  g.grad_kind = b.at(c->d_pins, h_gk);
  g.grad_param = b.at(c->d_pins, h_gp);
  g.n_avg = n_avg;
  g.avg_param = b.at(c->d_pins, h_ap);
  g.avg_off = b.at(c->d_pins, h_ao);
  g.avg_row = b.at(c->d_pins, h_ar);
  g.n_touch = (int)touch.size();
  g.touch_row = b.at(c->d_pins, h_t);
  c->pin_lane = lane;
  c->carry.invalidate();  // (G no longer describes this row set)
  return MS_OK;
}

int ms_enforce_pins(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_enforce_pins: single shard only");
  if (!pins_set(c)) return fail(c, MS_ERR_STATE, "ms_enforce_pins: no pin tables (ms_set_pins)");
  int rc = pin_enforce_run(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  return MS_OK;
}

int ms_pin_stats(ms_ctx* c, int64_t stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->pin_lane;
  stats[1] = c->pin_enforce_launches;
  stats[2] = c->pin_grad_launches;
  stats[3] = c->pin_trials;
  return MS_OK;
}

}  // extern "C"
