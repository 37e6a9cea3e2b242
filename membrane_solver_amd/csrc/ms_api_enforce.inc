// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): the enforce-only
// shape constraints fixed_plane / perimeter -- the setters, perimeter's table builder (also a host entry point of its
// own) and the two enforcer launches on buffer X.  The kernels are ms_enforce.hip's; neither is a record of the one-tile
// interpreter: each launch flushes it first, as the area lane does.
namespace {

inline bool fplane_set(const ms_ctx* c) { return c->fplane_set; }
inline bool perimeter_set(const ms_ctx* c) { return c->d_perim != nullptr; }

// every call that moves positions: what ms_project_area_cached invalidates
inline void enforce_only_moved(ms_ctx* c) {
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
}

// fixed_plane.enforce_constraint (fixed_plane.py:25-53) on buffer X
int fplane_run(ms_ctx* c) {
  if (!fplane_set(c)) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  FixedPlaneArgs a;
  a.nv = c->til.nv;
  a.vflags = c->d_vflags;
  a.x = c->buf[MS_BUF_X];
  for (int k = 0; k < 3; ++k) {
    a.n[k] = c->fplane_n[k];
    a.q[k] = c->fplane_q[k];
  }
  HIPCHK(c, launch_fixed_plane(a, c->stream));
  ++c->enforce_only_launches[0];
  enforce_only_moved(c);
  return MS_OK;
}

// perimeter.enforce_constraint (perimeter.py:27-74) on buffer X: one launch for every loop and pass
int perimeter_run(ms_ctx* c, double tol, int max_iter) {
  if (!perimeter_set(c) || c->perim.n_loops == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  PerimeterArgs a = c->perim;
  a.vflags = c->d_vflags;
  a.x = c->buf[MS_BUF_X];
  a.tol = tol;
  a.max_iter = max_iter;
  HIPCHK(c, launch_perimeter(a, c->stream));
  ++c->enforce_only_launches[1];
  enforce_only_moved(c);
  return MS_OK;
}

// perimeter's tables from external rows (PerimeterArgs in ms_internal.h describes them)
struct PerimTables {
  std::vector<int32_t> et, eh, vert_off, vrow, csr_off, csr_ent;
  int max_ent = 0, max_verts = 0;
};

const char* build_perimeter_tables(int nv, const int32_t* iperm, int n_loops, const int32_t* loop_off, const int32_t* tail,
                                   const int32_t* head, PerimTables& t) {
  if (loop_off[0] != 0) return "ms_set_perimeter: loop_off[0] != 0";
  for (int l = 0; l < n_loops; ++l)
    if (loop_off[l + 1] < loop_off[l]) return "ms_set_perimeter: loop offsets decrease";
  const int n_ent = loop_off[n_loops];
  t.et.resize(n_ent);
  t.eh.resize(n_ent);
  for (int i = 0; i < n_ent; ++i) {
    if (tail[i] < 0 || tail[i] >= nv || head[i] < 0 || head[i] >= nv) return "ms_set_perimeter: edge row out of range";
    t.et[i] = iperm[tail[i]];
    t.eh[i] = iperm[head[i]];
    if (t.et[i] < 0 || t.et[i] >= nv || t.eh[i] < 0 || t.eh[i] >= nv) return "ms_set_perimeter: row permutation out of range";
  }
  t.vert_off.assign(1, 0);
  t.csr_off.assign(1, 0);
  std::vector<int32_t> slot((size_t)nv, -1);  // library row -> its place among this loop's distinct vertices
  for (int l = 0; l < n_loops; ++l) {
    const int e0 = loop_off[l], e1 = loop_off[l + 1];
    const int v0 = (int)t.vrow.size();
    std::vector<int32_t> cnt;
    auto note = [&](int32_t r) {  // (dict order of perimeter.py:20-21: first appearance, tail before head)
      if (slot[r] < 0) {
        slot[r] = (int32_t)cnt.size();
        cnt.push_back(0);
        t.vrow.push_back(r);
      }
      ++cnt[slot[r]];
    };
    for (int i = e0; i < e1; ++i) {
      note(t.et[i]);
      note(t.eh[i]);
    }
    const int nvl = (int)cnt.size();
    const int base = t.csr_off.back();
    std::vector<int32_t> at((size_t)nvl);
    int run = base;
    for (int j = 0; j < nvl; ++j) {
      at[j] = run;
      run += cnt[j];
      t.csr_off.push_back(run);
    }
    t.csr_ent.resize((size_t)run);
    for (int i = e0; i < e1; ++i) {  // (list order per vertex: :22 the tail's -dir, :23 the head's +dir)
      t.csr_ent[at[slot[t.et[i]]]++] = -(i + 1);
      t.csr_ent[at[slot[t.eh[i]]]++] = i + 1;
    }
    for (int j = 0; j < nvl; ++j) slot[t.vrow[v0 + j]] = -1;
    t.vert_off.push_back((int32_t)t.vrow.size());
    t.max_ent = std::max(t.max_ent, e1 - e0);
    t.max_verts = std::max(t.max_verts, nvl);
  }
  return nullptr;
}

int perimeter_clear(ms_ctx* c) {
  if (int rc = drop_table(c, c->d_perim)) return rc;
  c->perim = PerimeterArgs{};
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_fixed_plane(ms_ctx* c, const double normal[3], const double point[3]) {
  if (!c) return MS_ERR_INVALID;
  if (!normal) {
    c->fplane_set = false;
    return MS_OK;
  }
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_set_fixed_plane: fixed_plane is not sharded (single GPU only)");
  if (!point) return fail(c, MS_ERR_INVALID, "ms_set_fixed_plane: NULL point");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(normal[k]) || !std::isfinite(point[k]))
      return fail(c, MS_ERR_INVALID, "ms_set_fixed_plane: the normal and the point must be finite");
  // fixed_plane.py:39-43: np.linalg.norm, then normal /= norm
  const double norm = std::sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
  if (!(norm >= 1e-15) || !std::isfinite(norm))
    return fail(c, MS_ERR_INVALID, "ms_set_fixed_plane: |normal| < 1e-15 (the module skips the projection: set no plane)");
  for (int k = 0; k < 3; ++k) {
    c->fplane_n[k] = normal[k] / norm;
    c->fplane_q[k] = point[k];
  }
  c->fplane_set = true;
  return MS_OK;
}

int ms_enforce_fixed_plane(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_enforce_fixed_plane: fixed_plane is not sharded (single GPU only)");
  if (!fplane_set(c)) return fail(c, MS_ERR_STATE, "ms_enforce_fixed_plane: no plane (ms_set_fixed_plane)");
  if (int rc = fplane_run(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  return MS_OK;
}

int ms_perimeter_tables_host(int nv, const int32_t* iperm, int n_loops, const int32_t* loop_off, const int32_t* tail,
                             const int32_t* head, int32_t counts[2], int32_t* e_tail, int32_t* e_head, int32_t* vert_off,
                             int32_t* vrow, int32_t* csr_off, int32_t* csr_ent) {
  if (nv < 0 || n_loops < 0 || !iperm || !loop_off || !tail || !head || !counts || !e_tail || !e_head || !vert_off || !vrow ||
      !csr_off || !csr_ent)
    return fail(nullptr, MS_ERR_INVALID, "ms_perimeter_tables_host: bad argument");
  PerimTables t;
  if (const char* why = build_perimeter_tables(nv, iperm, n_loops, loop_off, tail, head, t)) return fail(nullptr, MS_ERR_INVALID, why);
  counts[0] = (int32_t)t.et.size();
  counts[1] = (int32_t)t.vrow.size();
  std::copy(t.et.begin(), t.et.end(), e_tail);
  std::copy(t.eh.begin(), t.eh.end(), e_head);
  std::copy(t.vert_off.begin(), t.vert_off.end(), vert_off);
  std::copy(t.vrow.begin(), t.vrow.end(), vrow);
  std::copy(t.csr_off.begin(), t.csr_off.end(), csr_off);
  std::copy(t.csr_ent.begin(), t.csr_ent.end(), csr_ent);
  return MS_OK;
}

int ms_set_perimeter(ms_ctx* c, int n_loops, const int32_t* loop_off, const int32_t* tail, const int32_t* head,
                     const double* target) {
  if (!c) return MS_ERR_INVALID;
  if (int rc = perimeter_clear(c)) return rc;
  if (n_loops == 0) return MS_OK;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_set_perimeter: perimeter is not sharded (single GPU only)");
  if (n_loops < 0 || !loop_off || !target || (loop_off[n_loops] > 0 && (!tail || !head)))
    return fail(c, MS_ERR_INVALID, "ms_set_perimeter: bad argument");
  for (int l = 0; l < n_loops; ++l)
    if (!std::isfinite(target[l])) return fail(c, MS_ERR_INVALID, "ms_set_perimeter: a target perimeter is not finite");
  PerimTables t;
  if (const char* why = build_perimeter_tables(c->til.nv, c->til.iperm.data(), n_loops, loop_off, tail, head, t))
    return fail(c, MS_ERR_INVALID, why);
  // one allocation (ms_table_blob.h): the targets, the result cells, the two scratch arrays; the int tables
  TableBlob b;
  const auto h_tg = b.f64((size_t)n_loops, target), h_res = b.f64(2 * (size_t)n_loops), h_ent = b.f64(4 * (size_t)t.max_ent),
             h_gv = b.f64(4 * (size_t)t.max_verts);
  const auto h_lo = b.i32((size_t)n_loops + 1, loop_off), h_et = b.i32(t.et), h_eh = b.i32(t.eh), h_vo = b.i32(t.vert_off),
             h_vr = b.i32(t.vrow), h_co = b.i32(t.csr_off), h_ce = b.i32(t.csr_ent);
  if (int rc = upload_table(c, b, &c->d_perim)) return rc;
  PerimeterArgs& a = c->perim;
  a.n_loops = n_loops;
  a.target = b.at(c->d_perim, h_tg);
  a.res = b.at(c->d_perim, h_res);
  a.ent = b.at(c->d_perim, h_ent);
  a.gv = b.at(c->d_perim, h_gv);
  a.max_ent = t.max_ent;
  a.max_verts = t.max_verts;
  a.loop_off = b.at(c->d_perim, h_lo);
  a.tail = b.at(c->d_perim, h_et);
  a.head = b.at(c->d_perim, h_eh);
  a.vert_off = b.at(c->d_perim, h_vo);
  a.vrow = b.at(c->d_perim, h_vr);
  a.csr_off = b.at(c->d_perim, h_co);
  a.csr_ent = b.at(c->d_perim, h_ce);
  return MS_OK;
}

int ms_project_perimeter(ms_ctx* c, double tol, int max_iter, int32_t* passes, double* perimeter) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_project_perimeter: perimeter is not sharded (single GPU only)");
  if (!perimeter_set(c)) return fail(c, MS_ERR_STATE, "ms_project_perimeter: no loops (ms_set_perimeter)");
  if (int rc = perimeter_run(c, tol, max_iter)) return rc;
  if (!passes && !perimeter) return MS_OK;  // (nothing comes back: no copy, no synchronise)
  std::vector<double> res(2 * (size_t)c->perim.n_loops);
  HIPCHK(c, hipMemcpyAsync(res.data(), c->perim.res, sizeof(double) * res.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int l = 0; l < c->perim.n_loops; ++l) {
    if (passes) passes[l] = (int32_t)res[2 * (size_t)l];
    if (perimeter) perimeter[l] = res[2 * (size_t)l + 1];
  }
  return MS_OK;
}

int ms_get_padded_rows(ms_ctx* c, int64_t* n_rows, double* rows) {
  if (!c || !n_rows) return MS_ERR_INVALID;
  const int64_t n = c->til.nvp - c->til.nv;
  *n_rows = n;
  if (!rows || n <= 0) return MS_OK;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(rows, c->buf[MS_BUF_X] + 3 * (size_t)c->til.nv, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_enforce_only_stats(ms_ctx* c, int64_t stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->enforce_only_launches[0];
  stats[1] = c->enforce_only_launches[1];
  stats[2] = c->enforce_only_trials;
  stats[3] = perimeter_set(c) ? c->perim.n_loops : 0;
  return MS_OK;
}

}  // extern "C"
