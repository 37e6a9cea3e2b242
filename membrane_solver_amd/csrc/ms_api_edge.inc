// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): the edge lane --
// line_tension and edge_length_penalty.  Each term has its tables (ms_set_line_tension, ms_set_edge_length_penalty), an
// energy kernel behind the energy pass and a gradient kernel behind the gradient pass; everything but the term's
// arithmetic (ms_edge.hip) and its column is shared.  No kernel of the lane is recorded by the one-tile interpreter:
// each flushes it first.
namespace {

// the terms in launch order (declared in ms_api_phases.inc); kEdgeTerms[t] goes with c->edge[t] and with EDGE_LINE / EDGE_PEN
constexpr EdgeTerm kEdgeTerms[2] = {
    {MS_MOD_LINE_TENSION, "line_tension", "ms_set_line_tension", false,
     {"ms_set_line_tension: edge row out of range", "ms_set_line_tension: gamma must be finite", "",
      "ms_set_line_tension: row permutation out of range"}},
    {MS_MOD_EDGE_LENGTH_PENALTY, "edge_length_penalty", "ms_set_edge_length_penalty", true,
     {"ms_set_edge_length_penalty: edge row out of range", "ms_set_edge_length_penalty: edge_stiffness must be finite",
      "ms_set_edge_length_penalty: target_length must be finite", "ms_set_edge_length_penalty: row permutation out of range"}}};
static_assert(EDGE_LINE == 0 && EDGE_PEN == 1, "kEdgeTerms is indexed by the kernels' term");
std::string edge_not_sharded(const EdgeTerm& t) { return std::string("the ") + t.name + " module is not sharded (single GPU only)"; }

// HIP events around a launch while profiling is on (ms_line_stats, ms_edge_penalty_stats)
struct EdgeProf {
  ms_ctx* c;
  std::vector<std::pair<hipEvent_t, hipEvent_t>>& sink;
  hipEvent_t a = nullptr, b = nullptr;
  EdgeProf(ms_ctx* ctx, std::vector<std::pair<hipEvent_t, hipEvent_t>>& into) : c(ctx), sink(into) {
    if (!c->profiling) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    (void)hipEventRecord(a, c->stream);
  }
  ~EdgeProf() {
    if (!a || !b) return;
    (void)hipEventRecord(b, c->stream);
    sink.push_back({a, b});
  }
};

// the tables of an edge term's two kernels from external rows: the edge table (first column != 0 only, ascending edge
// order) and the vertex -> edge CSR over the touched rows (ascending; each row's edges in ascending edge order, with the
// other end and the column), every row in the library's order (iperm: external -> library).  A second column (l0;
// nullptr without one) is carried to both tables.  Returns nullptr, or what is wrong with the input (one of msg's texts).
struct EdgeTables {
  std::vector<int32_t> et, eh, vrow, off, other;
  std::vector<double> eg, og;    // first column: per edge, per CSR entry
  std::vector<double> el0, ol0;  // second column (empty without one)
};
const char* build_edge_tables(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                              const double* gamma, const double* l0, const EdgeTableMsgs& msg, EdgeTables& t) {
  // validate every index the kernels use, drop gamma == 0 (line_tension.py:123-124)
  for (int e = 0; e < n_edges; ++e) {
    if (tail[e] < 0 || tail[e] >= nv || head[e] < 0 || head[e] >= nv) return msg.row;
    if (!std::isfinite(gamma[e])) return msg.first;
    if (l0 && !std::isfinite(l0[e])) return msg.second;
    if (gamma[e] == 0.0) continue;
    const int32_t a = iperm[tail[e]], b = iperm[head[e]];
    if (a < 0 || a >= nv || b < 0 || b >= nv) return msg.perm;
    t.et.push_back(a);
    t.eh.push_back(b);
    t.eg.push_back(gamma[e]);
    if (l0) t.el0.push_back(l0[e]);
  }
  const int ne = (int)t.et.size();
  std::vector<int32_t> cnt(ne > 0 ? nv : 0, 0);
  for (int e = 0; e < ne; ++e) {
    ++cnt[t.et[e]];
    ++cnt[t.eh[e]];
  }
  std::vector<int32_t> slot(cnt.size(), -1);
  t.off.assign(1, 0);
  for (int v = 0; v < (int)cnt.size(); ++v)
    if (cnt[v]) {
      slot[v] = (int32_t)t.vrow.size();
      t.vrow.push_back(v);
      t.off.push_back(t.off.back() + cnt[v]);
    }
  t.other.assign(2 * (size_t)ne, 0);
  t.og.assign(2 * (size_t)ne, 0.0);
  if (l0) t.ol0.assign(2 * (size_t)ne, 0.0);
  std::vector<int32_t> fill(t.off.begin(), t.off.end() - 1);
  for (int e = 0; e < ne; ++e) {
    const int32_t ends[2][2] = {{t.et[e], t.eh[e]}, {t.eh[e], t.et[e]}};
    for (const auto& p : ends) {
      const int32_t k = fill[slot[p[0]]]++;
      t.other[k] = p[1];
      t.og[k] = t.eg[e];
      if (l0) t.ol0[k] = t.el0[e];
    }
  }
  return nullptr;
}

// the tables on the device, one allocation (ms_table_blob.h): the term's column per edge (ecol) and per CSR entry (ccol),
// the energy kernel's workgroup sums, the module's energy, the arrival counter's cell; the int tables.  The lane's two
// argument records point into it.
int upload_edge_tables(ms_ctx* c, const char* who, const EdgeTables& tb, const std::vector<double>& ecol,
                       const std::vector<double>& ccol, ms_ctx::EdgeLane& l) {
  const int tiles = c->tile1 - c->tile0;
  const int ne = (int)tb.et.size(), nt = (int)tb.vrow.size();
  if (ne > 0 && tiles <= 0) return fail(c, MS_ERR_STATE, std::string(who) + ": the context has no tiles");
  const int grid_e = ne > 0 ? std::min(tiles, (ne + 255) / 256) : 0;
  const int grid_g = nt > 0 ? std::min(tiles, (nt + 255) / 256) : 0;
  TableBlob b;
  const auto h_ecol = b.f64((size_t)ne, ecol.data()), h_ccol = b.f64(2 * (size_t)ne, ccol.data());
  const auto h_wg = b.f64((size_t)std::max(1, grid_e)), h_en = b.f64(1), h_done = b.f64(1);
  const auto h_t = b.i32(tb.et), h_h = b.i32(tb.eh), h_v = b.i32(tb.vrow), h_o = b.i32(tb.off), h_x = b.i32(tb.other);
  if (int rc = upload_table(c, b, &l.d_blob)) return rc;
  l.en.n_edges = ne;
  l.en.grid = grid_e;
  l.en.col = b.at(l.d_blob, h_ecol);
  l.en.wg_sums = b.at(l.d_blob, h_wg);
  l.en.energy = b.at(l.d_blob, h_en);
  l.en.done = b.u32(l.d_blob, h_done);
  l.en.tail = b.at(l.d_blob, h_t);
  l.en.head = b.at(l.d_blob, h_h);
  l.gr.n_touch = nt;
  l.gr.grid = grid_g;
  l.gr.vrow = b.at(l.d_blob, h_v);
  l.gr.off = b.at(l.d_blob, h_o);
  l.gr.other = b.at(l.d_blob, h_x);
  l.gr.col = b.at(l.d_blob, h_ccol);
  return MS_OK;
}

// a term's tables from its setter's arguments.  line_tension's column is gamma, the first one; edge_length_penalty hands
// its stiffness as every edge's first column -- so k == 0 charges nothing, by the rule that drops gamma == 0 -- and the
// target lengths as the second
const char* build_term_tables(int term, int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                              const double* col, double k, EdgeTables& t) {
  const EdgeTerm& T = kEdgeTerms[term];
  if (!T.second) return build_edge_tables(nv, iperm, n_edges, tail, head, col, nullptr, T.msgs, t);
  if (!std::isfinite(k)) return T.msgs.first;
  const std::vector<double> kcol((size_t)std::max(n_edges, 0), k);
  return build_edge_tables(nv, iperm, n_edges, tail, head, kcol.data(), col, T.msgs, t);
}

// the term's energy of its edges at x (or at x + alpha d) into the MS_S_ESURF partials of the energy pass just launched
int edge_energy_run(ms_ctx* c, int term, bool use_dir, double alpha) {
  ms_ctx::EdgeLane& l = c->edge[term];
  if (!l.set || l.en.n_edges == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  EdgeEnergyArgs a = l.en;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  {
    EdgeProf ep(c, l.prof[0]);
    HIPCHK(c, launch_edge_energy(term, a, c->stream));
  }
  ++l.launches[0];
  return MS_OK;
}

// the term's rows added into g (the gradient pass has just written it), <g,gC> partials corrected with the volume row
int edge_grad_run(ms_ctx* c, int term, double* g, bool volrow) {
  ms_ctx::EdgeLane& l = c->edge[term];
  if (!l.set || l.gr.n_touch == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  EdgeGradArgs a = l.gr;
  a.x = c->buf[MS_BUF_X];
  a.g = g;
  a.gc = volrow ? c->buf[MS_BUF_GC] : nullptr;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  {
    EdgeProf ep(c, l.prof[1]);
    HIPCHK(c, launch_edge_grad(term, a, c->stream));
  }
  ++l.launches[1];
  c->carry.maxg2_valid = false;  // (whatever max|g_i|^2 was reduced before predates these rows)
  return MS_OK;
}

// the setters: col is gamma / the target lengths; tail == nullptr clears the term's tables
int edge_lane_set(ms_ctx* c, int term, int n_edges, const int32_t* tail, const int32_t* head, const double* col, double k) {
  const EdgeTerm& T = kEdgeTerms[term];
  ms_ctx::EdgeLane& l = c->edge[term];
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, std::string(T.setter) + ": " + edge_not_sharded(T));
  if (int rc = drop_table(c, l.d_blob)) return rc;
  l.en = EdgeEnergyArgs{};
  l.gr = EdgeGradArgs{};
  l.set = false;
  c->carry.invalidate();  // (energies and G held are the old term's)
  if (!tail) return MS_OK;
  if (n_edges < 0 || !head || !col) return fail(c, MS_ERR_INVALID, std::string(T.setter) + ": bad argument");
  EdgeTables tb;
  if (const char* why = build_term_tables(term, c->til.nv, c->til.iperm.data(), n_edges, tail, head, col, k, tb))
    return fail(c, MS_ERR_INVALID, why);
  if (int rc = upload_edge_tables(c, T.setter, tb, T.second ? tb.el0 : tb.eg, T.second ? tb.ol0 : tb.og, l)) return rc;
  l.en.k = l.gr.k = k;
  l.set = true;
  return MS_OK;
}

// the tables as the setter would build them, into the caller's arrays (the *_tables_host entry points)
int edge_tables_out(int term, int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                    const double* col, double k, int32_t counts[2], int32_t* e_tail, int32_t* e_head, double* e_col,
                    int32_t* vrow, int32_t* off, int32_t* other, double* csr_col) {
  EdgeTables t;
  if (const char* why = build_term_tables(term, nv, iperm, n_edges, tail, head, col, k, t)) return fail(nullptr, MS_ERR_INVALID, why);
  const bool second = kEdgeTerms[term].second;
  const std::vector<double>&ecol = second ? t.el0 : t.eg, &ccol = second ? t.ol0 : t.og;
  counts[0] = (int32_t)t.et.size();
  counts[1] = (int32_t)t.vrow.size();
  std::copy(t.et.begin(), t.et.end(), e_tail);
  std::copy(t.eh.begin(), t.eh.end(), e_head);
  std::copy(ecol.begin(), ecol.end(), e_col);
  std::copy(t.vrow.begin(), t.vrow.end(), vrow);
  std::copy(t.off.begin(), t.off.end(), off);
  std::copy(t.other.begin(), t.other.end(), other);
  std::copy(ccol.begin(), ccol.end(), csr_col);
  return MS_OK;
}

// the term's own energy as the last energy pass summed it
int edge_lane_energy(ms_ctx* c, int term, double* energy) {
  const ms_ctx::EdgeLane& l = c->edge[term];
  *energy = 0.0;
  if (!l.set || l.en.n_edges == 0) return MS_OK;  // (0.0 as uploaded until the first energy pass)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, l.en.energy, sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

// {energy launches, gradient launches, their summed event microseconds}; reading resets the event brackets
int edge_lane_stats(ms_ctx* c, int term, double stats[4]) {
  ms_ctx::EdgeLane& l = c->edge[term];
  HIPCHK(c, hipStreamSynchronize(S(c)));
  for (int w = 0; w < 2; ++w) {
    stats[w] = (double)l.launches[w];
    double us = 0.0;
    for (auto& ev : l.prof[w]) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) us += 1e3 * (double)ms;
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    l.prof[w].clear();
    stats[2 + w] = us;
  }
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_line_tension(ms_ctx* c, int n_edges, const int32_t* tail, const int32_t* head, const double* gamma) {
  if (!c) return MS_ERR_INVALID;
  return edge_lane_set(c, EDGE_LINE, n_edges, tail, head, gamma, 0.0);
}

int ms_line_tables_host(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                        const double* gamma, int32_t counts[2], int32_t* e_tail, int32_t* e_head, double* e_gamma,
                        int32_t* vrow, int32_t* off, int32_t* other, double* csr_gamma) {
  if (nv < 0 || n_edges < 0 || !iperm || !tail || !head || !gamma || !counts || !e_tail || !e_head || !e_gamma || !vrow ||
      !off || !other || !csr_gamma)
    return fail(nullptr, MS_ERR_INVALID, "ms_line_tables_host: bad argument");
  return edge_tables_out(EDGE_LINE, nv, iperm, n_edges, tail, head, gamma, 0.0, counts, e_tail, e_head, e_gamma, vrow, off,
                         other, csr_gamma);
}

int ms_get_line_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_line_energy: NULL argument");
  return edge_lane_energy(c, EDGE_LINE, energy);
}

int ms_line_stats(ms_ctx* c, double stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  return edge_lane_stats(c, EDGE_LINE, stats);
}

int ms_set_edge_length_penalty(ms_ctx* c, int n_edges, const int32_t* tail, const int32_t* head, const double* target_length,
                               double k) {
  if (!c) return MS_ERR_INVALID;
  return edge_lane_set(c, EDGE_PEN, n_edges, tail, head, target_length, k);
}

int ms_edge_penalty_tables_host(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                                const double* target_length, double k, int32_t counts[2], int32_t* e_tail, int32_t* e_head,
                                double* e_l0, int32_t* vrow, int32_t* off, int32_t* other, double* csr_l0) {
  if (nv < 0 || n_edges < 0 || !iperm || !tail || !head || !target_length || !counts || !e_tail || !e_head || !e_l0 ||
      !vrow || !off || !other || !csr_l0)
    return fail(nullptr, MS_ERR_INVALID, "ms_edge_penalty_tables_host: bad argument");
  return edge_tables_out(EDGE_PEN, nv, iperm, n_edges, tail, head, target_length, k, counts, e_tail, e_head, e_l0, vrow,
                         off, other, csr_l0);
}

int ms_get_edge_penalty_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_edge_penalty_energy: NULL argument");
  return edge_lane_energy(c, EDGE_PEN, energy);
}

int ms_edge_penalty_stats(ms_ctx* c, double stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  return edge_lane_stats(c, EDGE_PEN, stats);
}

}  // extern "C"
