// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): line_tension --
// the tables (ms_set_line_tension), k_line_energy behind the energy pass and k_line_grad behind the gradient pass.
// Neither kernel is recorded by the one-tile interpreter: both flush it first.
namespace {

// HIP events around a launch while profiling is on (ms_line_stats, ms_edge_penalty_stats)
struct LineProf {
  ms_ctx* c;
  std::vector<std::pair<hipEvent_t, hipEvent_t>>& sink;
  hipEvent_t a = nullptr, b = nullptr;
  LineProf(ms_ctx* ctx, std::vector<std::pair<hipEvent_t, hipEvent_t>>& into) : c(ctx), sink(into) {
    if (!c->profiling) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    (void)hipEventRecord(a, c->stream);
  }
  ~LineProf() {
    if (!a || !b) return;
    (void)hipEventRecord(b, c->stream);
    sink.push_back({a, b});
  }
};

// the tables of an edge module's two kernels from external rows: the edge table (first column != 0 only, ascending edge
// order) and the vertex -> edge CSR over the touched rows (ascending; each row's edges in ascending edge order, with the
// other end and the column), every row in the library's order (iperm: external -> library).  line_tension's column is
// gamma; edge_length_penalty (ms_api_edgepen.inc) hands its stiffness as the first column -- so k == 0 charges nothing,
// by the rule that drops gamma == 0 -- and the target lengths as a second one (l0; nullptr for line_tension), which is
// carried to both tables.  Returns nullptr, or what is wrong with the input (one of msg's texts).
struct LineTables {
  std::vector<int32_t> et, eh, vrow, off, other;
  std::vector<double> eg, og;    // first column: per edge, per CSR entry
  std::vector<double> el0, ol0;  // second column (empty without one)
};
struct LineTableMsgs {
  const char *row, *first, *second, *perm;
};
constexpr LineTableMsgs kLineMsgs = {"ms_set_line_tension: edge row out of range", "ms_set_line_tension: gamma must be finite",
                                     "", "ms_set_line_tension: row permutation out of range"};
const char* build_line_tables(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                              const double* gamma, const double* l0, const LineTableMsgs& msg, LineTables& t) {
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

// the tables on the device, one allocation: doubles first (the per-edge column, the CSR column, the energy kernel's
// workgroup sums, the module's energy, the arrival counter's cell), then the int tables
struct EdgeBlob {
  int ne = 0, nt = 0, grid_e = 0, grid_g = 0;
  const double *ecol = nullptr, *ccol = nullptr;
  double *wg_sums = nullptr, *energy = nullptr;
  uint32_t* done = nullptr;
  const int32_t *tail = nullptr, *head = nullptr, *vrow = nullptr, *off = nullptr, *other = nullptr;
};
int upload_edge_tables(ms_ctx* c, const char* who, const LineTables& tb, const std::vector<double>& ecol,
                       const std::vector<double>& ccol, void** d_blob, EdgeBlob& out) {
  const int tiles = c->tile1 - c->tile0;
  const int ne = (int)tb.et.size(), nt = (int)tb.vrow.size();
  if (ne > 0 && tiles <= 0) return fail(c, MS_ERR_STATE, std::string(who) + ": the context has no tiles");
  const int grid_e = ne > 0 ? std::min(tiles, (ne + 255) / 256) : 0;
  const int grid_g = nt > 0 ? std::min(tiles, (nt + 255) / 256) : 0;
  const size_t n_dbl = (size_t)ne + 2 * (size_t)ne + (size_t)std::max(1, grid_e) + 2;
  const size_t n_int = 2 * (size_t)ne + (size_t)nt + (size_t)nt + 1 + 2 * (size_t)ne;
  std::vector<double> blob(n_dbl + (n_int + 1) / 2 + 1, 0.0);
  double* bp = blob.data();
  if (ne) {
    memcpy(bp, ecol.data(), sizeof(double) * ne);
    memcpy(bp + ne, ccol.data(), sizeof(double) * 2 * (size_t)ne);
  }
  int32_t* ip = reinterpret_cast<int32_t*>(bp + n_dbl);
  size_t at = 0;
  auto put = [&](const std::vector<int32_t>& v) {
    const size_t o = at;
    if (!v.empty()) memcpy(ip + at, v.data(), sizeof(int32_t) * v.size());
    at += v.size();
    return o;
  };
  const size_t o_t = put(tb.et), o_h = put(tb.eh), o_v = put(tb.vrow), o_o = put(tb.off), o_x = put(tb.other);
  HIPCHK(c, hipMalloc(d_blob, blob.size() * sizeof(double)));
  HIPCHK(c, hipMemcpy(*d_blob, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  double* dp = static_cast<double*>(*d_blob);
  const int32_t* di = reinterpret_cast<const int32_t*>(dp + n_dbl);
  out.ne = ne;
  out.nt = nt;
  out.grid_e = grid_e;
  out.grid_g = grid_g;
  out.ecol = dp;
  out.ccol = dp + ne;
  out.wg_sums = dp + 3 * (size_t)ne;
  out.energy = out.wg_sums + std::max(1, grid_e);
  out.done = reinterpret_cast<uint32_t*>(out.energy + 1);
  out.tail = di + o_t;
  out.head = di + o_h;
  out.vrow = di + o_v;
  out.off = di + o_o;
  out.other = di + o_x;
  return MS_OK;
}

// gamma |e| of the tagged edges at x (or at x + alpha d) into the MS_S_ESURF partials of the energy pass just launched
int line_energy_run(ms_ctx* c, bool use_dir, double alpha) {
  if (!c->line_set || c->line_en.n_edges == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  LineEnergyArgs a = c->line_en;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  {
    LineProf lp(c, c->line_prof[0]);
    HIPCHK(c, launch_line_energy(a, c->stream));
  }
  ++c->line_launches[0];
  return MS_OK;
}

// the module's rows added into g (the gradient pass has just written it), <g,gC> partials corrected with the volume row
int line_grad_run(ms_ctx* c, double* g, bool volrow) {
  if (!c->line_set || c->line_gr.n_touch == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  LineGradArgs a = c->line_gr;
  a.x = c->buf[MS_BUF_X];
  a.g = g;
  a.gc = volrow ? c->buf[MS_BUF_GC] : nullptr;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  {
    LineProf lp(c, c->line_prof[1]);
    HIPCHK(c, launch_line_grad(a, c->stream));
  }
  ++c->line_launches[1];
  c->carry.maxg2_valid = false;  // (whatever max|g_i|^2 was reduced before predates these rows)
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_line_tension(ms_ctx* c, int n_edges, const int32_t* tail, const int32_t* head, const double* gamma) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_set_line_tension: the line_tension module is not sharded (single GPU only)");
  if (c->d_line) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    HIPCHK(c, hipFree(c->d_line));
    c->d_line = nullptr;
  }
  c->line_en = LineEnergyArgs{};
  c->line_gr = LineGradArgs{};
  c->line_set = false;
  c->carry.carry_valid = c->carry.grad_valid = c->carry.maxg2_valid = false;  // (energies and G held are the old term's)
  if (!tail) return MS_OK;
  if (n_edges < 0 || !head || !gamma) return fail(c, MS_ERR_INVALID, "ms_set_line_tension: bad argument");
  LineTables tb;
  if (const char* why = build_line_tables(c->til.nv, c->til.iperm.data(), n_edges, tail, head, gamma, nullptr, kLineMsgs, tb))
    return fail(c, MS_ERR_INVALID, why);
  EdgeBlob bl;
  if (int rc = upload_edge_tables(c, "ms_set_line_tension", tb, tb.eg, tb.og, &c->d_line, bl)) return rc;
  LineEnergyArgs& en = c->line_en;
  en.n_edges = bl.ne;
  en.gamma = bl.ecol;
  en.wg_sums = bl.wg_sums;
  en.energy = bl.energy;
  en.done = bl.done;
  en.tail = bl.tail;
  en.head = bl.head;
  en.grid = bl.grid_e;
  LineGradArgs& gr = c->line_gr;
  gr.n_touch = bl.nt;
  gr.vrow = bl.vrow;
  gr.off = bl.off;
  gr.other = bl.other;
  gr.gamma = bl.ccol;
  gr.grid = bl.grid_g;
  c->line_set = true;
  return MS_OK;
}

int ms_line_tables_host(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                        const double* gamma, int32_t counts[2], int32_t* e_tail, int32_t* e_head, double* e_gamma,
                        int32_t* vrow, int32_t* off, int32_t* other, double* csr_gamma) {
  if (nv < 0 || n_edges < 0 || !iperm || !tail || !head || !gamma || !counts || !e_tail || !e_head || !e_gamma || !vrow ||
      !off || !other || !csr_gamma)
    return fail(nullptr, MS_ERR_INVALID, "ms_line_tables_host: bad argument");
  LineTables t;
  if (const char* why = build_line_tables(nv, iperm, n_edges, tail, head, gamma, nullptr, kLineMsgs, t)) return fail(nullptr, MS_ERR_INVALID, why);
  counts[0] = (int32_t)t.et.size();
  counts[1] = (int32_t)t.vrow.size();
  std::copy(t.et.begin(), t.et.end(), e_tail);
  std::copy(t.eh.begin(), t.eh.end(), e_head);
  std::copy(t.eg.begin(), t.eg.end(), e_gamma);
  std::copy(t.vrow.begin(), t.vrow.end(), vrow);
  std::copy(t.off.begin(), t.off.end(), off);
  std::copy(t.other.begin(), t.other.end(), other);
  std::copy(t.og.begin(), t.og.end(), csr_gamma);
  return MS_OK;
}

int ms_get_line_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_line_energy: NULL argument");
  *energy = 0.0;
  if (!c->line_set || c->line_en.n_edges == 0) return MS_OK;  // (0.0 as uploaded until the first energy pass)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, c->line_en.energy, sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_line_stats(ms_ctx* c, double stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  for (int w = 0; w < 2; ++w) {
    stats[w] = (double)c->line_launches[w];
    double us = 0.0;
    for (auto& ev : c->line_prof[w]) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) us += 1e3 * (double)ms;
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    c->line_prof[w].clear();
    stats[2 + w] = us;
  }
  return MS_OK;
}

}  // extern "C"
