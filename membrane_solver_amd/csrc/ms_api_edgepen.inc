// libmembrane_hip.so host side, part of ms_api.cpp (included there, behind ms_api_line.inc, whose table builder, upload and
// event brackets it shares): edge_length_penalty -- the tables (ms_set_edge_length_penalty), k_edgepen_energy behind the
// energy pass and k_edgepen_grad behind the gradient pass.  Neither kernel is recorded by the one-tile interpreter: both
// flush it first.
namespace {

constexpr LineTableMsgs kEdgePenMsgs = {"ms_set_edge_length_penalty: edge row out of range",
                                        "ms_set_edge_length_penalty: edge_stiffness must be finite",
                                        "ms_set_edge_length_penalty: target_length must be finite",
                                        "ms_set_edge_length_penalty: row permutation out of range"};

// the shared builder with the stiffness as every edge's first column (k == 0 keeps no edge) and L0 as the second
const char* build_edgepen_tables(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                                 const double* target_length, double k, LineTables& t) {
  if (!std::isfinite(k)) return kEdgePenMsgs.first;
  const std::vector<double> kcol((size_t)std::max(n_edges, 0), k);
  return build_line_tables(nv, iperm, n_edges, tail, head, kcol.data(), target_length, kEdgePenMsgs, t);
}

// 0.5 k (|e| - L0)^2 of the charged edges at x (or at x + alpha d) into the MS_S_ESURF partials of the energy pass just
// launched
int edgepen_energy_run(ms_ctx* c, bool use_dir, double alpha) {
  if (!c->edgepen_set || c->edgepen_en.n_edges == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  EdgePenEnergyArgs a = c->edgepen_en;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  {
    LineProf lp(c, c->edgepen_prof[0]);
    HIPCHK(c, launch_edgepen_energy(a, c->stream));
  }
  ++c->edgepen_launches[0];
  return MS_OK;
}

// the module's rows added into g (behind the gradient pass and k_line_grad), <g,gC> partials corrected with the volume row
int edgepen_grad_run(ms_ctx* c, double* g, bool volrow) {
  if (!c->edgepen_set || c->edgepen_gr.n_touch == 0) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  EdgePenGradArgs a = c->edgepen_gr;
  a.x = c->buf[MS_BUF_X];
  a.g = g;
  a.gc = volrow ? c->buf[MS_BUF_GC] : nullptr;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  {
    LineProf lp(c, c->edgepen_prof[1]);
    HIPCHK(c, launch_edgepen_grad(a, c->stream));
  }
  ++c->edgepen_launches[1];
  c->carry.maxg2_valid = false;  // (whatever max|g_i|^2 was reduced before predates these rows)
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_edge_length_penalty(ms_ctx* c, int n_edges, const int32_t* tail, const int32_t* head, const double* target_length,
                               double k) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_edge_length_penalty: the edge_length_penalty module is not sharded (single GPU only)");
  if (c->d_edgepen) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    HIPCHK(c, hipFree(c->d_edgepen));
    c->d_edgepen = nullptr;
  }
  c->edgepen_en = EdgePenEnergyArgs{};
  c->edgepen_gr = EdgePenGradArgs{};
  c->edgepen_set = false;
  c->carry.carry_valid = c->carry.grad_valid = c->carry.maxg2_valid = false;  // (energies and G held are the old term's)
  if (!tail) return MS_OK;
  if (n_edges < 0 || !head || !target_length) return fail(c, MS_ERR_INVALID, "ms_set_edge_length_penalty: bad argument");
  LineTables tb;
  if (const char* why = build_edgepen_tables(c->til.nv, c->til.iperm.data(), n_edges, tail, head, target_length, k, tb))
    return fail(c, MS_ERR_INVALID, why);
  EdgeBlob bl;
  if (int rc = upload_edge_tables(c, "ms_set_edge_length_penalty", tb, tb.el0, tb.ol0, &c->d_edgepen, bl)) return rc;
  EdgePenEnergyArgs& en = c->edgepen_en;
  en.k = k;
  en.n_edges = bl.ne;
  en.l0 = bl.ecol;
  en.wg_sums = bl.wg_sums;
  en.energy = bl.energy;
  en.done = bl.done;
  en.tail = bl.tail;
  en.head = bl.head;
  en.grid = bl.grid_e;
  EdgePenGradArgs& gr = c->edgepen_gr;
  gr.k = k;
  gr.n_touch = bl.nt;
  gr.vrow = bl.vrow;
  gr.off = bl.off;
  gr.other = bl.other;
  gr.l0 = bl.ccol;
  gr.grid = bl.grid_g;
  c->edgepen_set = true;
  return MS_OK;
}

int ms_edge_penalty_tables_host(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                                const double* target_length, double k, int32_t counts[2], int32_t* e_tail, int32_t* e_head,
                                double* e_l0, int32_t* vrow, int32_t* off, int32_t* other, double* csr_l0) {
  if (nv < 0 || n_edges < 0 || !iperm || !tail || !head || !target_length || !counts || !e_tail || !e_head || !e_l0 ||
      !vrow || !off || !other || !csr_l0)
    return fail(nullptr, MS_ERR_INVALID, "ms_edge_penalty_tables_host: bad argument");
  LineTables t;
  if (const char* why = build_edgepen_tables(nv, iperm, n_edges, tail, head, target_length, k, t))
    return fail(nullptr, MS_ERR_INVALID, why);
  counts[0] = (int32_t)t.et.size();
  counts[1] = (int32_t)t.vrow.size();
  std::copy(t.et.begin(), t.et.end(), e_tail);
  std::copy(t.eh.begin(), t.eh.end(), e_head);
  std::copy(t.el0.begin(), t.el0.end(), e_l0);
  std::copy(t.vrow.begin(), t.vrow.end(), vrow);
  std::copy(t.off.begin(), t.off.end(), off);
  std::copy(t.other.begin(), t.other.end(), other);
  std::copy(t.ol0.begin(), t.ol0.end(), csr_l0);
  return MS_OK;
}

int ms_get_edge_penalty_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_edge_penalty_energy: NULL argument");
  *energy = 0.0;
  if (!c->edgepen_set || c->edgepen_en.n_edges == 0) return MS_OK;  // (0.0 as uploaded until the first energy pass)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, c->edgepen_en.energy, sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_edge_penalty_stats(ms_ctx* c, double stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  for (int w = 0; w < 2; ++w) {
    stats[w] = (double)c->edgepen_launches[w];
    double us = 0.0;
    for (auto& ev : c->edgepen_prof[w]) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) us += 1e3 * (double)ms;
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    c->edgepen_prof[w].clear();
    stats[2 + w] = us;
  }
  return MS_OK;
}

}  // extern "C"
