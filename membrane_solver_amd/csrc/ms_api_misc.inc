// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): state rebinding, statistics, profiling, the tiling planner, the kernel-provider seam.
size_t ms_state_bytes(const ms_ctx* c) {
  if (!c) return 0;
  return sizeof(double) * (8 * 3 * (size_t)c->til.nvp + 2 * (size_t)c->til.nvp);
}

int ms_rebind_state(ms_ctx* c, void* device_base, size_t bytes) {
  if (!c || !device_base) return fail(c, MS_ERR_INVALID, "ms_rebind_state: NULL argument");
  const size_t need = ms_state_bytes(c);
  if (bytes < need) return fail(c, MS_ERR_INVALID, "ms_rebind_state: buffer smaller than ms_state_bytes");
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(device_base, c->state, need, hipMemcpyDeviceToDevice));
  double* nb = static_cast<double*>(device_base);
  for (int b = 0; b <= MS_BUF_FA; ++b) c->buf[b] = nb + (c->buf[b] - c->state);
  c->carry.last_g = nb + (c->carry.last_g - c->state);
  if (c->own_state) HIPCHK(c, hipFree(c->state));
  c->state = nb;
  c->own_state = false;
  return MS_OK;
}

int ms_fetch_scalars(ms_ctx* c, double* out) {
  if (!c || !out) return MS_ERR_INVALID;
  int rc = fetch(c);
  if (rc) return rc;
  memcpy(out, c->h_scal, sizeof(double) * MS_NSCAL);
  return MS_OK;
}

int ms_store_scalars(ms_ctx* c, const double* in) {
  if (!c || !in) return MS_ERR_INVALID;
  for (int sl = 0; sl < MS_NSCAL; ++sl) put_mailbox(c, sl, in[sl]);
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  HIPCHK(c, hipMemcpyAsync(c->d_scal, c->h_scal, sizeof(double) * MS_NSCAL, hipMemcpyHostToDevice,
                           S(c)));
  HIPCHK(c, hipStreamSynchronize(S(c)));
  return MS_OK;
}

int ms_device_buffer(ms_ctx* c, int buffer, void** dev_ptr, size_t* bytes) {
  if (c) (void)exec_flush(c);  // (the caller may read the buffer on its own stream: nothing stays recorded)
  if (!c || !dev_ptr || buffer < 0 || buffer >= MS_BUF_COUNT) return MS_ERR_INVALID;
  *dev_ptr = c->buf[buffer];
  if (bytes) {
    if (buffer == MS_BUF_SCAL)
      *bytes = sizeof(double) * MS_NSCAL;
    else
      *bytes = sizeof(double) * (size_t)c->til.nvp * (buffer == MS_BUF_FA ? 2 : 3);
  }
  return MS_OK;
}

int ms_shard_info(ms_ctx* c, int64_t* nvp, int64_t* row0, int64_t* row1, int64_t* rows_per_shard) {
  if (!c) return MS_ERR_INVALID;
  const Tiling& t = c->til;
  if (nvp) *nvp = t.nvp;
  if (rows_per_shard) *rows_per_shard = (int64_t)t.tiles_per_shard * t.own;
  if (row0) *row0 = (int64_t)c->shard_rank * t.tiles_per_shard * t.own;
  if (row1) *row1 = (int64_t)(c->shard_rank + 1) * t.tiles_per_shard * t.own;
  return MS_OK;
}

int ms_tile_stats(ms_ctx* c, int64_t* n_tiles, int64_t* facet_instances, int64_t* max_halo,
                  int64_t* lds_bytes_energy, int64_t* lds_bytes_gradient) {
  if (!c) return MS_ERR_INVALID;
  const Tiling& t = c->til;
  const bool bend = (c->params.modules & MS_MOD_BENDING) != 0;
  if (n_tiles) *n_tiles = t.n_tiles;
  if (facet_instances) *facet_instances = (int64_t)t.tile_facets.size();
  if (max_halo) *max_halo = t.max_halo;
  if (lds_bytes_energy) *lds_bytes_energy = (int64_t)energy_lds_bytes(t.T, c->cap, t.max_ent, bend, false, c->has_boundary, !c->deterministic);
  if (lds_bytes_gradient)
    *lds_bytes_gradient = (int64_t)gradient_lds_bytes(t.T, c->cap, t.max_ent, bend,
                                                      (c->params.modules & MS_CON_VOLUME) != 0, !c->deterministic);
  return MS_OK;
}

int ms_queue_stats(ms_ctx* c, int64_t stats[8]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 8; ++k) stats[k] = 0;
  stats[0] = c->q_rounds;
  stats[1] = c->q_multi;
  stats[2] = c->q_wasted;
  stats[3] = c->q_side_accepts;
  stats[4] = c->queue_mismatches;
  stats[5] = c->q_ahead;
  stats[6] = c->q_adopted;
  stats[7] = c->q_dropped;
  return MS_OK;
}

int ms_search_trials(ms_ctx* c, double* rows, int max_rows, int* n_rows, int64_t first_launch_hist[8]) {
  static_assert(MS_MAX_TRIALS == 8, "ms_search_trials: the histogram has one bin per launch size");
  if (!c || !n_rows || max_rows < 0 || (max_rows > 0 && !rows)) return MS_ERR_INVALID;
  const int n = (int)c->trial_log.size();
  *n_rows = n;
  for (int k = 0; k < std::min(n, max_rows); ++k) {
    const ms_ctx::TrialRow& t = c->trial_log[(size_t)k];
    double* r = rows + (size_t)MS_TRIAL_COLS * k;
    r[0] = t.alpha;
    r[1] = t.energy;
    r[2] = t.rhs;
    r[3] = (double)t.launch;
    r[4] = (double)t.slot;
    r[5] = (double)t.flags;
  }
  if (first_launch_hist)
    for (int k = 0; k < MS_MAX_TRIALS; ++k) first_launch_hist[k] = c->first_launch_hist[k];
  return MS_OK;
}

int ms_direction_stats(ms_ctx* c, int64_t* skipped, int64_t* materialized) {
  if (!c || !skipped || !materialized) return MS_ERR_INVALID;
  *skipped = c->dir_skipped;
  *materialized = c->dir_materialized;
  return MS_OK;
}

int ms_energy_stats(ms_ctx* c, int64_t* lean, int64_t* general) {
  if (!c || !lean || !general) return MS_ERR_INVALID;
  *lean = c->ka_lean;
  *general = c->ka_general;
  return MS_OK;
}

int ms_resident_stats(ms_ctx* c, int64_t stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->resident_ok;
  stats[1] = c->resident_launches;
  stats[2] = c->resident_steps;
  stats[3] = c->resident_bails;
  return MS_OK;
}

int ms_tsearch_stats(ms_ctx* c, int64_t stats[2]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->tsearch_launches;
  stats[1] = c->tsearch_trials;
  return MS_OK;
}

namespace {
// (the functions and limits the planners decide by -- ms_internal.h -- not a second copy of them)
void tilt_lane_fill(int T, int own, int cap, int max_ent, bool volrow, bool atomic, int64_t stats[12]) {
  stats[0] = cap;
  stats[1] = max_ent;
  for (int nf = 1; nf <= 2; ++nf) {
    int64_t* s = stats + 2 + 3 * (nf - 1);
    s[0] = tsearch_fits(cap, nf, MS_MAX_TRIALS) ? 1 : 0;                          // tsearch_plan
    s[1] = (s[0] && tgrad_fits(T, cap, max_ent, nf)) ? 1 : 0;                     // tgrad_plan
    s[2] = tsearch_fits(cap, nf, 1) ? 1 : 0;                                      // tilt_energy_pass
  }
  const size_t leaf = leaflet_gradient_lds_bytes(T, cap, max_ent, volrow, atomic);
  stats[8] = (int64_t)leaf;
  stats[9] = leaf <= MS_LDS_CU ? 1 : 0;                                           // leaflet_gradient_admit
  stats[10] = T;
  stats[11] = own;
}
}  // namespace

int ms_tilt_lane_stats(ms_ctx* c, int64_t stats[12]) {
  if (!c || !stats) return MS_ERR_INVALID;
  const Tiling& t = c->til;
  tilt_lane_fill(t.T, t.own, c->cap, t.max_ent, (c->params.modules & MS_CON_VOLUME) != 0, !c->deterministic, stats);
  return MS_OK;
}

int ms_plan_tilt_lanes(int nv, int nf, const double* positions, const int32_t* tri, int tile_vertices,
                       int fixed_order, int64_t stats[12]) {
  if (!stats) return fail(nullptr, MS_ERR_INVALID, "ms_plan_tilt_lanes: stats is NULL");
  Tiling t;
  std::string err;
  int rc = build_tiling(nv, nf, positions, tri, nullptr, tile_vertices, 1, t, err);
  if (rc != MS_OK) return fail(nullptr, rc, err);
  tilt_lane_fill(t.T, t.own, t.own + t.max_halo, t.max_ent, false, fixed_order == 0, stats);
  return MS_OK;
}

int ms_tilt_lane_plan(int threads, int cap, int max_ent, int fixed_order, int64_t stats[12]) {
  if (!stats || threads < 1 || cap < 1 || max_ent < 0) return fail(nullptr, MS_ERR_INVALID, "ms_tilt_lane_plan: bad argument");
  tilt_lane_fill(threads, threads, cap, max_ent, false, fixed_order == 0, stats);
  return MS_OK;
}

int ms_exec_stats(ms_ctx* c, int64_t stats[4]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->exec_on ? 1 : 0;
  stats[1] = c->exec.launches;
  stats[2] = c->exec.cmds;
  stats[3] = (c->exec_wanted ? 1 : 0) | ((int64_t)(c->relax_programs & 0xffffff) << 8) | ((int64_t)c->relax_fused_runs << 32);
  return MS_OK;
}

// Diagnostic: how long does each record of the one-workgroup interpreter take?  on != 0 arms a device buffer that
// k_exec appends {kind, mode, instance, duration} to; reading returns, per (kind, mode) pair seen, the count and the
// total duration in microseconds -- rows of {kind, mode | inst << 16, count, total_us} -- and clears the buffer.
int ms_exec_trace(ms_ctx* c, int on, double* rows, int max_rows, int* n_rows) {
  if (!c) return MS_ERR_INVALID;
  if (n_rows) *n_rows = 0;
  int rc = exec_flush(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->exec.d_stamps && rows && max_rows > 0 && n_rows) {
    std::vector<unsigned long long> h((size_t)2 * EXEC_STAMP_CAP);
    HIPCHK(c, hipMemcpy(h.data(), c->exec.d_stamps, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    const size_t n = (size_t)std::min<unsigned long long>(h[0], (unsigned long long)EXEC_STAMP_CAP - 1);
    std::map<unsigned long long, std::pair<long, double>> acc;
    for (size_t i = 0; i < n; ++i) {
      auto& e = acc[h[1 + 2 * i]];
      e.first += 1;
      e.second += 0.01 * (double)h[2 + 2 * i];  // s_memrealtime: 100 MHz
    }
    int k = 0;
    for (auto& kv : acc) {
      if (k >= max_rows) break;
      rows[4 * k] = (double)(kv.first >> 32);
      rows[4 * k + 1] = (double)(kv.first & 0xffffffffull);
      rows[4 * k + 2] = (double)kv.second.first;
      rows[4 * k + 3] = kv.second.second;
      ++k;
    }
    *n_rows = k;
  }
  if (on && !c->exec.d_stamps)
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->exec.d_stamps), sizeof(unsigned long long) * 2 * EXEC_STAMP_CAP));
  if (c->exec.d_stamps) HIPCHK(c, hipMemset(c->exec.d_stamps, 0, sizeof(unsigned long long) * 2 * EXEC_STAMP_CAP));
  if (!on && c->exec.d_stamps) {
    (void)hipFree(c->exec.d_stamps);
    c->exec.d_stamps = nullptr;
  }
  return MS_OK;
}

int ms_profile_enable(ms_ctx* c, int on) {
  if (!c) return MS_ERR_INVALID;
  if (on && !c->d_prof_ran) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_prof_ran), sizeof(uint32_t) * ms_ctx::PROF_RAN_CAP));
    HIPCHK(c, hipMemset(c->d_prof_ran, 0, sizeof(uint32_t) * ms_ctx::PROF_RAN_CAP));
  }
  // per-kernel timing needs one launch per kernel: the one-workgroup interpreter steps aside while it is on
  if (on && c->exec_on) {
    int rc = exec_flush(c);
    if (rc) return rc;
    exec_detach(&c->exec);
    c->exec_on = false;
  } else if (!on && c->exec_wanted && !c->exec_on) {
    c->exec.stream = c->stream;
    exec_attach(&c->exec);
    c->exec_on = true;
  }
  c->profiling = on != 0;
  return MS_OK;
}

int ms_profile_read(ms_ctx* c, double total_ms[MS_PROF_KINDS], int64_t launches[MS_PROF_KINDS]) {
  if (!c || !total_ms || !launches) return MS_ERR_INVALID;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  std::vector<uint32_t> ran((size_t)c->prof_ran_next);
  if (c->prof_ran_next > 0)
    HIPCHK(c, hipMemcpy(ran.data(), c->d_prof_ran, sizeof(uint32_t) * ran.size(), hipMemcpyDeviceToHost));
  c->prof_ran_next = 0;
  for (auto& r : c->prof_pending) {
    float ms = 0.f;
    // a gated launch that found its gate closed (the probe behind it saw another code than the one it was queued for)
    // is not a sample of the kernel
    const bool empty = r.ran_idx >= 0 && ran[(size_t)r.ran_idx] == 0u;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && !empty) {
      c->prof_ms[r.kind] += ms;
      c->prof_n[r.kind] += 1;
    }
    c->prof_pool.push_back(r.a);
    c->prof_pool.push_back(r.b);
  }
  c->prof_pending.clear();
  for (int k = 0; k < MS_PROF_KINDS; ++k) {
    total_ms[k] = c->prof_ms[k];
    launches[k] = c->prof_n[k];
    c->prof_ms[k] = 0.0;
    c->prof_n[k] = 0;
  }
  return MS_OK;
}

int ms_plan_tiling(int nv, int nf, const double* positions, const int32_t* tri, int tile_vertices,
                   int shard_count, int64_t stats[8], int32_t* perm_out) {
  if (!stats) return fail(nullptr, MS_ERR_INVALID, "ms_plan_tiling: stats is NULL");
  Tiling t;
  std::string err;
  int rc = build_tiling(nv, nf, positions, tri, nullptr, tile_vertices, shard_count, t, err);
  if (rc != MS_OK) return fail(nullptr, rc, err);
  int64_t owners = 0, owned_corners = 0;
  for (int tile = 0; tile < t.n_tiles; ++tile) {
    const int n_owned = std::min(t.own, t.nv - tile * t.own);
    for (int p = t.tile_facet_off[tile]; p < t.tile_facet_off[tile + 1]; ++p) {
      const TileFacet& f = t.tile_facets[p];
      if (f.flags & TF_OWNER) ++owners;
      owned_corners += (f.l0 < n_owned) + (f.l1 < n_owned) + (f.l2 < n_owned);
    }
  }
  stats[0] = t.n_tiles;
  stats[1] = (int64_t)t.tile_facets.size();
  stats[2] = t.max_halo;
  stats[3] = t.max_tile_facets;
  stats[4] = t.dropped_facets;
  stats[5] = owners;
  stats[6] = owned_corners;
  stats[7] = (int64_t)gradient_lds_bytes(t.T, t.own + t.max_halo, t.max_ent, true, true);
  if (perm_out) memcpy(perm_out, t.perm.data(), sizeof(int32_t) * (size_t)nv);
  return MS_OK;
}

int ms_plan_tiling_conflicts(int nv, int nf, const double* positions, const int32_t* tri, int tile_vertices,
                             double model[4]) {
  if (!model) return fail(nullptr, MS_ERR_INVALID, "ms_plan_tiling_conflicts: model is NULL");
  Tiling t;
  std::string err;
  int rc = build_tiling(nv, nf, positions, tri, nullptr, tile_vertices, 1, t, err);
  if (rc != MS_OK) return fail(nullptr, rc, err);
  double rd_cyc = 0, at_cyc = 0, rd_free = 0, at_free = 0;
  int64_t rd_groups = 0, at_groups = 0;
  for (int tile = 0; tile < t.n_tiles; ++tile) {
    const int n_owned = std::min(t.own, t.nv - tile * t.own);
    const int f0 = t.tile_facet_off[tile], f1 = t.tile_facet_off[tile + 1];
    for (int k = 0; k < 3; ++k) {
      for (int g0 = f0; g0 < f1; g0 += 32) {  // reads: 32 lanes, bank pair = slot mod 32, same slot broadcasts
        int slots[32], ns = 0, cnt[32] = {0};
        for (int p = g0; p < std::min(f1, g0 + 32); ++p) {
          const TileFacet& f = t.tile_facets[p];
          const int s = k == 0 ? f.l0 : (k == 1 ? f.l1 : f.l2);
          bool dup = false;
          for (int q = 0; q < ns; ++q) dup |= slots[q] == s;
          if (!dup) {
            slots[ns++] = s;
            ++cnt[s & 31];
          }
        }
        int mx = 1;
        for (int q = 0; q < 32; ++q) mx = std::max(mx, cnt[q]);
        rd_cyc += mx;
        rd_free += mx == 1;
        ++rd_groups;
      }
      for (int g0 = f0; g0 < f1; g0 += 16) {  // atomics: 16 lanes, bank pair = slot mod 16, owned corners only
        int cnt[16] = {0}, any = 0;
        for (int p = g0; p < std::min(f1, g0 + 16); ++p) {
          const TileFacet& f = t.tile_facets[p];
          const int s = k == 0 ? f.l0 : (k == 1 ? f.l1 : f.l2);
          if (s < n_owned) {
            ++cnt[s & 15];
            any = 1;
          }
        }
        if (!any) continue;
        int mx = 1;
        for (int q = 0; q < 16; ++q) mx = std::max(mx, cnt[q]);
        at_cyc += mx;
        at_free += mx == 1;
        ++at_groups;
      }
    }
  }
  model[0] = rd_groups ? rd_cyc / rd_groups : 0.0;
  model[1] = at_groups ? at_cyc / at_groups : 0.0;
  model[2] = rd_groups ? rd_free / rd_groups : 0.0;
  model[3] = at_groups ? at_free / at_groups : 0.0;
  return MS_OK;
}

int ms_plan_lane_order(int nv, int nf, const double* positions, const int32_t* tri, int tile_vertices, double model[16],
                       int32_t* facet_off_out, int32_t* common_out, int32_t* lean_out) {
  if (!model) return fail(nullptr, MS_ERR_INVALID, "ms_plan_lane_order: model is NULL");
  Tiling t;
  std::string err;
  int rc = build_tiling(nv, nf, positions, tri, nullptr, tile_vertices, 1, t, err);
  if (rc != MS_OK) return fail(nullptr, rc, err);
  const LaneModel* ms[2] = {&t.model_common, &t.model_lean};
  for (int i = 0; i < 2; ++i) {
    const LaneModel& m = *ms[i];
    double* o = model + 8 * i;
    o[0] = m.a16_groups > 0 ? m.a16_sum / m.a16_groups : 0.0;
    o[1] = m.r16_groups > 0 ? m.r16_sum / m.r16_groups : 0.0;
    o[2] = m.r32_groups > 0 ? m.r32_sum / m.r32_groups : 0.0;
    o[3] = m.ka();
    o[4] = m.kc();
    o[5] = m.a16_groups;
    o[6] = m.r16_groups;
    o[7] = m.r32_groups;
  }
  if (facet_off_out) memcpy(facet_off_out, t.tile_facet_off.data(), sizeof(int32_t) * t.tile_facet_off.size());
  const std::vector<TileFacet>* src[2] = {&t.tile_facets, &t.tile_facets_lean};
  int32_t* dst[2] = {common_out, lean_out};
  for (int i = 0; i < 2; ++i)
    if (dst[i])
      for (size_t p = 0; p < src[i]->size(); ++p) {
        const TileFacet& f = (*src[i])[p];
        dst[i][4 * p] = f.l0;
        dst[i][4 * p + 1] = f.l1;
        dst[i][4 * p + 2] = f.l2;
        dst[i][4 * p + 3] = f.flags;
      }
  return MS_OK;
}

int ms_lane_order_stats(ms_ctx* c, int64_t stats[2]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->lane_order_on ? 1 : 0;
  stats[1] = 0;
  return MS_OK;
}

// ---- kernel-provider seam ---------------------------------------------------

int ms_surface_energy_and_gradient_host(int nv, int nf, const double* pos, const int32_t* tri,
                                        const double* gamma, double* grad, double* energy) {
  if (!pos || !gamma || !energy || (nf > 0 && !tri))
    return fail(nullptr, MS_ERR_INVALID, "ms_surface_energy_and_gradient_host: NULL argument");
  ms_ctx* c = nullptr;
  int rc = ms_create(&c, 0, nv, nf, pos, tri, nullptr, nullptr, nullptr, 0, 0, 1);
  if (rc) return rc;
  rc = ms_set_surface_tension(c, gamma);
  ms_params p = c->params;
  p.modules = MS_MOD_SURFACE;
  if (!rc) rc = ms_set_params(c, &p);
  double e[3] = {0, 0, 0};
  std::vector<double> g;
  if (!rc) {
    g.resize(3 * (size_t)nv);
    rc = ms_energy_and_gradient(c, e, grad ? g.data() : nullptr);
  }
  if (rc) g_last_error = c->err;
  ms_destroy(c);
  if (rc) return rc;
  *energy = e[0];
  if (grad)
    for (size_t i = 0; i < g.size(); ++i) grad[i] += g[i];  // intent(inout): accumulate
  return MS_OK;
}

int ms_grad_cotan_batch_host(int n, const double* u, const double* v, double* grad_u, double* grad_v) {
  if (n < 0 || !u || !v || !grad_u || !grad_v)
    return fail(nullptr, MS_ERR_INVALID, "ms_grad_cotan_batch_host: bad argument");
  const size_t b = sizeof(double) * 3 * (size_t)n;
  DevBuf du, dv, dgu, dgv;
  SEAM_HIP(du.alloc(b));
  SEAM_HIP(dv.alloc(b));
  SEAM_HIP(dgu.alloc(b));
  SEAM_HIP(dgv.alloc(b));
  SEAM_HIP(hipMemcpy(du.p, u, b, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemcpy(dv.p, v, b, hipMemcpyHostToDevice));
  SEAM_HIP(launch_grad_cotan(n, du.as<double>(), dv.as<double>(), dgu.as<double>(), dgv.as<double>(), nullptr));
  SEAM_HIP(hipMemcpy(grad_u, dgu.p, b, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(grad_v, dgv.p, b, hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_apply_beltrami_laplacian_host(int dim, int nv, int nf, const double* weights,
                                     const int32_t* tri, const double* field, double* out) {
  if (dim <= 0 || nv <= 0 || nf < 0 || !weights || !tri || !field || !out)
    return fail(nullptr, MS_ERR_INVALID, "ms_apply_beltrami_laplacian_host: bad argument");
  const size_t bw = sizeof(double) * 3 * (size_t)nf, bt = sizeof(int32_t) * 3 * (size_t)nf,
               bf = sizeof(double) * (size_t)nv * dim;
  DevBuf dw, dt, df, dout;
  SEAM_HIP(dw.alloc(bw));
  SEAM_HIP(dt.alloc(bt));
  SEAM_HIP(df.alloc(bf));
  SEAM_HIP(dout.alloc(bf));
  SEAM_HIP(hipMemcpy(dw.p, weights, bw, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemcpy(dt.p, tri, bt, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemcpy(df.p, field, bf, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemset(dout.p, 0, bf));
  SEAM_HIP(launch_laplacian_scatter(dim, nv, nf, dw.as<double>(), dt.as<int32_t>(), df.as<double>(),
                                    dout.as<double>(), nullptr));
  SEAM_HIP(hipMemcpy(out, dout.p, bf, hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_p1_triangle_divergence_host(int nv, int nf, const double* pos, const double* tilts,
                                   const int32_t* tri, double* div_tri, double* area, double* g0,
                                   double* g1, double* g2) {
  if (nv <= 0 || nf < 0 || !pos || !tilts || !tri || !div_tri || !area || !g0 || !g1 || !g2)
    return fail(nullptr, MS_ERR_INVALID, "ms_p1_triangle_divergence_host: bad argument");
  const size_t bp = sizeof(double) * 3 * (size_t)nv, bt = sizeof(int32_t) * 3 * (size_t)nf,
               b1 = sizeof(double) * (size_t)nf, b3 = 3 * b1;
  DevBuf dp, dtl, dt, dd, da, d0, d1, d2;
  SEAM_HIP(dp.alloc(bp));
  SEAM_HIP(dtl.alloc(bp));
  SEAM_HIP(dt.alloc(bt));
  SEAM_HIP(dd.alloc(b1));
  SEAM_HIP(da.alloc(b1));
  SEAM_HIP(d0.alloc(b3));
  SEAM_HIP(d1.alloc(b3));
  SEAM_HIP(d2.alloc(b3));
  SEAM_HIP(hipMemcpy(dp.p, pos, bp, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemcpy(dtl.p, tilts, bp, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemcpy(dt.p, tri, bt, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemset(dd.p, 0, b1));
  SEAM_HIP(hipMemset(da.p, 0, b1));
  SEAM_HIP(hipMemset(d0.p, 0, b3));
  SEAM_HIP(hipMemset(d1.p, 0, b3));
  SEAM_HIP(hipMemset(d2.p, 0, b3));
  SEAM_HIP(launch_p1_divergence(nv, nf, dp.as<double>(), dtl.as<double>(), dt.as<int32_t>(),
                                dd.as<double>(), da.as<double>(), d0.as<double>(), d1.as<double>(),
                                d2.as<double>(), nullptr));
  SEAM_HIP(hipMemcpy(div_tri, dd.p, b1, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(area, da.p, b1, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(g0, d0.p, b3, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(g1, d1.p, b3, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(g2, d2.p, b3, hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_compute_curvature_data_host(int nv, int nf, const double* pos, const int32_t* tri,
                                   double* k_vecs, double* vertex_areas, double* weights,
                                   double* va0, double* va1, double* va2) {
  if (nv <= 0 || nf < 0 || !pos || !tri || !k_vecs || !vertex_areas || !weights)
    return fail(nullptr, MS_ERR_INVALID, "ms_compute_curvature_data_host: bad argument");
  const size_t bp = sizeof(double) * 3 * (size_t)nv, bt = sizeof(int32_t) * 3 * (size_t)nf,
               b1 = sizeof(double) * (size_t)nf, bv = sizeof(double) * (size_t)nv;
  DevBuf dp, dt, dk, da, dw, d0, d1, d2;
  SEAM_HIP(dp.alloc(bp));
  SEAM_HIP(dt.alloc(bt));
  SEAM_HIP(dk.alloc(bp));
  SEAM_HIP(da.alloc(bv));
  SEAM_HIP(dw.alloc(3 * b1));
  SEAM_HIP(d0.alloc(b1));
  SEAM_HIP(d1.alloc(b1));
  SEAM_HIP(d2.alloc(b1));
  SEAM_HIP(hipMemcpy(dp.p, pos, bp, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemcpy(dt.p, tri, bt, hipMemcpyHostToDevice));
  SEAM_HIP(hipMemset(dk.p, 0, bp));
  SEAM_HIP(hipMemset(da.p, 0, bv));
  SEAM_HIP(hipMemset(dw.p, 0, 3 * b1));
  SEAM_HIP(hipMemset(d0.p, 0, b1));
  SEAM_HIP(hipMemset(d1.p, 0, b1));
  SEAM_HIP(hipMemset(d2.p, 0, b1));
  SEAM_HIP(launch_curvature_raw(nv, nf, dp.as<double>(), dt.as<int32_t>(), dk.as<double>(),
                                da.as<double>(), dw.as<double>(), d0.as<double>(), d1.as<double>(),
                                d2.as<double>(), nullptr));
  SEAM_HIP(hipMemcpy(k_vecs, dk.p, bp, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(vertex_areas, da.p, bv, hipMemcpyDeviceToHost));
  SEAM_HIP(hipMemcpy(weights, dw.p, 3 * b1, hipMemcpyDeviceToHost));
  if (va0) SEAM_HIP(hipMemcpy(va0, d0.p, b1, hipMemcpyDeviceToHost));
  if (va1) SEAM_HIP(hipMemcpy(va1, d1.p, b1, hipMemcpyDeviceToHost));
  if (va2) SEAM_HIP(hipMemcpy(va2, d2.p, b1, hipMemcpyDeviceToHost));
  return MS_OK;
}

}  // extern "C"
