// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): create / destroy, setters and getters, curvature fields.
extern "C" {

const char* ms_version(void) { return "membrane_hip 0.1 (gfx950)"; }

int ms_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
    return MS_ERR_HIP;
  }
  return n;
}

const char* ms_last_error(const ms_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

int ms_create(ms_ctx** out, int device, int nv, int nf, const double* positions,
              const int32_t* tri, const uint8_t* fixed, const uint8_t* boundary,
              const uint8_t* body_facets, int tile_vertices, int shard_rank, int shard_count) {
  if (!out) return fail(nullptr, MS_ERR_INVALID, "ms_create: out is NULL");
  *out = nullptr;
  if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count)
    return fail(nullptr, MS_ERR_INVALID, "ms_create: bad shard_rank/shard_count");
  ms_ctx* c = new (std::nothrow) ms_ctx();
  if (!c) return fail(nullptr, MS_ERR_NOMEM, "ms_create: out of host memory");
  std::string err;
  int rc = build_tiling(nv, nf, positions, tri, body_facets, tile_vertices, shard_count, c->til, err);
  if (rc != MS_OK) {
    delete c;
    return fail(nullptr, rc, err);
  }
  c->device = device;
  c->shard_rank = shard_rank;
  c->shard_count = shard_count;
  const Tiling& t = c->til;
  c->tile0 = std::min(t.n_tiles, shard_rank * t.tiles_per_shard);
  c->tile1 = std::min(t.n_tiles, (shard_rank + 1) * t.tiles_per_shard);
  c->cap = t.own + t.max_halo;
  {
    const size_t le = energy_lds_bytes(t.T, c->cap, t.max_ent, true, true, true);
    const size_t lg = gradient_lds_bytes(t.T, c->cap, t.max_ent, true, true);
    if (le > MS_LDS_CU || lg > MS_LDS_CU) {
      delete c;
      return fail(nullptr, MS_ERR_TILE_CAPACITY,
                  "ms_create: a vertex patch (tile + halo) exceeds the 160 KiB LDS of a CU; "
                  "use a smaller tile_vertices");
    }
  }
#define CREATE_CHK(call)                                       \
  do {                                                         \
    int rc_ = (call);                                          \
    if (rc_ != MS_OK) {                                        \
      std::string m_ = c->err;                                 \
      ms_destroy(c);                                           \
      return fail(nullptr, rc_, m_);                           \
    }                                                          \
  } while (0)
#define CREATE_HIP(call)                                                         \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      std::string m_ = std::string(#call) + ": " + hipGetErrorString(e_);        \
      ms_destroy(c);                                                             \
      return fail(nullptr, MS_ERR_HIP, m_);                                      \
    }                                                                            \
  } while (0)
  CREATE_HIP(hipSetDevice(device));
  CREATE_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->own_stream = true;
  CREATE_CHK(upload(c, &c->d_perm, t.perm));
  CREATE_CHK(upload(c, &c->d_tile_facet_off, t.tile_facet_off));
  CREATE_CHK(upload(c, &c->d_tile_facets, t.tile_facets));
  if (t.own + t.max_halo <= 1024) {
    std::vector<uint32_t> packed(t.tile_facets.size());
    for (size_t i = 0; i < packed.size(); ++i) {
      const TileFacet& f = t.tile_facets[i];
      packed[i] = (uint32_t)f.l0 | ((uint32_t)f.l1 << 10) | ((uint32_t)f.l2 << 20) | ((uint32_t)(f.flags & 3u) << 30);
    }
    CREATE_CHK(upload(c, &c->d_tile_facets32, packed));
    // MS_LANE_ORDER=0: the lean k_energy instances read the common array too (the A/B switch)
    if (!(getenv("MS_LANE_ORDER") != nullptr && atoi(getenv("MS_LANE_ORDER")) == 0)) {
      for (size_t i = 0; i < packed.size(); ++i) {
        const TileFacet& f = t.tile_facets_lean[i];
        packed[i] = (uint32_t)f.l0 | ((uint32_t)f.l1 << 10) | ((uint32_t)f.l2 << 20) | ((uint32_t)(f.flags & 3u) << 30);
      }
      CREATE_CHK(upload(c, &c->d_tile_facets_lean, packed));
      c->lane_order_on = true;
    }
  }
  CREATE_CHK(upload(c, &c->d_tile_halo_off, t.tile_halo_off));
  CREATE_CHK(upload(c, &c->d_halo_ids, t.halo_ids));
  CREATE_CHK(upload(c, &c->d_tile_ent_off, t.tile_ent_off));
  CREATE_CHK(upload(c, &c->d_tile_voff, t.tile_voff));
  CREATE_CHK(upload(c, &c->d_vent, t.vent));
  {
    std::vector<double> ones(t.tile_facets.size(), 1.0);
    CREATE_CHK(upload(c, &c->d_tf_gamma, ones));
  }
  {
    std::vector<uint8_t> fl((size_t)t.nvp, VF_FIXED);  // padded rows never move
    for (int i = 0; i < nv; ++i) {
      const int e = t.perm[i];
      uint8_t f = 0;
      if (fixed && fixed[e]) f |= VF_FIXED;
      if (boundary && boundary[e]) {
        f |= VF_BOUNDARY;
        c->has_boundary = true;
      }
      fl[i] = f;
    }
    CREATE_CHK(upload(c, &c->d_vflags, fl));
    c->h_vflags = fl;
    std::vector<double> zeros((size_t)t.nvp, 0.0);
    CREATE_CHK(upload(c, &c->d_kappa, zeros));
    CREATE_CHK(upload(c, &c->d_c0, zeros));
  }
  // state: 8 (nvp,3) vectors + fA (nvp,2)
  {
    const size_t n3 = 3 * (size_t)t.nvp;
    const size_t total = 8 * n3 + 2 * (size_t)t.nvp;
    CREATE_HIP(hipMalloc(reinterpret_cast<void**>(&c->state), total * sizeof(double)));
    CREATE_HIP(hipMemset(c->state, 0, total * sizeof(double)));
    for (int b = 0; b <= MS_BUF_FK; ++b) c->buf[b] = c->state + (size_t)b * n3;
    c->buf[MS_BUF_FA] = c->state + 8 * n3;
  }
  CREATE_HIP(hipMalloc(reinterpret_cast<void**>(&c->d_partials),
                       sizeof(double) * MS_NPART * (size_t)std::max(1, t.n_tiles)));
  CREATE_HIP(hipMemset(c->d_partials, 0, sizeof(double) * MS_NPART * (size_t)std::max(1, t.n_tiles)));
  CREATE_HIP(hipMalloc(reinterpret_cast<void**>(&c->d_scal), sizeof(double) * MS_NSCAL));
  CREATE_HIP(hipMemset(c->d_scal, 0, sizeof(double) * MS_NSCAL));
  c->buf[MS_BUF_SCAL] = c->d_scal;
  c->h_scal = static_cast<double*>(calloc(MS_NSCAL, sizeof(double)));
  CREATE_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_seq), sizeof(unsigned long long) * 2 * MS_MB_WORDS,
                           hipHostMallocMapped));
  memset(c->h_seq, 0, sizeof(unsigned long long) * 2 * MS_MB_WORDS);
  CREATE_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_h_seq), c->h_seq, 0));
  CREATE_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_err), sizeof(unsigned long long) * 8, hipHostMallocMapped));
  memset(c->h_err, 0, sizeof(unsigned long long) * 8);
  CREATE_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_h_err), c->h_err, 0));
  CREATE_HIP(hipMalloc(reinterpret_cast<void**>(&c->d_stage), sizeof(double) * 3 * (size_t)nv));
  {
    // boundary lists of every rank (each rank derives all of them from the shared tiling)
    const int W = shard_count;
    const int rows_per = t.tiles_per_shard * t.own;
    std::vector<std::vector<int32_t>> lists((size_t)W);
    std::vector<int32_t> my_halo;
    for (int tile = 0; tile < t.n_tiles; ++tile) {
      const int tr = tile / t.tiles_per_shard;
      for (int h = t.tile_halo_off[tile]; h < t.tile_halo_off[tile + 1]; ++h) {
        const int32_t v = t.halo_ids[h];
        const int owner = v / rows_per;
        if (owner == tr) continue;
        lists[(size_t)owner].push_back(v);
        if (tr == shard_rank) my_halo.push_back(v);
      }
    }
    std::vector<int32_t> flat;
    c->bnd_off.assign((size_t)W + 1, 0);
    for (int r = 0; r < W; ++r) {
      auto& l = lists[(size_t)r];
      std::sort(l.begin(), l.end());
      l.erase(std::unique(l.begin(), l.end()), l.end());
      c->bnd_off[(size_t)r + 1] = c->bnd_off[(size_t)r] + (int32_t)l.size();
      c->bnd_max = std::max(c->bnd_max, (int)l.size());
      flat.insert(flat.end(), l.begin(), l.end());
    }
    std::sort(my_halo.begin(), my_halo.end());
    my_halo.erase(std::unique(my_halo.begin(), my_halo.end()), my_halo.end());
    c->n_halo_rows = (int)my_halo.size();
    CREATE_CHK(upload(c, &c->d_bnd_rows, flat));
    CREATE_CHK(upload(c, &c->d_bnd_off, c->bnd_off));
    CREATE_CHK(upload(c, &c->d_halo_rows, my_halo));
    CREATE_HIP(hipMalloc(reinterpret_cast<void**>(&c->d_scal_all), sizeof(double) * MS_NSCAL * (size_t)W));
    CREATE_HIP(hipMemset(c->d_scal_all, 0, sizeof(double) * MS_NSCAL * (size_t)W));
  }
  {
    TiltField& f0 = c->tf[0];
    f0.fixed_bit = VF_TILT_FIXED; f0.mod_tilt = MS_MOD_TILT; f0.mod_smooth = MS_MOD_TILT_SMOOTH;
    f0.s_etilt = MS_S_ETILT; f0.s_ets = MS_S_ETS; f0.s_gn2 = MS_S_TGNORM2; f0.s_rz = MS_S_TRZ;
    TiltField& f1 = c->tf[1];
    f1.fixed_bit = VF_TILT_FIXED_IN; f1.mod_tilt = MS_MOD_TILT_IN; f1.mod_smooth = MS_MOD_TILT_SMOOTH_IN;
    f1.s_etilt = MS_S_ETILT_IN; f1.s_ets = MS_S_ETS_IN; f1.s_gn2 = MS_S_TGNORM2_IN; f1.s_rz = MS_S_TRZ_IN;
    f1.mod_bt = MS_MOD_BENDING_TILT_IN; f1.s_ebt = MS_S_EBT_IN; f1.div_sign = -1.0;  // bending_tilt_in.py:46
    f0.mod_bt = MS_MOD_BENDING_TILT; f0.s_ebt = MS_S_EBT;
    f1.mod_dt = MS_MOD_TILT_DISK_TARGET_IN; f1.s_edt = MS_S_EDT_IN; f1.s_dtr = MS_S_DTR_IN;
    f1.mod_rs = MS_MOD_TILT_RIM_SOURCE_IN;
    f1.mod_addons = addon_readers(1, /*rsm_inner=*/false);  // (rim_slope_match_out's bit: ms_set_rim_match, with a disk ring)
    TiltField& f2 = c->tf[2];
    f2.fixed_bit = VF_TILT_FIXED_OUT; f2.mod_tilt = MS_MOD_TILT_OUT; f2.mod_smooth = MS_MOD_TILT_SMOOTH_OUT;
    f2.s_etilt = MS_S_ETILT_OUT; f2.s_ets = MS_S_ETS_OUT; f2.s_gn2 = MS_S_TGNORM2_OUT; f2.s_rz = MS_S_TRZ_OUT;
    f2.mod_bt = MS_MOD_BENDING_TILT_OUT; f2.s_ebt = MS_S_EBT_OUT; f2.div_sign = 1.0;
    f2.mod_dt = MS_MOD_TILT_DISK_TARGET_OUT; f2.s_edt = MS_S_EDT_OUT; f2.s_dtr = MS_S_DTR_OUT;
    f2.mod_rs = MS_MOD_TILT_RIM_SOURCE_OUT;
    f2.mod_addons = addon_readers(2, false);
  }
  if (const char* pe = getenv("MS_PAIR")) {
    c->pair_enable = atoi(pe) != 0;
    c->pair_force = atoi(pe) >= 2 ? std::min(atoi(pe), 4) : 0;  // 4: triple launches whenever possible
  }
  c->speculate = !(getenv("MS_SPECULATE") != nullptr && atoi(getenv("MS_SPECULATE")) == 0);
  c->ahead_enable = !(getenv("MS_AHEAD") != nullptr && atoi(getenv("MS_AHEAD")) == 0);
  c->escalate = !(getenv("MS_ESCALATE") != nullptr && atoi(getenv("MS_ESCALATE")) == 0);
  if (getenv("MS_ESCALATE") != nullptr && atoi(getenv("MS_ESCALATE")) > 0) c->escalate_after = atoi(getenv("MS_ESCALATE"));
  c->ls_reset = !(getenv("MS_LS_RESET") != nullptr && atoi(getenv("MS_LS_RESET")) == 0);
  c->no_fast = variant_env("MS_NO_FAST") != nullptr && atoi(variant_env("MS_NO_FAST")) != 0;
  c->pair_lean_enable = !(getenv("MS_PAIR_LEAN") != nullptr && atoi(getenv("MS_PAIR_LEAN")) == 0);
  c->deterministic = getenv("MS_DETERMINISTIC") != nullptr && atoi(getenv("MS_DETERMINISTIC")) != 0;
  // MS_KA_LEAN=0: the general k_energy instance everywhere (the A/B switch, and how the tests set the two instances
  // against each other).  A one-tile mesh never takes the lean instance: its launches are k_exec's, and stay the same
  // kernel code whether the recorder is attached or not (MS_EXEC=0, profiling)
  c->ka_lean_off = ((getenv("MS_KA_LEAN") != nullptr && atoi(getenv("MS_KA_LEAN")) == 0) || t.n_tiles == 1) ? 1u : 0u;
  c->resident_enable = !(getenv("MS_RESIDENT") != nullptr && atoi(getenv("MS_RESIDENT")) == 0);
  c->params.modules = MS_MOD_SURFACE;
  c->params.bending_model = MS_BEND_HELFRICH;
  c->params.bending_grad_mode = MS_GRAD_ANALYTIC;
  c->params.volume_stiffness = 1000.0;
  c->params.target_volume = 0.0;
  c->carry.last_g = c->buf[MS_BUF_G];
  // A mesh of ONE tile: every kernel is one workgroup and a step is launches and host round trips -- record the launches
  // and run them pack by pack in one workgroup (k_exec).  MS_EXEC=0 keeps the launch-per-kernel path (A/B, tests).
  c->exec_wanted = t.n_tiles == 1 && t.T == 256 && t.own == 256 && shard_count == 1 &&
                   !(getenv("MS_EXEC") != nullptr && atoi(getenv("MS_EXEC")) == 0);
  if (c->exec_wanted) {
    c->exec.stream = c->stream;
    c->exec.T = t.T;
    exec_attach(&c->exec);
    c->exec_on = true;
    c->pair_enable = false;  // (several trials per launch buy nothing inside one workgroup)
    c->exec_relax = !(getenv("MS_EXEC_RELAX") != nullptr && atoi(getenv("MS_EXEC_RELAX")) == 0);
    c->exec_fused = !(getenv("MS_EXEC_FUSED") != nullptr && atoi(getenv("MS_EXEC_FUSED")) == 0);
    c->exec_pins = !(getenv("MS_EXEC_PINS") != nullptr && atoi(getenv("MS_EXEC_PINS")) == 0);
  }
  c->shard_chain_enable = !(getenv("MS_SHARD_CHAIN") != nullptr && atoi(getenv("MS_SHARD_CHAIN")) == 0);
  // tilt relaxations of multi-tile meshes: the backtracking search as multi-trial passes (MS_TSEARCH=0: one launch per
  // module, field and trial, the form the one-tile interpreter records)
  c->tenergy_enable = shard_count == 1 && !(getenv("MS_TSEARCH") != nullptr && atoi(getenv("MS_TSEARCH")) == 0);
  c->tsearch_enable = !c->exec_on && c->tenergy_enable;
  CREATE_CHK(ext_to_patch(c, positions, c->buf[MS_BUF_X], 3));
#undef CREATE_CHK
#undef CREATE_HIP
  *out = c;
  return MS_OK;
}

void ms_destroy(ms_ctx* c) {
  if (g_host_timing.on && g_host_timing.n > 0) {
    fprintf(stderr, "[ms host timing] %ld waits followed by an energy launch: mailbox seen -> launch call returned %.2f us "
                    "on average (max %.1f), of which the launch call itself %.2f us\n",
            g_host_timing.n, g_host_timing.sum_gap / g_host_timing.n, g_host_timing.max_gap,
            g_host_timing.sum_launch / g_host_timing.n);
    g_host_timing.n = 0;
    g_host_timing.sum_gap = g_host_timing.sum_launch = g_host_timing.max_gap = 0.0;
  }
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->exec_on) {
    (void)c->exec.flush();
    exec_detach(&c->exec);
    c->exec_on = false;
  }
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (!c->own_state) c->state = nullptr;
  void* ptrs[] = {c->d_perm, c->d_tile_facet_off, c->d_tile_facets, c->d_tile_facets32, c->d_tile_facets_lean, c->d_tf_gamma, c->d_volgrad_cache,
                  c->d_tile_halo_off, c->d_halo_ids, c->d_tile_ent_off, c->d_tile_voff, c->d_vent,
                  c->d_vflags, c->d_kappa, c->d_c0, c->tf[0].tilts, c->tf[0].grad, c->tf[0].trial, c->d_bt_vert, c->d_tn, c->tf[0].dir, c->tf[0].minv,
                  c->tf[1].tilts, c->tf[1].grad, c->tf[1].trial, c->tf[1].dir, c->tf[1].minv,
                  c->tf[2].tilts, c->tf[2].grad, c->tf[2].trial, c->tf[2].dir, c->tf[2].minv,
                  c->tf[1].kappa, c->tf[1].c0, c->tf[1].bt_vert, c->tf[2].kappa, c->tf[2].c0, c->tf[2].bt_vert,
                  c->tf[1].disk, c->tf[1].diff, c->tf[2].disk, c->tf[2].diff, c->tf[0].va, c->tf[1].va, c->tf[2].va,
                  c->state, c->d_partials, c->d_scal, c->d_stage, c->d_bnd_rows, c->d_bnd_off,
                  c->d_halo_rows, c->d_scal_all, c->d_pins, c->edge[0].d_blob, c->edge[1].d_blob, c->tf[1].d_rim, c->tf[2].d_rim,
                  c->d_cpl, c->d_st, c->d_rimb, c->d_tb, c->d_tbb, c->d_rsm,
                  c->d_area_ga, c->d_area_part, c->d_area_res, c->d_area_cache, c->d_perim};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (auto& lane : c->edge)
    for (int w = 0; w < 2; ++w)
      for (auto& ev : lane.prof[w]) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
      }
  for (void* q : c->peer_opened) (void)hipIpcCloseMemHandle(q);
  if (c->d_peer_slab) (void)hipFree(c->d_peer_slab);
  if (c->d_peer_flag) (void)hipFree(c->d_peer_flag);
  if (c->d_peer_flagtab) (void)hipFree(c->d_peer_flagtab);
  if (c->d_peer_arrived) (void)hipFree(c->d_peer_arrived);
  if (c->comm) shard_comm_destroy(c->comm);
  if (c->d_xsend) (void)hipFree(c->d_xsend);
  if (c->d_xrecv) (void)hipFree(c->d_xrecv);
  if (c->h_scal_all) (void)hipHostFree(c->h_scal_all);
  if (c->h_xseq) (void)hipHostFree(c->h_xseq);
  for (int p = 0; p < 2; ++p) {
    for (auto& m : c->spec[p]) {
      free(m.h_scal);
      if (m.h_seq) (void)hipHostFree(m.h_seq);
    }
    for (ms_ctx::Mailbox* m : {&c->grad_mb[p], &c->first_mb[p]}) {
      free(m->h_scal);
      if (m->h_seq) (void)hipHostFree(m->h_seq);
    }
  }
  if (c->d_sh_dec) (void)hipFree(c->d_sh_dec);
  if (c->h_sh_post) (void)hipHostFree(c->h_sh_post);
  free(c->tsearch_mb.h_scal);
  if (c->tsearch_mb.h_seq) (void)hipHostFree(c->tsearch_mb.h_seq);
  if (c->d_dec) (void)hipFree(c->d_dec);
  if (c->h_err) (void)hipHostFree(c->h_err);
  if (c->d_prof_ran) (void)hipFree(c->d_prof_ran);
  if (c->exec.d_stamps) (void)hipFree(c->exec.d_stamps);
  if (c->d_res_partials) (void)hipFree(c->d_res_partials);
  if (c->d_res_bar) (void)hipFree(c->d_res_bar);
  if (c->d_res_log) (void)hipFree(c->d_res_log);
  if (c->d_res_result) (void)hipFree(c->d_res_result);
  for (int l = 0; l < 3; ++l)
    if (c->tf[l].dt_target) (void)hipFree(c->tf[l].dt_target);
  if (c->d_relax_cells) (void)hipFree(c->d_relax_cells);
  if (c->h_relax_box) (void)hipHostFree(c->h_relax_box);
  for (auto& sd : c->side) {
    if (sd.partials) (void)hipFree(sd.partials);
    if (sd.scal) (void)hipFree(sd.scal);
    for (auto& m : sd.mb) {
      free(m.h_scal);
      if (m.h_seq) (void)hipHostFree(m.h_seq);
    }
  }
  for (double* q : {c->xt2, c->fK2, c->fA2, c->xt3, c->fK3, c->fA3})
    if (q) (void)hipFree(q);
  free(c->h_scal);
  if (c->h_seq) (void)hipHostFree(c->h_seq);
  for (auto& r : c->prof_pending) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : c->prof_pool) (void)hipEventDestroy(e);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int ms_set_stream(ms_ctx* c, void* hip_stream) {
  if (!c) return MS_ERR_INVALID;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  if (c->own_stream && c->stream) {
    HIPCHK(c, hipStreamDestroy(c->stream));
    c->own_stream = false;
  }
  if (hip_stream) {
    c->stream = static_cast<hipStream_t>(hip_stream);
  } else {
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  // (nothing is pending: S(c) above launched it)  A recorder is found by its stream: two contexts on one caller-provided
  // stream cannot both record -- the second one keeps the launch-per-kernel path
  if (c->exec_on) {
    exec_detach(&c->exec);
    c->exec.stream = c->stream;
    if (exec_find(c->stream) != nullptr) {
      c->exec_on = false;
      c->exec_wanted = false;
    } else {
      exec_attach(&c->exec);
    }
  } else {
    c->exec.stream = c->stream;
  }
  return MS_OK;
}

int ms_set_surface_tension(ms_ctx* c, const double* gamma) {
  if (!c || !gamma) return fail(c, MS_ERR_INVALID, "ms_set_surface_tension: NULL argument");
  const Tiling& t = c->til;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  std::vector<double> g(t.tile_facets.size());
  for (size_t p = 0; p < g.size(); ++p) g[p] = gamma[t.tile_facet_ext[p]];
  c->gamma_uniform = true;
  c->gamma_const = t.nf > 0 ? gamma[0] : 1.0;
  for (int f = 1; f < t.nf && c->gamma_uniform; ++f) c->gamma_uniform = gamma[f] == c->gamma_const;
  if (!g.empty())
    HIPCHK(c, hipMemcpy(c->d_tf_gamma, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return MS_OK;
}

int ms_set_bending_params(ms_ctx* c, const double* kappa, const double* c0) {
  if (!c || !kappa || !c0) return fail(c, MS_ERR_INVALID, "ms_set_bending_params: NULL argument");
  const Tiling& t = c->til;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  std::vector<double> k((size_t)t.nvp, 0.0), z((size_t)t.nvp, 0.0);
  c->kc_uniform = true;
  c->kappa_const = kappa[0];
  c->c0_const = c0[0];
  for (int i = 0; i < t.nv; ++i) {
    k[i] = kappa[t.perm[i]];
    z[i] = c0[t.perm[i]];
    c->kc_uniform = c->kc_uniform && kappa[i] == c->kappa_const && c0[i] == c->c0_const;
  }
  HIPCHK(c, hipMemcpy(c->d_kappa, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_c0, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice));
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return MS_OK;
}

int ms_set_params(ms_ctx* c, const ms_params* p) {
  if (!c || !p) return fail(c, MS_ERR_INVALID, "ms_set_params: NULL argument");
  if (p->bending_model != MS_BEND_HELFRICH && p->bending_model != MS_BEND_WILLMORE)
    return fail(c, MS_ERR_INVALID, "ms_set_params: bad bending_model");
  if (p->bending_grad_mode != MS_GRAD_ANALYTIC && p->bending_grad_mode != MS_GRAD_APPROX)
    return fail(c, MS_ERR_INVALID, "ms_set_params: bad bending_grad_mode");
  if ((p->modules & MS_MOD_BENDING) && (p->modules & MS_MOD_BENDING_TILT))
    return fail(c, MS_ERR_INVALID, "ms_set_params: bending and bending_tilt are mutually exclusive");
  if ((p->modules & MS_LEAFLET_BT) && (p->modules & (MS_MOD_BENDING | MS_MOD_BENDING_TILT)))
    return fail(c, MS_ERR_INVALID, "ms_set_params: bending / bending_tilt together with bending_tilt_in/out is outside the device path");
  if ((p->modules & MS_MOD_BENDING_TILT) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the bending_tilt module is not sharded yet (single GPU only)");
  if ((p->modules & MS_MOD_AREA_PENALTY) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the body_area_penalty module is not sharded (single GPU only)");
  if ((p->modules & MS_MOD_AREA_PENALTY) && (p->modules & MS_ANY_TILT_MODS))
    return fail(c, MS_ERR_STATE, "body_area_penalty together with a tilt-family module is outside the device path");
  for (const EdgeTerm& t : kEdgeTerms) {
    if ((p->modules & t.bit) && c->shard_count != 1) return fail(c, MS_ERR_STATE, edge_not_sharded(t));
    if ((p->modules & t.bit) && (p->modules & MS_ANY_TILT_MODS))
      return fail(c, MS_ERR_STATE, std::string(t.name) + " together with a tilt-family module is outside the device path");
  }
  if ((p->modules & MS_LEAFLET_RS) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the tilt_rim_source_in/out modules are not sharded (single GPU only)");
  if ((p->modules & MS_MOD_TILT_RIM_SOURCE_BILAYER) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the tilt_rim_source_bilayer module is not sharded (single GPU only)");
  if ((p->modules & MS_MOD_TILT_RIM_SOURCE_BILAYER) && (p->modules & MS_TILT_MODS))
    return fail(c, MS_ERR_STATE, "tilt_rim_source_bilayer together with a single-field tilt module is outside the device path");
  if ((p->modules & MS_MOD_TILT_THETAB_CONTACT_IN) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the tilt_thetaB_contact_in module is not sharded (single GPU only)");
  if ((p->modules & MS_MOD_TILT_THETAB_CONTACT_IN) && (p->modules & MS_TILT_MODS))
    return fail(c, MS_ERR_STATE, "tilt_thetaB_contact_in together with a single-field tilt module is outside the device path");
  if ((p->modules & MS_MOD_RIM_SLOPE_MATCH_OUT) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the rim_slope_match_out module is not sharded (single GPU only)");
  if ((p->modules & MS_MOD_RIM_SLOPE_MATCH_OUT) && (p->modules & MS_TILT_MODS))
    return fail(c, MS_ERR_STATE, "rim_slope_match_out together with a single-field tilt module is outside the device path");
  if ((p->modules & MS_MOD_TILT_COUPLING) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the tilt_coupling module is not sharded (single GPU only)");
  if ((p->modules & MS_MOD_TILT_COUPLING) && (p->modules & MS_TILT_MODS))
    return fail(c, MS_ERR_STATE, "tilt_coupling together with a single-field tilt module is outside the device path");
  if ((p->modules & MS_MOD_TILT_SPLAY_TWIST_IN) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the tilt_splay_twist_in module is not sharded (single GPU only)");
  if ((p->modules & MS_MOD_TILT_SPLAY_TWIST_IN) && (p->modules & MS_TILT_MODS))
    return fail(c, MS_ERR_STATE, "tilt_splay_twist_in together with a single-field tilt module is outside the device path");
  if ((p->modules & MS_MOD_BENDING_TILT) && !c->d_bt_vert) {
    const size_t bytes = sizeof(double) * 4 * (size_t)c->til.nvp;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_bt_vert), bytes));
    HIPCHK(c, hipMemset(c->d_bt_vert, 0, bytes));
  }
  if ((p->modules & MS_CON_BODY_AREA) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the body_area constraint row is not sharded (single GPU only)");
  if ((p->modules & MS_CON_BODY_AREA) && (p->modules & MS_ANY_TILT_MODS))
    return fail(c, MS_ERR_STATE, "the body_area constraint row together with a tilt-family module is outside the device path");
  if ((p->modules & MS_CON_BODY_AREA) && (p->modules & MS_MOD_AREA_PENALTY))
    return fail(c, MS_ERR_STATE, "the body_area constraint row together with body_area_penalty is outside the device path");
  c->params = *p;
  // (no kernel reads the bit: the row is the area lane's own, ms_api_area_con.inc)
  c->area_row = (p->modules & MS_CON_BODY_AREA) != 0;
  c->params.modules &= ~MS_CON_BODY_AREA;
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return MS_OK;
}

int ms_set_area_penalty(ms_ctx* c, double stiffness, double target_area) {
  if (!c) return MS_ERR_INVALID;
  if (!std::isfinite(stiffness) || !std::isfinite(target_area))
    return fail(c, MS_ERR_INVALID, "ms_set_area_penalty: stiffness and target area must be finite");
  c->area_stiffness = stiffness;
  c->target_area = target_area;
  c->carry.invalidate();  // (the energies and the gradient held are the old term's)
  c->sh_carry_valid = c->sh_grad_valid = false;
  return MS_OK;
}

int ms_get_body_area(ms_ctx* c, double* area) {
  if (!c || !area) return fail(c, MS_ERR_INVALID, "ms_get_body_area: NULL argument");
  if (!(c->params.modules & MS_MOD_AREA_PENALTY))
    return fail(c, MS_ERR_STATE, "ms_get_body_area: MS_MOD_AREA_PENALTY is not in the module mask");
  int rc = fetch(c);
  if (rc) return rc;
  *area = c->h_scal[MS_S_AREA];
  return MS_OK;
}

int ms_set_tilts(ms_ctx* c, const double* tilts, double tilt_rigidity) {
  if (!c || !tilts) return fail(c, MS_ERR_INVALID, "ms_set_tilts: NULL argument");
  const size_t bytes = sizeof(double) * 3 * (size_t)c->til.nvp;
  if (!c->tf[0].tilts) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->tf[0].tilts), bytes));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->tf[0].grad), bytes));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->tf[0].trial), bytes));
    HIPCHK(c, hipMemset(c->tf[0].trial, 0, bytes));
    HIPCHK(c, hipMemset(c->tf[0].tilts, 0, bytes));
    HIPCHK(c, hipMemset(c->tf[0].grad, 0, bytes));
  }
  c->tf[0].k_tilt = tilt_rigidity;
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return ext_to_patch(c, tilts, c->tf[0].tilts, 3);
}

int ms_get_tilts(ms_ctx* c, double* tilts) {
  if (!c || !tilts || !c->tf[0].tilts) return fail(c, MS_ERR_INVALID, "ms_get_tilts: no tilts set");
  return patch_to_ext(c, c->tf[0].tilts, tilts, 3);
}

int ms_get_tilt_gradient(ms_ctx* c, double* tilt_grad) {
  if (!c || !tilt_grad || !c->tf[0].grad) return fail(c, MS_ERR_INVALID, "ms_get_tilt_gradient: no tilts set");
  return patch_to_ext(c, c->tf[0].grad, tilt_grad, 3);
}

int ms_angle_defects(ms_ctx* c, double* defects) {
  if (!c || !defects) return fail(c, MS_ERR_INVALID, "ms_angle_defects: NULL argument");
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_angle_defects: single shard only");
  const Tiling& t = c->til;
  double* d_out = nullptr;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(double) * (size_t)std::max<int64_t>(1, t.nvp)));
  HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)std::max<int64_t>(1, t.nvp), S(c)));
  TiltArgs a;
  a.fields = nullptr;
  a.fields_rows = 0;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = nullptr;
  a.alpha = 0.0;
  a.tilts = c->buf[MS_BUF_X];  // (read, not used)
  a.tilts_out = nullptr;
  a.k_tilt = 0.0;
  a.g = nullptr;
  a.tilt_grad = nullptr;
  a.minv = d_out;
  a.partials = c->d_partials;
  a.e_slot = MS_S_ETILT;
  a.consistent = 0;
  a.tg_accumulate = 0;
  a.cons_tilt_grad = 0;
  a.va_out = nullptr;
  hipError_t e = launch_tilt(a, 4, c->cap, t.max_ent, c->stream);
  int rc = MS_OK;
  if (e != hipSuccess) rc = fail(c, MS_ERR_HIP, std::string("ms_angle_defects: ") + hipGetErrorString(e));
  if (rc == MS_OK) rc = patch_to_ext(c, d_out, defects, 1);
  (void)hipStreamSynchronize(S(c));
  (void)hipFree(d_out);
  return rc;
}

int ms_curvature_fields(ms_ctx* c, double* mean_curvature_normal, double* h_area_anglesum, double* defect_kg,
                        double* principal) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_curvature_fields: single shard only");
  const Tiling& t = c->til;
  const size_t plane = 3 * (size_t)std::max<int64_t>(1, t.nvp);
  double* d_out = nullptr;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(double) * 4 * plane));
  HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(double) * 4 * plane, S(c)));
  TiltArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = nullptr;
  a.alpha = 0.0;
  a.tilts = c->buf[MS_BUF_X];  // (read, not used)
  a.tilts_out = nullptr;
  a.k_tilt = 0.0;
  a.g = nullptr;
  a.tilt_grad = nullptr;
  a.minv = nullptr;
  a.partials = c->d_partials;
  a.e_slot = MS_S_ETILT;
  a.consistent = 0;
  a.tg_accumulate = 0;
  a.cons_tilt_grad = 0;
  a.va_out = nullptr;
  a.fields = d_out;
  a.fields_rows = t.nvp;
  hipError_t e = launch_tilt(a, 5, c->cap, t.max_ent, c->stream);
  int rc = MS_OK;
  if (e != hipSuccess) rc = fail(c, MS_ERR_HIP, std::string("ms_curvature_fields: ") + hipGetErrorString(e));
  double* outs[4] = {mean_curvature_normal, h_area_anglesum, defect_kg, principal};
  for (int k = 0; k < 4 && rc == MS_OK; ++k)
    if (outs[k]) rc = patch_to_ext(c, d_out + (size_t)k * plane, outs[k], 3);
  (void)hipStreamSynchronize(S(c));
  (void)hipFree(d_out);
  return rc;
}

int ms_project_tilts_to_tangent(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "tilt passes are single-shard only");
  TiltField* fl[3];
  const int n = active_fields(c, c->params.modules, fl);
  for (int k = 0; k < n; ++k) {  // every field the module set reads (geometry/mesh.py:788-814)
    int rc = tilt_pass_f(c, *fl[k], 2, false, 0.0);
    if (rc) return rc;
  }
  if (n == 0) {
    int rc = tilt_pass(c, 2, false, 0.0);
    if (rc) return rc;
  }
  return fetch(c);
}

int ms_set_deterministic(ms_ctx* c, int on) {
  if (!c) return MS_ERR_INVALID;
  if (c->deterministic == (on != 0)) return MS_OK;
  c->deterministic = on != 0;
  c->carry.invalidate_with_bt();
  c->carry.factors_valid = false;
  return MS_OK;
}

int ms_set_tilt_smoothness(ms_ctx* c, double k_smooth) {
  if (!c) return MS_ERR_INVALID;
  c->tf[0].k_smooth = k_smooth;
  c->carry.invalidate_with_bt();
  return MS_OK;
}

int ms_set_tilt_fixed(ms_ctx* c, const uint8_t* tilt_fixed) {
  if (!c) return fail(c, MS_ERR_INVALID, "ms_set_tilt_fixed: NULL context");
  const Tiling& t = c->til;
  for (int i = 0; i < t.nv; ++i) {
    uint8_t f = c->h_vflags[(size_t)i] & (uint8_t)~VF_TILT_FIXED;
    if (tilt_fixed && tilt_fixed[t.perm[i]]) f |= VF_TILT_FIXED;
    c->h_vflags[(size_t)i] = f;
  }
  c->tf[0].any_free = t.nv == 0;
  for (int i = 0; i < t.nv && !c->tf[0].any_free; ++i) c->tf[0].any_free = !(c->h_vflags[(size_t)i] & VF_TILT_FIXED);
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(c->d_vflags, c->h_vflags.data(), c->h_vflags.size(), hipMemcpyHostToDevice));
  return MS_OK;
}
