// libmembrane_hip.so device side, part of ms_kernels.hip (included there, inside namespace ms).
// ---------------------------------------------------------------------------
// k_tsearch: the backtracking search of a tilt relaxation (runtime/steppers/tilt_relaxation.py:326-347, 380-398,
// 918-973, 1150-1230) tries step, step/2, ... on E(P(t + step*src)) with the POSITIONS FROZEN.  One trial used to be
// k_tvec mode 2 (write the trial field) + one energy-only launch per module and field + a fold + a host poll.  This
// pass evaluates n_trials step sizes of the ladder for every tilt-reading module of up to two fields in ONE sweep over
// the facets: the geometry of a facet (P1 gradients, cotans, effective corner areas) is formed once, the trial rows
// where they are used, and trial j's per-tile partials land in partial set j, slot for slot what the single-trial
// kernels leave there:
//   bending_tilt (+ leaflet forms)  k_bt<0>       1/2 sum kappa_k (base_k + s div_f t)^2 va_eff[f,k]
//   tilt, per-facet form            k_bt<0> fused 1/2 k_t (sum |t_k|^2 / 3) A_f
//   tilt, vertex-area form          k_tvec mode 4 1/2 k_t sum_v |t_v|^2 A_v   (leaflet driver, positions frozen)
//   tilt_smoothness                 k_tsmooth<0>  k_s/4 sum_f [c0|t1-t2|^2 + c1|t2-t0|^2 + c2|t0-t1|^2]
// with the same per-thread facet assignment, the same expressions and the same block reduction: a trial's energies are
// the doubles the separate launches produce (tests/test_gpu_tsearch.py compares them bit for bit).
// LDS: px[3][cap] | nr[3][cap] (NT > 1) | per field: tl[3][cap] (NT == 1: the trial rows themselves) | sr[3][cap]
//      (NT > 1) | bs[cap] | kp[cap] || red[NF*NT*3][8] | lfl[cap]
// ---------------------------------------------------------------------------
template <int NF, int NT>
__device__ __forceinline__ void tsearch_body(const TsearchArgs& a, int cap, double* lds, int block_id) {
  constexpr int PERV_F = 3 + (NT > 1 ? 3 : 0) + 2;  // doubles per staged vertex and field
  constexpr int NVAL = NF * NT * 3;
  const int T = a.m.T;
  double* px = lds;
  double* nr = px + 3 * cap;
  double* fbase = nr + (NT > 1 ? 3 * cap : 0);
  double* red = fbase + (size_t)NF * PERV_F * cap;
  uint8_t* lfl = reinterpret_cast<uint8_t*>(red + NVAL * 8);
  auto f_tl = [&](int fi) { return fbase + (size_t)fi * PERV_F * cap; };
  auto f_sr = [&](int fi) { return f_tl(fi) + 3 * cap; };
  auto f_bs = [&](int fi) { return f_tl(fi) + (NT > 1 ? 6 : 3) * cap; };
  auto f_kp = [&](int fi) { return f_bs(fi) + cap; };

  const TileCtx t = tile_ctx(a.m, a.tile0 + xcd_tile(block_id, a.tile1 - a.tile0));
  const int tid = threadIdx.x;
  FacetRec<false> tf_nx = facet_null<false>();
  if (t.f0 + tid < t.f1) tf_nx = facet_load<false>(a.m, (size_t)(t.f0 + tid));

  // ---- stage the rows of the owned and halo vertices (all loads of a row before its LDS writes) ---------------------
  auto stage = [&](int v, int sl, bool own_row) {
    const size_t g = 3 * (size_t)v;
    const uint8_t fl = a.m.vflags[v];
    double x0 = a.x[g], x1 = a.x[g + 1], x2 = a.x[g + 2];
    const bool plain = NT == 1 && a.plain != 0;
    if (NT == 1 && a.d != nullptr) {
      const double d0 = a.d[g], d1 = a.d[g + 1], d2 = a.d[g + 2];
      if (!(fl & VF_FIXED)) {
        x0 = axpy1(x0, a.alpha, d0);
        x1 = axpy1(x1, a.alpha, d1);
        x2 = axpy1(x2, a.alpha, d2);
      }
    }
    V3 n = mk(0, 0, 0);
    if (!plain) n = mk(a.normals[g], a.normals[g + 1], a.normals[g + 2]);
    V3 tt[NF], ss[NF];
    double b[NF], k[NF];
#pragma unroll
    for (int fi = 0; fi < NF; ++fi) {
      const TsearchField& f = a.f[fi];
      tt[fi] = mk(f.tilts[g], f.tilts[g + 1], f.tilts[g + 2]);
      ss[fi] = plain ? tt[fi] : mk(f.src[g], f.src[g + 1], f.src[g + 2]);
      b[fi] = f.s_ebt >= 0 ? f.bt_vert[4 * (size_t)v] : 0.0;
      k[fi] = f.s_ebt >= 0 ? f.kappa[v] : 0.0;
    }
    px[sl] = x0;
    px[cap + sl] = x1;
    px[2 * cap + sl] = x2;
    lfl[sl] = fl;
    if (NT > 1) {
      nr[sl] = n.x;
      nr[cap + sl] = n.y;
      nr[2 * cap + sl] = n.z;
    }
#pragma unroll
    for (int fi = 0; fi < NF; ++fi) {
      V3 r = tt[fi];
      if (NT == 1 && !plain && !(fl & a.f[fi].fixed_bit)) r = tilt_trial_row(tt[fi], ss[fi], n, a.coef[0]);
      double* tl = f_tl(fi);
      tl[sl] = r.x;
      tl[cap + sl] = r.y;
      tl[2 * cap + sl] = r.z;
      if (NT == 1 && own_row && a.f[fi].trial_out != nullptr) {  // (an accepted first step size needs no k_tvec launch)
        double* o = a.f[fi].trial_out + g;
        o[0] = r.x;
        o[1] = r.y;
        o[2] = r.z;
      }
      if (NT > 1) {
        double* sr = f_sr(fi);
        sr[sl] = ss[fi].x;
        sr[cap + sl] = ss[fi].y;
        sr[2 * cap + sl] = ss[fi].z;
      }
      f_bs(fi)[sl] = b[fi];
      f_kp(fi)[sl] = k[fi];
    }
  };
  if (tid < t.n_owned) stage(t.v_lo + tid, tid, true);
  for (int h = tid; h < t.nh; h += T) stage(a.m.halo_ids[t.h0 + h], t.n_owned + h, false);
  __syncthreads();

  // trial row j of staged vertex sl of field fi
  auto trial_row = [&](int fi, int sl, int j, const V3& t0, const V3& s, const V3& n) -> V3 {
    if (NT == 1) return t0;
    if (lfl[sl] & a.f[fi].fixed_bit) return t0;
    return tilt_trial_row(t0, s, n, a.coef[j]);
  };

  double e_bt[NF][NT], e_tl[NF][NT], e_ts[NF][NT];
#pragma unroll
  for (int fi = 0; fi < NF; ++fi)
#pragma unroll
    for (int j = 0; j < NT; ++j) e_bt[fi][j] = e_tl[fi][j] = e_ts[fi][j] = 0.0;
  bool any_bt = false;
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) any_bt = any_bt || a.f[fi].s_ebt >= 0;

  for (int c0f = t.f0; c0f < t.f1; c0f += T) {
    const int p = c0f + tid;
    const TileFacet tf = facet_unpack<false>(tf_nx);
    if (p + T < t.f1) tf_nx = facet_load<false>(a.m, (size_t)(p + T));
    if (p < t.f1) {
      const bool owner = (tf.flags & TF_OWNER) != 0;
      const V3 v0 = lds_v3(px, cap, tf.l0), v1 = lds_v3(px, cap, tf.l1), v2 = lds_v3(px, cap, tf.l2);
      const V3 e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0;
      const double l0 = dot(e0, e0), l1 = dot(e1, e1), l2 = dot(e2, e2);
      const V3 n = cross(e2, -e1);
      const double n2 = dot(n, n);
      const double A2 = sqrt(n2);
      const double denom = n2 > 1.0e-20 ? n2 : 1.0e-20;
      const double i2 = 1.0 / denom;
      const V3 g0 = i2 * cross(n, e0), g1 = i2 * cross(n, e1), g2 = i2 * cross(n, e2);
      const double ad = A2 < 1.0e-12 ? 1.0e-12 : A2;
      const double inv_ad = 1.0 / ad;
      const double cc0 = dot(-e1, e2) * inv_ad, cc1 = dot(-e2, e0) * inv_ad, cc2 = dot(-e0, e1) * inv_ad;
      double ve0 = 0.0, ve1 = 0.0, ve2 = 0.0;
      if (any_bt) {  // effective corner areas, as k_bt forms them
        corner_areas(cc0, cc1, cc2, l0, l1, l2, fmax(0.5 * A2, 1.0e-12), ve0, ve1, ve2);
        int b0 = 0, b1 = 0, b2 = 0;
        if (a.m.has_boundary) {
          b0 = (lfl[tf.l0] & VF_BOUNDARY) ? 1 : 0;
          b1 = (lfl[tf.l1] & VF_BOUNDARY) ? 1 : 0;
          b2 = (lfl[tf.l2] & VF_BOUNDARY) ? 1 : 0;
        }
        const int n_int = 3 - (b0 + b1 + b2);
        if (n_int > 0 && n_int < 3) {
          const double b_sum = ve0 * b0 + ve1 * b1 + ve2 * b2;
          const double extra = b_sum / (double)n_int;
          const double m0 = b0 ? 0.0 : 1.0, m1 = b1 ? 0.0 : 1.0, m2 = b2 ? 0.0 : 1.0;
          ve0 = ve0 * m0 + m0 * extra;
          ve1 = ve1 * m1 + m1 * extra;
          ve2 = ve2 * m2 + m2 * extra;
        }
      }
      V3 n0 = mk(0, 0, 0), n1 = n0, n2r = n0;
      if (NT > 1) {
        n0 = lds_v3(nr, cap, tf.l0);
        n1 = lds_v3(nr, cap, tf.l1);
        n2r = lds_v3(nr, cap, tf.l2);
      }
#pragma unroll
      for (int fi = 0; fi < NF; ++fi) {
        const TsearchField& f = a.f[fi];
        const double* tl = f_tl(fi);
        const V3 b0r = lds_v3(tl, cap, tf.l0), b1r = lds_v3(tl, cap, tf.l1), b2r = lds_v3(tl, cap, tf.l2);
        V3 s0 = mk(0, 0, 0), s1 = s0, s2 = s0;
        if (NT > 1) {
          const double* sr = f_sr(fi);
          s0 = lds_v3(sr, cap, tf.l0);
          s1 = lds_v3(sr, cap, tf.l1);
          s2 = lds_v3(sr, cap, tf.l2);
        }
        const bool bt_on = f.s_ebt >= 0, ts_on = f.s_ets >= 0, facet_tilt = f.tilt_form == 1;
        double kb0 = 0, kb1 = 0, kb2 = 0, bs0 = 0, bs1 = 0, bs2 = 0;
        if (bt_on) {
          const double* bs = f_bs(fi);
          const double* kp = f_kp(fi);
          bs0 = bs[tf.l0]; bs1 = bs[tf.l1]; bs2 = bs[tf.l2];
          kb0 = kp[tf.l0]; kb1 = kp[tf.l1]; kb2 = kp[tf.l2];
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const V3 tt0 = trial_row(fi, tf.l0, j, b0r, s0, n0), tt1 = trial_row(fi, tf.l1, j, b1r, s1, n1),
                   tt2 = trial_row(fi, tf.l2, j, b2r, s2, n2r);
          if (bt_on) {
            const double dv = f.div_sign * (dot(tt0, g0) + dot(tt1, g1) + dot(tt2, g2));
            const double t0 = bs0 + dv, t1 = bs1 + dv, t2 = bs2 + dv;
            if (owner) e_bt[fi][j] += 0.5 * ((kb0 * (t0 * t0) * ve0 + kb1 * (t1 * t1) * ve1) + kb2 * (t2 * t2) * ve2);
          }
          if (facet_tilt && f.k_tilt != 0.0 && A2 >= 1.0e-12 && owner) {
            const double sq = (dot(tt0, tt0) + dot(tt1, tt1)) + dot(tt2, tt2);
            const double coeff = 0.5 * f.k_tilt * (sq / 3.0);
            e_tl[fi][j] += coeff * (0.5 * A2);
          }
          if (ts_on) {
            const V3 d12 = tt1 - tt2, d20 = tt2 - tt0, d01 = tt0 - tt1;
            if (owner)
              e_ts[fi][j] += 0.25 * f.k_smooth * ((cc0 * dot(d12, d12) + cc1 * dot(d20, d20)) + cc2 * dot(d01, d01));
          }
        }
      }
    }
  }
  // vertex-area form of the tilt magnitude: one term per owned row (k_tvec mode 4)
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) {
    const TsearchField& f = a.f[fi];
    if (f.tilt_form != 2 || tid >= t.n_owned) continue;
    const double av = f.va[t.v_lo + tid];
    const V3 b = lds_v3(f_tl(fi), cap, tid);
    V3 s = mk(0, 0, 0), n = s;
    if (NT > 1) {
      s = lds_v3(f_sr(fi), cap, tid);
      n = lds_v3(nr, cap, tid);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const V3 tv = trial_row(fi, tid, j, b, s, n);
      e_tl[fi][j] = 0.0 + (dot(tv, tv)) * av;
    }
  }
  // ---- block sums (wave sums, then the waves in order: block_reduce_store's arithmetic) and the partial stores --------
  const int lane = tid & 63, w = tid >> 6;
  const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int fi = 0; fi < NF; ++fi)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double r0 = wave_sum(e_bt[fi][j]), r1 = wave_sum(e_tl[fi][j]), r2 = wave_sum(e_ts[fi][j]);
      if (lane == 0) {
        double* rr = red + ((fi * NT + j) * 3) * 8;
        rr[w] = r0;
        rr[8 + w] = r1;
        rr[16 + w] = r2;
      }
    }
  __syncthreads();
  if (tid < NVAL) {
    const int fi = tid / (NT * 3), j = (tid / 3) % NT, q = tid % 3;
    int slot = -1, form = 0;
    double kt = 0.0;
#pragma unroll
    for (int ff = 0; ff < NF; ++ff)
      if (ff == fi) {
        const TsearchField& f = a.f[ff];
        slot = q == 0 ? f.s_ebt : (q == 1 ? (f.tilt_form != 0 ? f.s_etilt : -1) : f.s_ets);
        form = f.tilt_form;
        kt = f.k_tilt;
      }
    double* out = nullptr;
#pragma unroll
    for (int jj = 0; jj < NT; ++jj)
      if (jj == j) out = a.partials[jj];
    if (slot >= 0 && j < a.n_trials && out != nullptr) {
      const double* rr = red + tid * 8;
      double r = rr[0];
      for (int i = 1; i < nw; ++i) r = r + rr[i];
      if (q == 1 && form == 2) r = (0.5 * kt) * r;
      out[(size_t)slot * a.m.n_tiles + t.tile] = r;
    }
  }
}

template <int NF, int NT>
__global__ __launch_bounds__(512) void k_tsearch(TsearchArgs a, int cap) {
  extern __shared__ double lds[];
  tsearch_body<NF, NT>(a, cap, lds, (int)blockIdx.x);
}

size_t tsearch_lds_bytes(int cap, int n_fields, int n_trials) {
  const int nt = n_trials <= 1 ? 1 : (n_trials <= 2 ? 2 : (n_trials <= 4 ? 4 : 8));
  const size_t per_f = 3 + (nt > 1 ? 3 : 0) + 2;
  const size_t perv = 3 + (nt > 1 ? 3 : 0) + (size_t)n_fields * per_f;
  return (perv * (size_t)cap + (size_t)n_fields * nt * 3 * 8) * sizeof(double) + (((size_t)cap + 15) / 16) * 16;
}

hipError_t launch_tsearch(const TsearchArgs& a, int cap, hipStream_t s) {
  const int nb = a.tile1 - a.tile0;
  if (nb <= 0) return hipSuccess;
  if (a.n_fields < 1 || a.n_fields > 2 || a.n_trials < 1 || a.n_trials > MS_MAX_TRIALS || a.m.T > 512)
    return hipErrorInvalidValue;
  const size_t lds = tsearch_lds_bytes(cap, a.n_fields, a.n_trials);
  // (the one-workgroup interpreter runs the single-step-size form: an energy-only evaluation's tilt-module pass)
  if (ExecRecorder* r = exec_find(s)) {
    if (a.n_trials != 1) return hipErrorInvalidValue;
    return r->push(CK_TSEARCH, a.n_fields, cap, 0, nb, 0, lds, &a, sizeof(a), &a.m);
  }
  const int nt = a.n_trials <= 1 ? 1 : (a.n_trials <= 2 ? 2 : (a.n_trials <= 4 ? 4 : 8));
  return pick_int<1, 2>(a.n_fields, [&](auto NF) {
    return pick_int<1, 2, 4, 8>(nt, [&](auto NT) {
      return launch(k_tsearch<decltype(NF)::value, decltype(NT)::value>, nb, a.m.T, lds, s, a, cap);
    });
  });
}

// ---------------------------------------------------------------------------
// k_tgrad: the other evaluation of a relaxation step -- energy AND tilt gradients at the current tilts, positions
// frozen (tilt_relaxation.py:312-318, 352-369, 892-917, 1059-1141) -- for every tilt-reading module of up to two
// fields in one sweep, followed on the owned rows by what k_tvec mode 0 does to the finished gradient (clamped rows
// zeroed, |g|^2 and <r, M^-1 r> partials).  It replaces, per field, the tilt-magnitude pass (k_tilt<1> / k_tvec mode 4),
// k_bt<2>, k_tsmooth<1> and k_tvec mode 0, and leaves the doubles they leave: every module's per-corner terms are
// staged and gathered on their own, in the CSR order, and added to the row in the module order
// (tilt, bending_tilt, smoothness).
// LDS: px[3][cap] | per field: tl[3][cap] | bs[cap] | kp[cap] || stg[10][T] | red[NF*5][8] | vent | lfl
// ---------------------------------------------------------------------------
template <int NF, bool ATOMIC>
__device__ __forceinline__ void tgrad_body(const TgradArgs& a, int cap, int max_ent, double* lds, int block_id) {
  constexpr int NVAL = NF * 5;
  const int T = a.m.T;
  double* px = lds;
  double* fbase = px + 3 * cap;
  double* stg = fbase + (size_t)NF * 5 * cap;
  // ATOMIC: stg holds per-vertex accumulators (ds_add_f64) -- acc[field][xyz][T], then one area column per field when a
  // field has the per-facet tilt form -- instead of per-corner columns, and there is no CSR
  bool need_a3 = false;
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) need_a3 = need_a3 || a.f[fi].tilt_form == 1;
  const int n_acc = NF * 3 + (need_a3 ? NF : 0);
  double* red = stg + (ATOMIC ? n_acc : 10) * T;
  uint16_t* vent = reinterpret_cast<uint16_t*>(red + NVAL * 8);
  uint8_t* lfl = reinterpret_cast<uint8_t*>(vent + (ATOMIC ? 0 : ((max_ent + 3) & ~3)));
  auto f_tl = [&](int fi) { return fbase + (size_t)fi * 5 * cap; };
  auto f_bs = [&](int fi) { return f_tl(fi) + 3 * cap; };
  auto f_kp = [&](int fi) { return f_bs(fi) + cap; };

  const TileCtx t = tile_ctx(a.m, a.tile0 + xcd_tile(block_id, a.tile1 - a.tile0));
  const int tid = threadIdx.x;
  const bool own = tid < t.n_owned;
  FacetRec<false> tf_nx = facet_null<false>();
  if (t.f0 + tid < t.f1) tf_nx = facet_load<false>(a.m, (size_t)(t.f0 + tid));
  CsrStage cs;
  cs.vo0 = cs.vo1 = 0;
  if (!ATOMIC) csr_issue(cs, a.m, t, T, tid);
  else
    for (int i = tid; i < n_acc * T; i += T) stg[i] = 0.0;
  V3 tv[NF];
  uint8_t own_fl = 0;
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) tv[fi] = mk(0, 0, 0);
  auto stage = [&](int v, int sl, bool own_row) {
    const size_t g = 3 * (size_t)v;
    const uint8_t fl = a.m.vflags[v];
    const double x0 = a.x[g], x1 = a.x[g + 1], x2 = a.x[g + 2];
    V3 tt[NF];
    double b[NF], k[NF];
#pragma unroll
    for (int fi = 0; fi < NF; ++fi) {
      const TgradField& f = a.f[fi];
      tt[fi] = mk(f.tilts[g], f.tilts[g + 1], f.tilts[g + 2]);
      b[fi] = f.s_ebt >= 0 ? f.bt_vert[4 * (size_t)v] : 0.0;
      k[fi] = f.s_ebt >= 0 ? f.kappa[v] : 0.0;
    }
    px[sl] = x0;
    px[cap + sl] = x1;
    px[2 * cap + sl] = x2;
    lfl[sl] = fl;
    if (own_row) own_fl = fl;
#pragma unroll
    for (int fi = 0; fi < NF; ++fi) {
      double* tl = f_tl(fi);
      tl[sl] = tt[fi].x;
      tl[cap + sl] = tt[fi].y;
      tl[2 * cap + sl] = tt[fi].z;
      f_bs(fi)[sl] = b[fi];
      f_kp(fi)[sl] = k[fi];
      if (own_row) tv[fi] = tt[fi];
    }
  };
  if (own) stage(t.v_lo + tid, tid, true);
  for (int h = tid; h < t.nh; h += T) stage(a.m.halo_ids[t.h0 + h], t.n_owned + h, false);
  if (!ATOMIC) csr_commit(cs, a.m, t, T, tid, vent);
  __syncthreads();

  double e_bt[NF], e_tl[NF], e_ts[NF];
  V3 gb[NF], gs[NF];   // gathered bending_tilt / smoothness tilt gradients of the owned row
  double aw[NF];       // gathered barycentric vertex area (tilt_form 1)
  int cur_b[NF], cur_s[NF];
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) {
    e_bt[fi] = e_tl[fi] = e_ts[fi] = aw[fi] = 0.0;
    gb[fi] = gs[fi] = mk(0, 0, 0);
    cur_b[fi] = cur_s[fi] = own ? cs.vo0 : 0;
  }
  const int end = own ? cs.vo1 : 0;
  bool any_bt = false;
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) any_bt = any_bt || a.f[fi].s_ebt >= 0;

  for (int c0f = t.f0; c0f < t.f1; c0f += T) {
    const int p = c0f + tid;
    const TileFacet tf = facet_unpack<false>(tf_nx);
    if (p + T < t.f1) tf_nx = facet_load<false>(a.m, (size_t)(p + T));
    const bool live = p < t.f1;
    const bool owner = live && (tf.flags & TF_OWNER) != 0;
    V3 g0 = mk(0, 0, 0), g1 = g0, g2 = g0;
    double cc0 = 0, cc1 = 0, cc2 = 0, ve0 = 0, ve1 = 0, ve2 = 0, A2 = 0;
    if (live) {
      const V3 v0 = lds_v3(px, cap, tf.l0), v1 = lds_v3(px, cap, tf.l1), v2 = lds_v3(px, cap, tf.l2);
      const V3 e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0;
      const double l0 = dot(e0, e0), l1 = dot(e1, e1), l2 = dot(e2, e2);
      const V3 n = cross(e2, -e1);
      const double n2 = dot(n, n);
      A2 = sqrt(n2);
      const double denom = n2 > 1.0e-20 ? n2 : 1.0e-20;
      const double i2 = 1.0 / denom;
      g0 = i2 * cross(n, e0);
      g1 = i2 * cross(n, e1);
      g2 = i2 * cross(n, e2);
      const double ad = A2 < 1.0e-12 ? 1.0e-12 : A2;
      const double inv_ad = 1.0 / ad;
      cc0 = dot(-e1, e2) * inv_ad;
      cc1 = dot(-e2, e0) * inv_ad;
      cc2 = dot(-e0, e1) * inv_ad;
      if (any_bt) {
        corner_areas(cc0, cc1, cc2, l0, l1, l2, fmax(0.5 * A2, 1.0e-12), ve0, ve1, ve2);
        int b0 = 0, b1 = 0, b2 = 0;
        if (a.m.has_boundary) {
          b0 = (lfl[tf.l0] & VF_BOUNDARY) ? 1 : 0;
          b1 = (lfl[tf.l1] & VF_BOUNDARY) ? 1 : 0;
          b2 = (lfl[tf.l2] & VF_BOUNDARY) ? 1 : 0;
        }
        const int n_int = 3 - (b0 + b1 + b2);
        if (n_int > 0 && n_int < 3) {
          const double b_sum = ve0 * b0 + ve1 * b1 + ve2 * b2;
          const double extra = b_sum / (double)n_int;
          const double m0 = b0 ? 0.0 : 1.0, m1 = b1 ? 0.0 : 1.0, m2 = b2 ? 0.0 : 1.0;
          ve0 = ve0 * m0 + m0 * extra;
          ve1 = ve1 * m1 + m1 * extra;
          ve2 = ve2 * m2 + m2 * extra;
        }
      }
    }
    const int lo = c0f - t.f0, hi = min(c0f + T, t.f1) - t.f0;
#pragma unroll
    for (int fi = 0; fi < NF; ++fi) {
      const TgradField& f = a.f[fi];
      const bool bt_on = f.s_ebt >= 0, ts_on = f.s_ets >= 0;
      V3 tt0 = mk(0, 0, 0), tt1 = tt0, tt2 = tt0;
      if (live) {
        const double* tl = f_tl(fi);
        tt0 = lds_v3(tl, cap, tf.l0);
        tt1 = lds_v3(tl, cap, tf.l1);
        tt2 = lds_v3(tl, cap, tf.l2);
      }
      if (ATOMIC) {
        // default mode: a corner's bending_tilt and smoothness terms are added and go to the owned vertex's accumulator
        // by LDS atomics, as the shape gradient's do (K_C): no staging round, no barrier inside the sweep, no CSR; the
        // order of a vertex's sum is not fixed (MS_DETERMINISTIC=1 keeps the per-module launches' order)
        if (live) {
          V3 q0 = mk(0, 0, 0), q1 = q0, q2 = q0;
          double a3 = 0.0;
          if (bt_on) {
            const double* bs = f_bs(fi);
            const double* kp = f_kp(fi);
            const double dv = f.div_sign * (dot(tt0, g0) + dot(tt1, g1) + dot(tt2, g2));
            const double t0 = bs[tf.l0] + dv, t1 = bs[tf.l1] + dv, t2 = bs[tf.l2] + dv;
            const double k0 = kp[tf.l0], k1 = kp[tf.l1], k2 = kp[tf.l2];
            if (owner) e_bt[fi] += 0.5 * ((k0 * (t0 * t0) * ve0 + k1 * (t1 * t1) * ve1) + k2 * (t2 * t2) * ve2);
            const double dE = f.div_sign * ((k0 * t0 * ve0 + k1 * t1 * ve1) + k2 * t2 * ve2);
            q0 = dE * g0;
            q1 = dE * g1;
            q2 = dE * g2;
            if (f.tilt_form == 1 && A2 >= 1.0e-12) {
              const double area = 0.5 * A2;
              const double sq = (dot(tt0, tt0) + dot(tt1, tt1)) + dot(tt2, tt2);
              const double coeff = 0.5 * f.k_tilt * (sq / 3.0);
              if (owner) e_tl[fi] += coeff * area;
              a3 = area / 3.0;
            }
          }
          if (ts_on) {
            const double hk = 0.5 * f.k_smooth;
            const V3 d12 = tt1 - tt2, d20 = tt2 - tt0, d01 = tt0 - tt1;
            if (owner) e_ts[fi] += 0.25 * f.k_smooth * ((cc0 * dot(d12, d12) + cc1 * dot(d20, d20)) + cc2 * dot(d01, d01));
            q0 = q0 + hk * (cc2 * d01 - cc1 * d20);
            q1 = q1 + hk * (cc0 * d12 - cc2 * d01);
            q2 = q2 + hk * (cc1 * d20 - cc0 * d12);
          }
          const int no = t.n_owned;
          double* acc = stg + (size_t)(fi * 3) * T;
          if (tf.l0 < no) { atomicAdd(&acc[tf.l0], q0.x); atomicAdd(&acc[T + tf.l0], q0.y); atomicAdd(&acc[2 * T + tf.l0], q0.z); }
          if (tf.l1 < no) { atomicAdd(&acc[tf.l1], q1.x); atomicAdd(&acc[T + tf.l1], q1.y); atomicAdd(&acc[2 * T + tf.l1], q1.z); }
          if (tf.l2 < no) { atomicAdd(&acc[tf.l2], q2.x); atomicAdd(&acc[T + tf.l2], q2.y); atomicAdd(&acc[2 * T + tf.l2], q2.z); }
          if (f.tilt_form == 1 && a3 != 0.0) {
            double* ac3 = stg + (size_t)(NF * 3 + fi) * T;
            if (tf.l0 < no) atomicAdd(&ac3[tf.l0], a3);
            if (tf.l1 < no) atomicAdd(&ac3[tf.l1], a3);
            if (tf.l2 < no) atomicAdd(&ac3[tf.l2], a3);
          }
        }
        continue;
      }
      if (bt_on) {  // ---- bending_tilt: k_bt<2>'s staged terms (+ the facet's area third for the per-facet tilt form)
        if (live) {
          const double* bs = f_bs(fi);
          const double* kp = f_kp(fi);
          const double dv = f.div_sign * (dot(tt0, g0) + dot(tt1, g1) + dot(tt2, g2));
          const double t0 = bs[tf.l0] + dv, t1 = bs[tf.l1] + dv, t2 = bs[tf.l2] + dv;
          const double k0 = kp[tf.l0], k1 = kp[tf.l1], k2 = kp[tf.l2];
          if (owner) e_bt[fi] += 0.5 * ((k0 * (t0 * t0) * ve0 + k1 * (t1 * t1) * ve1) + k2 * (t2 * t2) * ve2);
          const double dE = f.div_sign * ((k0 * t0 * ve0 + k1 * t1 * ve1) + k2 * t2 * ve2);
          double* s = stg + tid;
          s[0 * T] = dE * g0.x; s[1 * T] = dE * g0.y; s[2 * T] = dE * g0.z;
          s[3 * T] = dE * g1.x; s[4 * T] = dE * g1.y; s[5 * T] = dE * g1.z;
          s[6 * T] = dE * g2.x; s[7 * T] = dE * g2.y; s[8 * T] = dE * g2.z;
          double a3 = 0.0;
          if (f.tilt_form == 1 && A2 >= 1.0e-12) {  // k_tilt<1>: E = coeff A_f, vertex area thirds
            const double area = 0.5 * A2;
            const double sq = (dot(tt0, tt0) + dot(tt1, tt1)) + dot(tt2, tt2);
            const double coeff = 0.5 * f.k_tilt * (sq / 3.0);
            if (owner) e_tl[fi] += coeff * area;
            a3 = area / 3.0;
          }
          s[9 * T] = a3;
        }
        __syncthreads();
        while (cur_b[fi] < end) {
          const int ent = vent[cur_b[fi]];
          const int fl = ent >> 2;
          if (fl >= hi) break;
          const int k = ent & 3;
          const double* s = stg + (fl - lo);
          gb[fi].x += s[(3 * k) * T];
          gb[fi].y += s[(3 * k + 1) * T];
          gb[fi].z += s[(3 * k + 2) * T];
          aw[fi] += s[9 * T];
          ++cur_b[fi];
        }
        __syncthreads();
      }
      if (ts_on) {  // ---- smoothness: k_tsmooth<1>'s staged terms
        if (live) {
          const double hk = 0.5 * f.k_smooth;
          const V3 d12 = tt1 - tt2, d20 = tt2 - tt0, d01 = tt0 - tt1;
          if (owner) e_ts[fi] += 0.25 * f.k_smooth * ((cc0 * dot(d12, d12) + cc1 * dot(d20, d20)) + cc2 * dot(d01, d01));
          const V3 q0 = hk * (cc2 * d01 - cc1 * d20);
          const V3 q1 = hk * (cc0 * d12 - cc2 * d01);
          const V3 q2 = hk * (cc1 * d20 - cc0 * d12);
          double* s = stg + tid;
          s[0 * T] = q0.x; s[1 * T] = q0.y; s[2 * T] = q0.z;
          s[3 * T] = q1.x; s[4 * T] = q1.y; s[5 * T] = q1.z;
          s[6 * T] = q2.x; s[7 * T] = q2.y; s[8 * T] = q2.z;
        }
        __syncthreads();
        while (cur_s[fi] < end) {
          const int ent = vent[cur_s[fi]];
          const int fl = ent >> 2;
          if (fl >= hi) break;
          const int k = ent & 3;
          const double* s = stg + (fl - lo);
          gs[fi].x += s[(3 * k) * T];
          gs[fi].y += s[(3 * k + 1) * T];
          gs[fi].z += s[(3 * k + 2) * T];
          ++cur_s[fi];
        }
        __syncthreads();
      }
    }
  }
  if (ATOMIC) {
    __syncthreads();
    if (own) {
#pragma unroll
      for (int fi = 0; fi < NF; ++fi) {
        const double* acc = stg + (size_t)(fi * 3) * T;
        gb[fi] = mk(acc[tid], acc[T + tid], acc[2 * T + tid]);
        if (a.f[fi].tilt_form == 1) aw[fi] = stg[(size_t)(NF * 3 + fi) * T + tid];
      }
    }
  }
  // ---- the owned row: module sums in module order, then k_tvec mode 0 -----------------------------------------------
  double gn2[NF], rz[NF];
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) {
    const TgradField& f = a.f[fi];
    gn2[fi] = rz[fi] = 0.0;
    if (!own) continue;
    const int v = t.v_lo + tid;
    const size_t o = 3 * (size_t)v;
    V3 g = mk(0, 0, 0);
    if (f.tilt_form == 2) {
      const double av = f.va[v];
      e_tl[fi] = 0.0 + (dot(tv[fi], tv[fi])) * av;
      g = mk(f.k_tilt * tv[fi].x * av, f.k_tilt * tv[fi].y * av, f.k_tilt * tv[fi].z * av);
    } else if (f.tilt_form == 1) {
      g = mk(f.k_tilt * tv[fi].x * aw[fi], f.k_tilt * tv[fi].y * aw[fi], f.k_tilt * tv[fi].z * aw[fi]);
    }
    if (ATOMIC) {
      if (f.s_ebt >= 0 || f.s_ets >= 0) g = mk(g.x + gb[fi].x, g.y + gb[fi].y, g.z + gb[fi].z);
    } else {
      if (f.s_ebt >= 0) g = mk(g.x + gb[fi].x, g.y + gb[fi].y, g.z + gb[fi].z);
      if (f.s_ets >= 0) g = mk(g.x + gs[fi].x, g.y + gs[fi].y, g.z + gs[fi].z);
    }
    if (own_fl & f.fixed_bit) g = mk(0, 0, 0);
    f.grad[o] = g.x;
    f.grad[o + 1] = g.y;
    f.grad[o + 2] = g.z;
    const double gg = dot_pinned(g, g);
    gn2[fi] = 0.0 + gg;
    rz[fi] = 0.0 + gg * f.minv[v];
  }
  const int lane = tid & 63, w = tid >> 6;
  const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int fi = 0; fi < NF; ++fi) {
    const double r0 = wave_sum(e_bt[fi]), r1 = wave_sum(e_tl[fi]), r2 = wave_sum(e_ts[fi]), r3 = wave_sum(gn2[fi]),
                 r4 = wave_sum(rz[fi]);
    if (lane == 0) {
      double* rr = red + (fi * 5) * 8;
      rr[w] = r0;
      rr[8 + w] = r1;
      rr[16 + w] = r2;
      rr[24 + w] = r3;
      rr[32 + w] = r4;
    }
  }
  __syncthreads();
  if (tid < NVAL) {
    const int fi = tid / 5, q = tid % 5;
    int slot = -1, form = 0;
    double kt = 0.0;
#pragma unroll
    for (int ff = 0; ff < NF; ++ff)
      if (ff == fi) {
        const TgradField& f = a.f[ff];
        slot = q == 0 ? f.s_ebt : (q == 1 ? (f.tilt_form != 0 ? f.s_etilt : -1) : (q == 2 ? f.s_ets : (q == 3 ? f.s_gn2 : f.s_rz)));
        form = f.tilt_form;
        kt = f.k_tilt;
      }
    if (slot >= 0) {
      const double* rr = red + tid * 8;
      double r = rr[0];
      for (int i = 1; i < nw; ++i) r = r + rr[i];
      if (q == 1 && form == 2) r = (0.5 * kt) * r;
      a.partials[(size_t)slot * a.m.n_tiles + t.tile] = r;
    }
  }
}

template <int NF, bool ATOMIC>
__global__ __launch_bounds__(512) void k_tgrad(TgradArgs a, int cap, int max_ent) {
  extern __shared__ double lds[];
  tgrad_body<NF, ATOMIC>(a, cap, max_ent, lds, (int)blockIdx.x);
}

size_t tgrad_lds_bytes(int T, int cap, int max_ent, int n_fields, bool atomic, bool need_a3) {
  const size_t cols = atomic ? (size_t)n_fields * (need_a3 ? 4 : 3) : 10;
  return ((3 + 5 * (size_t)n_fields) * (size_t)cap + cols * (size_t)T + (size_t)n_fields * 5 * 8) * sizeof(double) +
         (atomic ? 0 : 2 * ((size_t)((max_ent + 3) & ~3))) + (((size_t)cap + 15) / 16) * 16;
}

hipError_t launch_tgrad(const TgradArgs& a, int cap, int max_ent, bool combine, hipStream_t s) {
  const int nb = a.tile1 - a.tile0;
  if (nb <= 0) return hipSuccess;
  if (a.n_fields < 1 || a.n_fields > 2 || a.m.T > 512) return hipErrorInvalidValue;
  if (hipError_t es_ = exec_sync(s); es_ != hipSuccess) return es_;  // (not recorded: runs behind what was)
  bool need_a3 = false;
  for (int k = 0; k < a.n_fields; ++k) need_a3 = need_a3 || a.f[k].tilt_form == 1;
  const size_t lds = tgrad_lds_bytes(a.m.T, cap, max_ent, a.n_fields, combine, need_a3);
  return pick_int<1, 2>(a.n_fields, [&](auto NF) {
    return pick(combine, [&](auto CB) {
      return launch(k_tgrad<decltype(NF)::value, decltype(CB)::value>, nb, a.m.T, lds, s, a, cap, max_ent);
    });
  });
}
