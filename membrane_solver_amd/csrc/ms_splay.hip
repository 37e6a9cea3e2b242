// tilt_splay_twist_in on the device (modules/energy/tilt_splay_twist_in.py:113-252, ambient_v1 transport, native
// divergence): the split form of the tilt-gradient energy of the inner leaflet.  Per facet (rows i0 i1 i2, positions
// v_k, tilts t_k):
//   n = (v1 - v0) x (v2 - v0), n2 = n.n, denom = max(n2, 1e-20), e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0,
//   g_k = (n x e_k) / denom (geometry/triangle_ops.py:75-95), area = 0.5 sqrt(max(n2, 0)), n_hat = n / |n| (|n| > 1e-20, else 0),
//   div = t0.g0 + t1.g1 + t2.g2, curl_n = (g0 x t0 + g1 x t1 + g2 x t2) . n_hat,
//   E = 0.5 sum_f area (k_splay div^2 + k_twist curl_n^2),
//   dE/dt_k += area k_splay div g_k + area k_twist curl_n (n_hat x g_k).
// No shape gradient (the reference leaves grad_arr alone), no facet mask: a facet of area exactly 0 has n = 0, so
// g_k = 0 and area = 0, and every term of it is an exact zero.
//
// Part of the ms_kernels.hip translation unit (included there, inside namespace ms): the tile helpers (tile_ctx,
// csr_issue / csr_commit, lds_v3, xcd_tile, V3, the DPP reductions, axpy1) are that file's.
//
//   k_splay<MODE>: one workgroup per tile, k_tsmooth's data flow.  MODE 0 energy only (no staging block, no CSR);
//                  MODE 1 + the tilt gradient ADDED into tilt_grad, gathered through the tile's CSR in ascending facet
//                  order: one order in both modes of ms_set_deterministic, no atomics.
//
// The energy partial of a tile goes to the tile's cell of `slot` (MS_S_ETS_IN: MS_NSCAL has no room for a slot of the
// module's own): cell_mode 1 adds it behind the pass that defined the cell (k_tsmooth, the fused energy pass), 2 defines
// the cell, 0 leaves it alone.  Every workgroup parks its sum in wg_sums[tile] with a plain store;
// ms_get_tilt_splay_twist_energy adds them on the host in index order when somebody asks (no arrival counter).
// LDS: px[3][cap] | tl[3][cap] | stg[9][T] (MODE 1; red aliases it) or red[16] (MODE 0) | vent (u16, MODE 1)

template <int MODE>
__device__ __forceinline__ void splay_body(const SplayArgs& a, int cap, int max_ent, double* lds, int block_id) {
  const int T = a.m.T;
  double* px = lds;
  double* tl = px + 3 * cap;
  double* stg = tl + 3 * cap;
  double* red = stg;
  uint16_t* vent = reinterpret_cast<uint16_t*>(stg + 9 * T);

  const TileCtx t = tile_ctx(a.m, a.tile0 + xcd_tile(block_id, a.tile1 - a.tile0));
  const int tid = threadIdx.x;
  const bool have_d = a.d != nullptr;
  int cur = 0, end = 0;
  {
    const bool own = tid < t.n_owned;
    CsrStage cs;
    if (MODE != 0) csr_issue(cs, a.m, t, T, tid);
    struct Row {
      double x0, x1, x2, t0, t1, t2;
    };
    auto load_row = [&](int v) {
      Row r;
      const size_t g = 3 * (size_t)v;
      r.x0 = a.x[g];
      r.x1 = a.x[g + 1];
      r.x2 = a.x[g + 2];
      if (have_d) {
        const double d0 = a.d[g], d1 = a.d[g + 1], d2 = a.d[g + 2];
        if (!(a.m.vflags[v] & VF_FIXED)) {
          r.x0 = axpy1(r.x0, a.alpha, d0);
          r.x1 = axpy1(r.x1, a.alpha, d1);
          r.x2 = axpy1(r.x2, a.alpha, d2);
        }
      }
      r.t0 = a.tilts[g];
      r.t1 = a.tilts[g + 1];
      r.t2 = a.tilts[g + 2];
      return r;
    };
    auto put_row = [&](const Row& r, int sl) {
      px[sl] = r.x0;
      px[cap + sl] = r.x1;
      px[2 * cap + sl] = r.x2;
      tl[sl] = r.t0;
      tl[cap + sl] = r.t1;
      tl[2 * cap + sl] = r.t2;
    };
    const bool has_h = tid < t.nh;
    int hv = 0;
    if (has_h) hv = a.m.halo_ids[t.h0 + tid];
    Row ro{}, rh{};
    if (own) ro = load_row(t.v_lo + tid);
    if (has_h) rh = load_row(hv);
    if (own) put_row(ro, tid);
    if (has_h) put_row(rh, t.n_owned + tid);
    for (int h = tid + T; h < t.nh; h += T) put_row(load_row(a.m.halo_ids[t.h0 + h]), t.n_owned + h);
    if (MODE != 0) {
      csr_commit(cs, a.m, t, T, tid, vent);
      if (own) {
        cur = cs.vo0;
        end = cs.vo1;
      }
    }
  }
  __syncthreads();

  double e_st = 0.0;
  double ax = 0, ay = 0, az = 0;
  for (int c0f = t.f0; c0f < t.f1; c0f += T) {
    const int p = c0f + tid;
    if (p < t.f1) {
      const TileFacet tf = a.m.tile_facets[p];
      const V3 v0 = lds_v3(px, cap, tf.l0), v1 = lds_v3(px, cap, tf.l1), v2 = lds_v3(px, cap, tf.l2);
      const V3 e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0;
      const V3 n = cross(e2, -e1);  // (v1 - v0) x (v2 - v0)
      const double n2 = dot(n, n);
      const double inv_den = 1.0 / (n2 < 1.0e-20 ? 1.0e-20 : n2);
      const double nn = sqrt(n2);
      const double area = 0.5 * nn;
      const V3 nh = nn > 1.0e-20 ? (1.0 / nn) * n : mk(0, 0, 0);
      const V3 g0 = inv_den * cross(n, e0), g1 = inv_den * cross(n, e1), g2 = inv_den * cross(n, e2);
      const V3 t0 = lds_v3(tl, cap, tf.l0), t1 = lds_v3(tl, cap, tf.l1), t2 = lds_v3(tl, cap, tf.l2);
      const double div = (dot(t0, g0) + dot(t1, g1)) + dot(t2, g2);
      const V3 curl = (cross(g0, t0) + cross(g1, t1)) + cross(g2, t2);
      const double curl_n = dot(curl, nh);
      if (tf.flags & TF_OWNER) e_st += 0.5 * (area * (a.k_splay * (div * div) + a.k_twist * (curl_n * curl_n)));
      if (MODE == 1) {
        const double cd = area * a.k_splay * div, cc = area * a.k_twist * curl_n;
        const V3 d0 = cd * g0 + cc * cross(nh, g0);
        const V3 d1 = cd * g1 + cc * cross(nh, g1);
        const V3 d2 = cd * g2 + cc * cross(nh, g2);
        double* s = stg + tid;
        s[0 * T] = d0.x; s[1 * T] = d0.y; s[2 * T] = d0.z;
        s[3 * T] = d1.x; s[4 * T] = d1.y; s[5 * T] = d1.z;
        s[6 * T] = d2.x; s[7 * T] = d2.y; s[8 * T] = d2.z;
      }
    }
    if (MODE != 0) {
      __syncthreads();
      const int lo = c0f - t.f0, hi = min(c0f + T, t.f1) - t.f0;
      while (cur < end) {
        const int ent = vent[cur];
        const int fl = ent >> 2;
        if (fl >= hi) break;
        const int k = ent & 3;
        const double* s = stg + (fl - lo);
        ax += s[(3 * k) * T];
        ay += s[(3 * k + 1) * T];
        az += s[(3 * k + 2) * T];
        ++cur;
      }
      __syncthreads();
    }
  }
  if (MODE == 1 && tid < t.n_owned) {
    const size_t o = 3 * (size_t)(t.v_lo + tid);
    a.tilt_grad[o] += ax;
    a.tilt_grad[o + 1] += ay;
    a.tilt_grad[o + 2] += az;
  }
  const double e_tile = block_reduce(e_st, 0, red);  // (its first barrier is behind the last read of the staging block)
  if (tid == 0) {
    // (no other workgroup of this launch touches the cell)
    double* cell = a.partials + (size_t)a.slot * a.m.n_tiles + t.tile;
    if (a.cell_mode == 2) *cell = e_tile;
    else if (a.cell_mode == 1) *cell = *cell + e_tile;
    a.wg_sums[t.tile - a.tile0] = e_tile;
  }
}

template <int MODE>
__global__ __launch_bounds__(512) void k_splay(SplayArgs a, int cap, int max_ent) {
  extern __shared__ double lds[];
  splay_body<MODE>(a, cap, max_ent, lds, (int)blockIdx.x);
}

size_t splay_lds_bytes(int T, int cap, int max_ent, int mode) {
  if (mode == 0) return (6 * (size_t)cap + 16) * sizeof(double);
  return (6 * (size_t)cap + 9 * (size_t)T) * sizeof(double) + 2 * ((size_t)((max_ent + 3) & ~3)) + 64;
}

// (neither kernel is recorded by the one-tile interpreter: the host flushes it first, splay_pass)
hipError_t launch_splay(const SplayArgs& a, int mode, int cap, int max_ent, hipStream_t s) {
  const int nb = a.tile1 - a.tile0;
  if (nb <= 0) return hipSuccess;
  const size_t lds = splay_lds_bytes(a.m.T, cap, max_ent, mode);
  if (mode == 0) return launch(k_splay<0>, nb, a.m.T, lds, s, a, cap, max_ent);
  return launch(k_splay<1>, nb, a.m.T, lds, s, a, cap, max_ent);
}
