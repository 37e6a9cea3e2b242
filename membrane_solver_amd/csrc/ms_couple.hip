// tilt_coupling on the device (modules/energy/tilt_coupling.py:114-262): E = 1/2 k_c int |t_out + s t_in|^2 dA with
// s = -1 ("difference") or +1 ("sum").  Per vertex d_v = t_out,v + s t_in,v and q_v = |d_v|^2; per facet with
// |n| >= 1e-12, coeff_f = 0.5 k_c ((q_0 + q_1 + q_2) / 3) and E = sum coeff_f A_f; shape gradient coeff_f dA_f/dv_k;
// tilt gradients k_c d_v A_v into tilt_out and k_c s d_v A_v into tilt_in, A_v = sum A_f / 3 over the same facets.
// This is k_tilt's lumped MODE 0 / 1 arithmetic applied to the field d, operation for operation (sq, coeff, hs, G_k,
// a3), so the two modules round alike.  d itself never reaches global memory.
//
// Part of the ms_kernels.hip translation unit (included there, inside namespace ms): the tile helpers (tile_ctx,
// facet_load / facet_unpack, lds_v3, xcd_tile, V3, the DPP reductions, axpy1) are that file's.
//
//   k_couple<MODE>: one workgroup per tile.  MODE 0 energy only (no staging block, no CSR); MODE 1 + the shape gradient
//                   ADDED into g, + both tilt gradients ADDED into tg_out / tg_in (each of the three optional).
//   k_couple_vec  : positions frozen (a relaxation in progress), barycentric vertex areas `va` at hand:
//                   E = 1/2 k_c sum_v q_v A_v and the same two tilt gradients, one streaming pass (k_tvec mode 4's shape).
//
// The energy partial of a tile goes to the tile's cell of `slot` (MS_S_ETILT_OUT: MS_NSCAL has no room for a slot of the
// module's own): cell_mode 1 adds it behind the pass that defined the cell, 2 defines the cell, 0 leaves it alone.
// The module's own energy: every workgroup parks its sum in wg_sums[tile]; ms_get_tilt_coupling_energy adds them up on
// the host in index order when somebody asks (a counter every workgroup of a 4 000-tile launch increments costs more
// than the kernel: measured).  No atomics anywhere: every sum has a fixed order in both modes of
// ms_set_deterministic.
// LDS of k_couple: px[3][cap] | q[cap] | stg[10][T] (MODE 1) | red[16] | voff, vent (u16, MODE 1) -- k_tilt's budget.

// s: the tile's sum, valid in thread 0
__device__ __forceinline__ void couple_finish(const CoupleArgs& a, int tile, double s) {
  if (threadIdx.x == 0) {
    // (no other workgroup of this launch touches the cell)
    double* cell = a.partials + (size_t)a.slot * a.m.n_tiles + tile;
    if (a.cell_mode == 2) *cell = s;
    else if (a.cell_mode == 1) *cell = *cell + s;
    a.wg_sums[tile - a.tile0] = s;
  }
}

template <int MODE>
__device__ __forceinline__ void couple_body(const CoupleArgs& a, int cap, int max_ent, double* lds, int block_id) {
  const int T = a.m.T;
  double* px = lds;
  double* tq = px + 3 * cap;
  double* stg = tq + cap;
  double* red = stg + (MODE == 0 ? 0 : 10 * T);
  uint16_t* voff = reinterpret_cast<uint16_t*>(red + 16);
  uint16_t* vent = voff + (T + 2);

  const TileCtx t = tile_ctx(a.m, a.tile0 + xcd_tile(block_id, a.tile1 - a.tile0));
  const int tid = threadIdx.x;
  const bool have_d = a.d != nullptr;
  const double sgn = a.sign;

  V3 dv = mk(0, 0, 0);  // this thread's owned d_v
  FacetRec<false> tf_nx = facet_null<false>();
  if (t.f0 + tid < t.f1) tf_nx = facet_load<false>(a.m, (size_t)(t.f0 + tid));
  {
    struct Row {
      double x0, x1, x2, d0, d1, d2;
    };
    auto load_row = [&](int v) {
      Row r;
      const size_t g = 3 * (size_t)v;
      const uint8_t fl = a.m.vflags[v];
      r.x0 = a.x[g];
      r.x1 = a.x[g + 1];
      r.x2 = a.x[g + 2];
      if (have_d) {
        const double d0 = a.d[g], d1 = a.d[g + 1], d2 = a.d[g + 2];
        if (!(fl & VF_FIXED)) {
          r.x0 = axpy1(r.x0, a.alpha, d0);
          r.x1 = axpy1(r.x1, a.alpha, d1);
          r.x2 = axpy1(r.x2, a.alpha, d2);
        }
      }
      // d = t_out + s t_in (tilt_coupling.py:153; s t_in is exact)
      r.d0 = a.t_out[g] + sgn * a.t_in[g];
      r.d1 = a.t_out[g + 1] + sgn * a.t_in[g + 1];
      r.d2 = a.t_out[g + 2] + sgn * a.t_in[g + 2];
      return r;
    };
    auto put_row = [&](const Row& r, int sl) {
      px[sl] = r.x0;
      px[cap + sl] = r.x1;
      px[2 * cap + sl] = r.x2;
      const V3 th = mk(r.d0, r.d1, r.d2);
      tq[sl] = dot(th, th);
    };
    const bool own = tid < t.n_owned, has_h = tid < t.nh;
    int hv = 0;
    if (has_h) hv = a.m.halo_ids[t.h0 + tid];
    Row ro{}, rh{};
    if (own) ro = load_row(t.v_lo + tid);
    if (has_h) rh = load_row(hv);
    if (own) {
      put_row(ro, tid);
      dv = mk(ro.d0, ro.d1, ro.d2);
    }
    if (has_h) put_row(rh, t.n_owned + tid);
    for (int h = tid + T; h < t.nh; h += T) put_row(load_row(a.m.halo_ids[t.h0 + h]), t.n_owned + h);
  }
  if (MODE != 0) {
    const uint16_t* gv = a.m.tile_voff + (size_t)t.tile * (T + 1);
    voff[tid] = gv[tid];
    if (tid == 0) voff[T] = gv[T];
    const uint16_t* ge = a.m.vent + t.e0;
    for (int j = tid; j < t.n_ent; j += T) vent[j] = ge[j];
  }
  __syncthreads();

  double e_c = 0.0;
  double ax = 0, ay = 0, az = 0, aw = 0;  // vertex accumulators: shape gradient (xyz), area (w)
  int cur = 0, end = 0;
  if (MODE != 0 && tid < t.n_owned) {
    cur = voff[tid];
    end = voff[tid + 1];
  }
  for (int c0 = t.f0; c0 < t.f1; c0 += T) {
    const int p = c0 + tid;
    const TileFacet tf = facet_unpack<false>(tf_nx);
    if (p + T < t.f1) tf_nx = facet_load<false>(a.m, (size_t)(p + T));
    if (p < t.f1) {
      const V3 v0 = lds_v3(px, cap, tf.l0), v1 = lds_v3(px, cap, tf.l1), v2 = lds_v3(px, cap, tf.l2);
      const V3 e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0;
      const V3 n = cross(e2, -e1);
      const double A2 = norm(n);
      V3 G0 = mk(0, 0, 0), G1 = mk(0, 0, 0), G2 = mk(0, 0, 0);
      double a3 = 0.0;
      if (A2 >= 1.0e-12) {
        const double area = 0.5 * A2;
        const double sq = (tq[tf.l0] + tq[tf.l1]) + tq[tf.l2];
        const double coeff = 0.5 * a.k_c * (sq / 3.0);
        if (tf.flags & TF_OWNER) e_c += coeff * area;
        if (MODE == 1) {
          const double hs = 0.5 * coeff / A2;
          G0 = hs * cross(n, e0);
          G1 = hs * cross(n, e1);
          G2 = hs * cross(n, e2);
          a3 = area / 3.0;
        }
      }
      if (MODE == 1) {
        double* s = stg + tid;
        s[0 * T] = G0.x; s[1 * T] = G0.y; s[2 * T] = G0.z;
        s[3 * T] = G1.x; s[4 * T] = G1.y; s[5 * T] = G1.z;
        s[6 * T] = G2.x; s[7 * T] = G2.y; s[8 * T] = G2.z;
        s[9 * T] = a3;
      }
    }
    if (MODE != 0) {
      __syncthreads();
      const int lo = c0 - t.f0, hi = min(c0 + T, t.f1) - t.f0;
      while (cur < end) {
        const int ent = vent[cur];
        const int fl = ent >> 2;
        if (fl >= hi) break;
        const double* s = stg + (fl - lo);
        const int k = ent & 3;
        ax += s[(3 * k) * T];
        ay += s[(3 * k + 1) * T];
        az += s[(3 * k + 2) * T];
        aw += s[9 * T];
        ++cur;
      }
      __syncthreads();
    }
  }
  if (MODE == 1 && tid < t.n_owned) {
    const size_t o = 3 * (size_t)(t.v_lo + tid);
    if (a.g) {
      a.g[o] += ax;
      a.g[o + 1] += ay;
      a.g[o + 2] += az;
    }
    if (a.tg_out) {  // k_c d_v A_v (:197)
      a.tg_out[o] += a.k_c * dv.x * aw;
      a.tg_out[o + 1] += a.k_c * dv.y * aw;
      a.tg_out[o + 2] += a.k_c * dv.z * aw;
    }
    if (a.tg_in) {  // k_c s d_v A_v (:203; k_c s is exact)
      const double ks = a.k_c * sgn;
      a.tg_in[o] += ks * dv.x * aw;
      a.tg_in[o + 1] += ks * dv.y * aw;
      a.tg_in[o + 2] += ks * dv.z * aw;
    }
  }
  const double e_tile = block_reduce(e_c, 0, red);
  couple_finish(a, t.tile, e_tile);
}

template <int MODE>
__global__ __launch_bounds__(512) void k_couple(CoupleArgs a, int cap, int max_ent) {
  extern __shared__ double lds[];
  couple_body<MODE>(a, cap, max_ent, lds, (int)blockIdx.x);
}

__global__ __launch_bounds__(BLOCK) void k_couple_vec(CoupleArgs a, int with_grad) {
  __shared__ double red[16];
  const int tile = a.tile0 + (int)blockIdx.x;
  const int T = a.m.own, nv = a.m.nv;
  const double sgn = a.sign, ks = a.k_c * sgn;
  double s0 = 0.0;
  for (int i = threadIdx.x; i < T; i += BLOCK) {
    const int v = tile * T + i;
    if (v >= nv) break;
    const size_t o = 3 * (size_t)v;
    const V3 dv = mk(a.t_out[o] + sgn * a.t_in[o], a.t_out[o + 1] + sgn * a.t_in[o + 1], a.t_out[o + 2] + sgn * a.t_in[o + 2]);
    const double av = a.va[v];
    s0 += (dot(dv, dv)) * av;
    if (with_grad) {
      if (a.tg_out) {
        a.tg_out[o] += a.k_c * dv.x * av;
        a.tg_out[o + 1] += a.k_c * dv.y * av;
        a.tg_out[o + 2] += a.k_c * dv.z * av;
      }
      if (a.tg_in) {
        a.tg_in[o] += ks * dv.x * av;
        a.tg_in[o + 1] += ks * dv.y * av;
        a.tg_in[o + 2] += ks * dv.z * av;
      }
    }
  }
  const double r = block_reduce(s0, 0, red);
  couple_finish(a, tile, (0.5 * a.k_c) * r);
}

size_t couple_lds_bytes(int T, int cap, int max_ent, int mode) {
  if (mode == 0) return (4 * (size_t)cap + 16) * sizeof(double);
  return (4 * (size_t)cap + 10 * (size_t)T + 16) * sizeof(double) + 2 * ((size_t)T + 2 + max_ent + 8);
}

// (neither kernel is recorded by the one-tile interpreter: the host flushes it first, couple_pass)
hipError_t launch_couple(const CoupleArgs& a, int mode, int cap, int max_ent, hipStream_t s) {
  const int nb = a.tile1 - a.tile0;
  if (nb <= 0) return hipSuccess;
  const size_t lds = couple_lds_bytes(a.m.T, cap, max_ent, mode);
  if (mode == 0) return launch(k_couple<0>, nb, a.m.T, lds, s, a, cap, max_ent);
  return launch(k_couple<1>, nb, a.m.T, lds, s, a, cap, max_ent);
}

hipError_t launch_couple_vec(const CoupleArgs& a, int with_grad, hipStream_t s) {
  const int nb = a.tile1 - a.tile0;
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_couple_vec, dim3(nb), dim3(BLOCK), 0, s, a, with_grad);
  return hipGetLastError();
}
