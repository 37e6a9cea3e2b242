// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): phase API, boundary exchange, the sharded drivers (RCCL, peer-to-peer), ms_shard_step.
// ---- phase-level API -------------------------------------------------------
int ms_phase_energy(ms_ctx* c, int use_direction, double alpha, int write_trial, int guard,
                    int write_bending_factors) {
  if (!c) return MS_ERR_INVALID;
  if ((c->params.modules & MS_ANY_TILT_MODS) && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "the tilt module is not sharded yet (single GPU only)");
  if (use_direction)  // (an ms_step before this call may have left D to be written on demand)
    if (int rc = materialize_direction(c)) return rc;
  return phase_energy(c, c->params.modules, use_direction != 0, alpha, write_trial != 0, guard != 0,
                      write_bending_factors != 0);
}

int ms_phase_gradient(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  c->carry.grad_valid = false;  // G receives the raw (unfinalized) gradient
  return phase_gradient(c, c->params.modules, c->buf[MS_BUF_G], false);
}

int ms_phase_direction(ms_ctx* c, int stepper, int use_history) {
  if (!c) return MS_ERR_INVALID;
  c->precond = false;  // (the phase API has no preconditioned lane: never inherit one from an earlier ms_step)
  if (area_row_active(c))  // (its projection sits between the gradient pass and the direction kernel of ms_step)
    return fail(c, MS_ERR_STATE, "the phase API has no area constraint row (ms_step / ms_energy_and_gradient project it)");
  return phase_direction(c, stepper, use_history != 0);
}

int ms_phase_accept(ms_ctx* c, int keep_history) {
  if (!c) return MS_ERR_INVALID;
  if (int rc = materialize_direction(c)) return rc;  // (D becomes PD below: never unwritten)
  std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  c->sh_maxg2_valid = false;
  if (keep_history) {
    std::swap(c->buf[MS_BUF_G], c->buf[MS_BUF_PG]);
    std::swap(c->buf[MS_BUF_D], c->buf[MS_BUF_PD]);
    c->carry.pd_neg_pg = c->carry.dir_implicit;  // the accepted direction was -G = -PG from now on
    c->carry.last_g = c->buf[MS_BUF_PG];
    c->carry.cg_have_history = true;
    ++c->carry.cg_iter_count;
  }
  c->carry.dir_implicit = false;
  return MS_OK;
}

int ms_phase_commit_trial(ms_ctx* c, double alpha, int keep_history) {
  if (!c) return MS_ERR_INVALID;
  if (int rc = materialize_direction(c)) return rc;
  if (c->shard_count > 1) {
    // x <- x + alpha d in place on the rows this rank reads: its own rows and the halo rows
    // of its tiles (d is valid there after the boundary exchange); same expression as the
    // trial pass, so the committed doubles are the evaluated ones
    const Tiling& t = c->til;
    const int64_t rows_per = (int64_t)t.tiles_per_shard * t.own;
    HIPCHK(c, launch_axpy_rows(c->shard_rank * rows_per, (c->shard_rank + 1) * rows_per, c->d_halo_rows,
                               c->n_halo_rows, c->d_vflags, c->buf[MS_BUF_X], trial_dir(c), trial_alpha(c, alpha),
                               c->stream));
    std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);  // undone by ms_phase_accept's swap
    return ms_phase_accept(c, keep_history);
  }
  const size_t n3 = 3 * (size_t)c->til.nvp;
  HIPCHK(c, hipMemcpyAsync(c->buf[MS_BUF_XT], c->buf[MS_BUF_X], n3 * sizeof(double),
                           hipMemcpyDeviceToDevice, S(c)));
  HIPCHK(c, launch_axpy_masked(c->til.nvp, c->d_vflags, c->buf[MS_BUF_XT], trial_dir(c), trial_alpha(c, alpha),
                               c->stream));
  return ms_phase_accept(c, keep_history);
}

int ms_phase_gradient_direction(ms_ctx* c, int stepper, int use_history) {
  if (!c) return MS_ERR_INVALID;
  if ((c->params.modules & (MS_CON_VOLUME | MS_TILT_SHAPE_MODS)) || area_row_active(c))
    return fail(c, MS_ERR_STATE, "fused gradient+direction needs no constraint row and no tilt module");
  c->carry.grad_valid = false;
  const int dir_mode = (stepper == MS_STEPPER_CG && use_history) ? 2 : 1;
  return phase_gradient(c, c->params.modules, c->buf[MS_BUF_G], false, dir_mode);
}

int ms_phase_set_factors_valid(ms_ctx* c, int valid) {
  if (!c) return MS_ERR_INVALID;
  c->carry.factors_valid = valid != 0;
  return MS_OK;
}

namespace {
constexpr int SH_BUF_FK2 = -1, SH_BUF_FA2 = -2;
// slabs (and flag rows) of the peer exchange, used in turn: three, because an exchange queued behind a device-side decision
// may stay out on every rank -- with two, the exchange after a skipped one would write the slab the one before it is
// still being read from on a slower peer; with three, two exchanges that share a slab always have one that RAN between
// them (a skippable exchange directly follows a trial's exchange, which always runs)
constexpr int PEER_SLABS = 3;
constexpr int SH_ALT = 16;  // header slots SH_ALT + s carry slot s of a pair launch's other trial (tilt slots: the
                            // tilt modules are not sharded)
int row_buffers(ms_ctx* c, int n, const int* ids, double* p[4], int ncomp[4], int* comps) {
  if (n < 0 || n > 4 || (n > 0 && !ids)) return fail(c, MS_ERR_INVALID, "boundary exchange: 0..4 buffers");
  *comps = 0;
  for (int k = 0; k < n; ++k) {
    if (ids[k] == SH_BUF_FK2 || ids[k] == SH_BUF_FA2) {  // (internal) a pair launch's second factor set
      if (!c->fK2) return fail(c, MS_ERR_STATE, "boundary exchange: pair buffers not allocated");
      p[k] = ids[k] == SH_BUF_FK2 ? c->fK2 : c->fA2;
      ncomp[k] = ids[k] == SH_BUF_FA2 ? 2 : 3;
      *comps += ncomp[k];
      continue;
    }
    if (ids[k] < 0 || ids[k] > MS_BUF_FA) return fail(c, MS_ERR_INVALID, "boundary exchange: bad buffer id");
    p[k] = c->buf[ids[k]];
    ncomp[k] = ids[k] == MS_BUF_FA ? 2 : 3;
    *comps += ncomp[k];
  }
  return MS_OK;
}
}  // namespace

int ms_boundary_info(ms_ctx* c, int64_t info[4]) {
  if (!c || !info) return MS_ERR_INVALID;
  info[0] = c->bnd_max;
  info[1] = c->bnd_off[(size_t)c->shard_rank + 1] - c->bnd_off[(size_t)c->shard_rank];
  info[2] = c->n_halo_rows;
  info[3] = c->shard_count;
  return MS_OK;
}

size_t ms_exchange_bytes(ms_ctx* c, int n_buffers, const int* buffer_ids) {
  double* p[4];
  int nc[4], comps = 0;
  if (!c || row_buffers(c, n_buffers, buffer_ids, p, nc, &comps)) return 0;
  return sizeof(double) * ((size_t)MS_NSCAL + (size_t)c->bnd_max * comps);
}

int ms_pack_boundary(ms_ctx* c, int n_buffers, const int* buffer_ids, void* send_dev, size_t send_bytes) {
  if (!c || !send_dev) return MS_ERR_INVALID;
  double* p[4];
  int nc[4], comps = 0;
  int rc = row_buffers(c, n_buffers, buffer_ids, p, nc, &comps);
  if (rc) return rc;
  if (send_bytes < ms_exchange_bytes(c, n_buffers, buffer_ids))
    return fail(c, MS_ERR_INVALID, "ms_pack_boundary: send buffer smaller than ms_exchange_bytes");
  const int me = c->shard_rank;
  HIPCHK(c, launch_pack_boundary(c->d_bnd_rows + c->bnd_off[(size_t)me],
                                 c->bnd_off[(size_t)me + 1] - c->bnd_off[(size_t)me], p, nc, n_buffers,
                                 c->d_scal, static_cast<double*>(send_dev), c->stream));
  return MS_OK;
}

int ms_unpack_boundary(ms_ctx* c, int n_buffers, const int* buffer_ids, const void* recv_dev,
                       size_t stride_bytes, double* scal_all_host) {
  if (!c || !recv_dev || !scal_all_host) return MS_ERR_INVALID;
  double* p[4];
  int nc[4], comps = 0;
  int rc = row_buffers(c, n_buffers, buffer_ids, p, nc, &comps);
  if (rc) return rc;
  if (stride_bytes < ms_exchange_bytes(c, n_buffers, buffer_ids) || stride_bytes % sizeof(double))
    return fail(c, MS_ERR_INVALID, "ms_unpack_boundary: bad stride");
  HIPCHK(c, launch_unpack_boundary(c->d_bnd_rows, c->d_bnd_off, c->shard_rank, c->shard_count, c->bnd_max,
                                   p, nc, n_buffers, static_cast<const double*>(recv_dev),
                                   stride_bytes / sizeof(double), c->d_scal_all, c->stream));
  HIPCHK(c, hipMemcpyAsync(scal_all_host, c->d_scal_all, sizeof(double) * MS_NSCAL * (size_t)c->shard_count,
                           hipMemcpyDeviceToHost, S(c)));
  HIPCHK(c, hipStreamSynchronize(S(c)));
  return MS_OK;
}

// ---- library-side sharded driver ------------------------------------------------
namespace {
struct NcclUniqueId {
  char internal[128];
};
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(NcclUniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, NcclUniqueId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
};
Rccl g_rccl;

int rccl_bind() {
  if (g_rccl.lib) return MS_OK;
  // the copy the process already uses (torch.distributed's) first, then the ROCm one
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  void* lib = nullptr;
  for (const char* n : names) {
    lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (lib) break;
  }
  for (size_t i = 0; !lib && i < sizeof(names) / sizeof(names[0]); ++i) lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return fail(nullptr, MS_ERR_STATE, std::string("librccl not found: ") + dlerror());
  g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  g_rccl.AllGather = reinterpret_cast<decltype(g_rccl.AllGather)>(dlsym(lib, "ncclAllGather"));
  g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  g_rccl.CommCount = reinterpret_cast<decltype(g_rccl.CommCount)>(dlsym(lib, "ncclCommCount"));
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather)
    return fail(nullptr, MS_ERR_STATE, "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather");
  g_rccl.lib = lib;
  return MS_OK;
}

int shard_buffers(ms_ctx* c) {
  if (c->d_xsend) return MS_OK;
  const size_t n_max = (size_t)MS_NSCAL + 10 * (size_t)c->bnd_max;  // at most 2 x (fK 3 + fA 2) per boundary row
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_xsend), sizeof(double) * n_max));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_xrecv), sizeof(double) * n_max * (size_t)c->shard_count));
  HIPCHK(c, hipMemset(c->d_xsend, 0, sizeof(double) * n_max));
  HIPCHK(c, hipMemset(c->d_xrecv, 0, sizeof(double) * n_max * (size_t)c->shard_count));
  // two sets of header mailboxes, by exchange parity: an exchange may be queued behind one whose headers the host
  // has not read yet (the chained gradient + direction pass of an accepted trial)
  const size_t sb = sizeof(double) * MS_NSCAL * (size_t)c->shard_count;
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_scal_all), 2 * sb, hipHostMallocMapped));
  memset(c->h_scal_all, 0, 2 * sb);
  HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_h_scal_all), c->h_scal_all, 0));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_xseq), 2 * sizeof(unsigned long long) * (size_t)c->shard_count,
                          hipHostMallocMapped));
  for (int r = 0; r < 2 * c->shard_count; ++r) c->h_xseq[r] = 0;
  HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_h_xseq), c->h_xseq, 0));
  return MS_OK;
}

const int SH_SUM[] = {MS_S_ESURF, MS_S_VOL, MS_S_EBEND, MS_S_GGC, MS_S_GCGC, MS_S_GNORM2, MS_S_GDOTD, MS_S_ETILT};
constexpr uint32_t SH_ENERGY = (1u << MS_S_ESURF) | (1u << MS_S_VOL) | (1u << MS_S_EBEND) |
                               (1u << MS_S_MINEDGE2) | (1u << MS_S_GUARD);
constexpr uint32_t SH_GRAD = (1u << MS_S_GGC) | (1u << MS_S_GCGC);
constexpr uint32_t SH_DIR = (1u << MS_S_GNORM2) | (1u << MS_S_GDOTD) | (1u << MS_S_MAXD2) | (1u << MS_S_MAXG2);

// One exchange: boundary rows of `ids` + the MS_NSCAL scalars of every rank; `slots` of the
// rank-ordered fold go to c->sh_scal (push: also to the device scalars).
// queue half of an exchange: pack (+ flags), transport, unpack.  gate != nullptr (peer-to-peer transport with in-kernel
// flags only): the kernels run iff *gate == gate_want -- a word every rank derives from the same doubles
// (shard_decide), so the exchange is skipped by all ranks or by none.  decide != nullptr: the exchange's unpack kernel
// takes a trial's decision (never of a gated exchange).  *ticket_out = the exchange's ticket for shard_exchange_take.
int shard_exchange_queue(ms_ctx* c, int n, const int* ids, unsigned long long* ticket_out, const uint32_t* gate = nullptr,
                         uint32_t gate_want = 0, const ShardDecideArgs* decide = nullptr) {
  double* p[4];
  int nc[4], comps = 0;
  int rc = row_buffers(c, n, ids, p, nc, &comps);
  if (rc) return rc;
  rc = shard_buffers(c);
  if (rc) return rc;
  const size_t count = (size_t)MS_NSCAL + (size_t)c->bnd_max * comps;
  const int me = c->shard_rank, W = c->shard_count;
  ++c->xticket;
  *ticket_out = c->xticket;
  const size_t hx = (size_t)(c->xticket & 1);
  double* const d_heads = c->d_h_scal_all + hx * MS_NSCAL * (size_t)W;
  unsigned long long* const d_seq = c->d_h_xseq + hx * (size_t)W;
  if (c->peer_on) {
    // peer-to-peer: this rank's message goes straight into slot `me` of every peer's slab (slab = exchange parity),
    // then its flag word there is raised; the unpack kernel runs behind a bounded wait for every peer's word here
    ++c->peer_ticket;
    const int par = (int)(c->peer_ticket % PEER_SLABS);
    if (count > c->peer_stride) return fail(c, MS_ERR_STATE, "peer exchange: message longer than the slab slot");
    double* dst[16];
    unsigned long long* flg[16];
    for (int r = 0; r < W; ++r) {
      dst[r] = c->peer_slabs[(size_t)r] + ((size_t)par * W + (size_t)me) * c->peer_stride;
      flg[r] = c->peer_flags[(size_t)r] + (size_t)par * 16;
    }
    // (the pack kernel's last block per peer raises the flag word itself)
    const bool fused_flags = c->d_peer_flagtab != nullptr;
    if (gate != nullptr && (!fused_flags || c->peer_barrier))
      return fail(c, MS_ERR_STATE, "peer exchange: a gated exchange needs the in-kernel flag words");
    if (gate != nullptr && decide != nullptr)
      return fail(c, MS_ERR_STATE, "peer exchange: a gated exchange cannot carry a trial's decision");
    HIPCHK(c, launch_pack_peers(c->d_bnd_rows + c->bnd_off[(size_t)me],
                                c->bnd_off[(size_t)me + 1] - c->bnd_off[(size_t)me], p, nc, n, c->d_scal, dst, W,
                                c->stream, fused_flags ? c->d_peer_flagtab + par : nullptr, c->d_peer_arrived, me,
                                c->peer_ticket, gate, gate_want));
    if (!fused_flags) HIPCHK(c, launch_flag_peers(flg, me, W, c->peer_ticket, c->stream));
    const unsigned long long* wait_flags = c->d_peer_flag + (size_t)par * 16;
    if (c->peer_barrier) {  // (contexts of one process wait on the host: see ms_shard_peer_set_barrier)
      HIPCHK(c, hipStreamSynchronize(S(c)));
      if (c->peer_barrier(c->peer_barrier_user) != 0) return fail(c, MS_ERR_STATE, "peer exchange: the caller's barrier failed");
      wait_flags = nullptr;
    }
    // every block row of the unpack kernel waits (bounded) for the flag of the rank whose message it unpacks
    HIPCHK(c, launch_unpack_boundary(c->d_bnd_rows, c->d_bnd_off, me, W, c->bnd_max, p, nc, n,
                                     c->d_peer_slab + (size_t)par * W * c->peer_stride, c->peer_stride,
                                     d_heads, c->stream, d_seq, c->xticket, /*remote_written=*/true,
                                     wait_flags, c->peer_ticket, c->d_h_err + 1,  // (a word of its own: h_err[0] is the queue's)
                                     gate, gate_want, decide, decide ? c->d_peer_arrived + 16 : nullptr));
  } else {
    if (gate != nullptr || decide != nullptr) return fail(c, MS_ERR_STATE, "a gated exchange needs the peer-to-peer transport");
    HIPCHK(c, launch_pack_boundary(c->d_bnd_rows + c->bnd_off[(size_t)me],
                                   c->bnd_off[(size_t)me + 1] - c->bnd_off[(size_t)me], p, nc, n, c->d_scal,
                                   c->d_xsend, c->stream));
    if (c->allgather_cb) {
      HIPCHK(c, hipStreamSynchronize(S(c)));
      if (c->allgather_cb(c->allgather_user, c->d_xsend, c->d_xrecv, count * sizeof(double)) != 0)
        return fail(c, MS_ERR_STATE, "caller-supplied all-gather failed");
    } else if (c->comm) {
      const int r = g_rccl.AllGather(c->d_xsend, c->d_xrecv, count, /*ncclDouble*/ 8, c->comm, S(c));
      if (r != 0)
        return fail(c, MS_ERR_HIP, std::string("ncclAllGather: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"));
    } else if (W == 1) {
      HIPCHK(c, hipMemcpyAsync(c->d_xrecv, c->d_xsend, count * sizeof(double), hipMemcpyDeviceToDevice, S(c)));
    } else {
      return fail(c, MS_ERR_STATE, "ms_shard_step: no communicator (ms_shard_comm_init / ms_shard_set_allgather / ms_shard_peer_*)");
    }
    // the unpack kernel posts one sequence word per rank as soon as that rank's scalar header is in the mailbox
    HIPCHK(c, launch_unpack_boundary(c->d_bnd_rows, c->d_bnd_off, me, W, c->bnd_max, p, nc, n, c->d_xrecv, count,
                                     d_heads, c->stream, d_seq, c->xticket));
  }
  return MS_OK;
}

// take half: wait for every rank's header of exchange `ticket`, fold `slots` in rank order into c->sh_scal
int shard_exchange_take(ms_ctx* c, unsigned long long ticket, uint32_t slots, bool push, bool fold_alt = false) {
  const int W = c->shard_count;
  const size_t hx = (size_t)(ticket & 1);
  const double* const heads = c->h_scal_all + hx * MS_NSCAL * (size_t)W;
  const unsigned long long* const seq = c->h_xseq + hx * (size_t)W;
  bool seen = false;
  for (long spin = 0; spin < 20000000L; ++spin) {
    seen = true;
    for (int r = 0; r < W && seen; ++r) seen = __atomic_load_n(seq + r, __ATOMIC_ACQUIRE) >= ticket;
    if (seen) break;
    __builtin_ia32_pause();
  }
  if (!seen) HIPCHK(c, hipStreamSynchronize(S(c)));
  if (c->peer_on && c->h_err && (__atomic_load_n(c->h_err + 1, __ATOMIC_ACQUIRE) >> 62) == 1) {
    const unsigned long long e = __atomic_exchange_n(c->h_err + 1, 0ull, __ATOMIC_ACQ_REL);  // reported once
    return fail(c, MS_ERR_STATE, "peer exchange: a peer's flag did not arrive within the bounded wait (rank " +
                                     std::to_string((int)((e >> 32) & 0xff)) + ")");
  }
  if (!seen) {
    bool now = true;
    for (int r = 0; r < W && now; ++r) now = __atomic_load_n(seq + r, __ATOMIC_ACQUIRE) >= ticket;
    if (!now) return fail(c, MS_ERR_STATE, "boundary exchange: the headers of an exchange the host waited for never arrived (a gated exchange that stayed out?)");
  }
  // fold in rank order: every rank adds the same doubles in the same order
  for (int sl : SH_SUM)
    if (slots & (1u << sl)) {
      double acc = 0.0;
      for (int r = 0; r < W; ++r) acc += heads[(size_t)r * MS_NSCAL + sl];
      c->sh_scal[sl] = acc;
    }
  if (slots & (1u << MS_S_MINEDGE2)) {
    double m = heads[MS_S_MINEDGE2];
    for (int r = 1; r < W; ++r) m = std::min(m, heads[(size_t)r * MS_NSCAL + MS_S_MINEDGE2]);
    c->sh_scal[MS_S_MINEDGE2] = m;
  }
  for (int sl : {(int)MS_S_GUARD, (int)MS_S_MAXD2, (int)MS_S_MAXG2})
    if (slots & (1u << sl)) {
      double m = heads[sl];
      for (int r = 1; r < W; ++r) m = std::max(m, heads[(size_t)r * MS_NSCAL + sl]);
      c->sh_scal[sl] = m;
    }
  if (fold_alt) {  // the pair launch's other trial: same folds, same rank order, from the SH_ALT header slots
    for (int sl : {(int)MS_S_ESURF, (int)MS_S_VOL, (int)MS_S_EBEND}) {
      double acc = 0.0;
      for (int r = 0; r < W; ++r) acc += heads[(size_t)r * MS_NSCAL + SH_ALT + sl];
      c->sh_scal2[sl] = acc;
    }
    double m = heads[SH_ALT + MS_S_MINEDGE2];
    for (int r = 1; r < W; ++r) m = std::min(m, heads[(size_t)r * MS_NSCAL + SH_ALT + MS_S_MINEDGE2]);
    c->sh_scal2[MS_S_MINEDGE2] = m;
  }
  if (push)
    HIPCHK(c, hipMemcpyAsync(c->d_scal, c->sh_scal, sizeof(double) * MS_NSCAL, hipMemcpyHostToDevice, S(c)));
  ++c->sh_exchanges;
  return MS_OK;
}

int shard_exchange(ms_ctx* c, int n, const int* ids, uint32_t slots, bool push, bool fold_alt = false) {
  unsigned long long ticket = 0;
  int rc = shard_exchange_queue(c, n, ids, &ticket);
  if (rc) return rc;
  return shard_exchange_take(c, ticket, slots, push, fold_alt);
}

double shard_energy_of(const ms_ctx* c, const double* scal) {
  const uint32_t m = c->params.modules;
  double e = 0.0;
  if (m & MS_MOD_SURFACE) e += scal[MS_S_ESURF];
  if (m & MS_MOD_BENDING) e += scal[MS_S_EBEND];
  e += penalty_energy(c, scal[MS_S_VOL], 0.0);  // (no area penalty here: ms_shard_step refuses the module)
  return e;
}
double shard_energy(const ms_ctx* c) { return shard_energy_of(c, c->sh_scal); }
}  // namespace

static void shard_comm_destroy(void* comm) {
  if (comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm);
}

int ms_shard_unique_id(void* id128) {
  if (!id128) return MS_ERR_INVALID;
  int rc = rccl_bind();
  if (rc) return rc;
  NcclUniqueId id;
  const int r = g_rccl.GetUniqueId(&id);
  if (r != 0) return fail(nullptr, MS_ERR_HIP, "ncclGetUniqueId failed");
  memcpy(id128, id.internal, 128);
  return MS_OK;
}

int ms_shard_comm_init(ms_ctx* c, const void* id128) {
  if (!c || !id128) return fail(c, MS_ERR_INVALID, "ms_shard_comm_init: NULL argument");
  int rc = rccl_bind();
  if (rc) return fail(c, rc, g_last_error);
  (void)hipSetDevice(c->device);
  NcclUniqueId id;
  memcpy(id.internal, id128, 128);
  const int r = g_rccl.CommInitRank(&c->comm, c->shard_count, id, c->shard_rank);
  if (r != 0) {
    c->comm = nullptr;
    return fail(c, MS_ERR_HIP, std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"));
  }
  return shard_buffers(c);
}

int ms_shard_set_allgather(ms_ctx* c, ms_allgather_fn fn, void* user) {
  if (!c) return MS_ERR_INVALID;
  c->allgather_cb = fn;
  c->allgather_user = user;
  return shard_buffers(c);
}

namespace {
int peer_alloc(ms_ctx* c) {
  if (c->d_peer_slab) return MS_OK;
  if (c->shard_count > 16) return fail(c, MS_ERR_INVALID, "peer exchange: at most 16 ranks");
  int rc = shard_buffers(c);
  if (rc) return rc;
  c->peer_stride = (size_t)MS_NSCAL + 10 * (size_t)c->bnd_max;
  const size_t sb = sizeof(double) * PEER_SLABS * (size_t)c->shard_count * c->peer_stride;
  // The slabs and flag words are written by OTHER GPUs over xGMI while a kernel of this one is resident and polls them.
  // Ordinary hipMalloc memory is coarse-grained (cached read-write in this GPU's L2, coherent across agents only at
  // kernel boundaries): a resident wave could keep reading a stale flag or a boundary row of exchange k-2.  Uncached
  // (MTYPE_UC) device memory is what the collective library's own IPC signal buffers use; fine-grained is the second
  // choice; plain hipMalloc stays as the last resort (MS_PEER_MEM=uncached|finegrained|default forces one).
  const char* want = getenv("MS_PEER_MEM");
  const unsigned kinds[3] = {hipDeviceMallocUncached, hipDeviceMallocFinegrained, hipDeviceMallocDefault};
  const char* names[3] = {"uncached", "finegrained", "default"};
  c->peer_mem_kind = -1;
  for (int k = 0; k < 3 && c->peer_mem_kind < 0; ++k) {
    if (want && *want && strcmp(want, names[k]) != 0) continue;
    void *ps = nullptr, *pf = nullptr;
    hipError_t e1 = kinds[k] == hipDeviceMallocDefault ? hipMalloc(&ps, sb) : hipExtMallocWithFlags(&ps, sb, kinds[k]);
    hipError_t e2 = e1 != hipSuccess ? e1
                    : (kinds[k] == hipDeviceMallocDefault ? hipMalloc(&pf, sizeof(unsigned long long) * 16 * PEER_SLABS)
                                                          : hipExtMallocWithFlags(&pf, sizeof(unsigned long long) * 16 * PEER_SLABS, kinds[k]));
    hipIpcMemHandle_t probe;
    // (memory that cannot be exported is of no use here: ms_shard_peer_export would fail later)
    if (e1 == hipSuccess && e2 == hipSuccess && hipIpcGetMemHandle(&probe, ps) == hipSuccess &&
        hipIpcGetMemHandle(&probe, pf) == hipSuccess) {
      c->d_peer_slab = static_cast<double*>(ps);
      c->d_peer_flag = static_cast<unsigned long long*>(pf);
      c->peer_mem_kind = k;
    } else {
      (void)hipGetLastError();
      if (ps) (void)hipFree(ps);
      if (pf) (void)hipFree(pf);
    }
  }
  if (c->peer_mem_kind < 0) return fail(c, MS_ERR_HIP, "peer exchange: no exportable device memory for the slabs / flag words");
  HIPCHK(c, hipMemset(c->d_peer_slab, 0, sb));
  HIPCHK(c, hipMemset(c->d_peer_flag, 0, sizeof(unsigned long long) * 16 * PEER_SLABS));
  HIPCHK(c, hipDeviceSynchronize());
  return MS_OK;
}
}  // namespace

namespace {
// the peers' flag rows as the pack kernel reads them: one table per exchange parity
int peer_flag_table(ms_ctx* c) {
  const int W = c->shard_count;
  PeerFlags tab[PEER_SLABS];
  memset(tab, 0, sizeof(tab));
  for (int par = 0; par < PEER_SLABS; ++par)
    for (int r = 0; r < W; ++r) tab[par].p[r] = c->peer_flags[(size_t)r] + (size_t)par * 16;
  if (!c->d_peer_flagtab) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_peer_flagtab), sizeof(tab)));
  HIPCHK(c, hipMemcpy(c->d_peer_flagtab, tab, sizeof(tab), hipMemcpyHostToDevice));
  if (!c->d_peer_arrived) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_peer_arrived), sizeof(unsigned int) * 32));  // [16]: the unpack kernel's header blocks
    HIPCHK(c, hipMemset(c->d_peer_arrived, 0, sizeof(unsigned int) * 32));
  }
  return MS_OK;
}
}  // namespace

int ms_shard_peer_local(ms_ctx* c, void** recv_slab, void** flag_words) {
  if (!c || !recv_slab || !flag_words) return MS_ERR_INVALID;
  int rc = peer_alloc(c);
  if (rc) return rc;
  *recv_slab = c->d_peer_slab;
  *flag_words = c->d_peer_flag;
  return MS_OK;
}

int ms_shard_peer_export(ms_ctx* c, void* handles128) {
  if (!c || !handles128) return MS_ERR_INVALID;
  int rc = peer_alloc(c);
  if (rc) return rc;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  hipIpcMemHandle_t h[2];
  HIPCHK(c, hipIpcGetMemHandle(&h[0], c->d_peer_slab));
  HIPCHK(c, hipIpcGetMemHandle(&h[1], c->d_peer_flag));
  memcpy(handles128, h, 128);
  return MS_OK;
}

int ms_shard_peer_open(ms_ctx* c, const void* handles_all) {
  if (!c || !handles_all) return MS_ERR_INVALID;
  int rc = peer_alloc(c);
  if (rc) return rc;
  const int W = c->shard_count;
  c->peer_slabs.assign((size_t)W, nullptr);
  c->peer_flags.assign((size_t)W, nullptr);
  for (int r = 0; r < W; ++r) {
    if (r == c->shard_rank) {
      c->peer_slabs[(size_t)r] = c->d_peer_slab;
      c->peer_flags[(size_t)r] = c->d_peer_flag;
      continue;
    }
    hipIpcMemHandle_t h[2];
    memcpy(h, static_cast<const char*>(handles_all) + 128 * (size_t)r, 128);
    void *ps = nullptr, *pf = nullptr;
    HIPCHK(c, hipIpcOpenMemHandle(&ps, h[0], hipIpcMemLazyEnablePeerAccess));
    c->peer_opened.push_back(ps);
    HIPCHK(c, hipIpcOpenMemHandle(&pf, h[1], hipIpcMemLazyEnablePeerAccess));
    c->peer_opened.push_back(pf);
    c->peer_slabs[(size_t)r] = static_cast<double*>(ps);
    c->peer_flags[(size_t)r] = static_cast<unsigned long long*>(pf);
  }
  rc = peer_flag_table(c);
  if (rc) return rc;
  c->peer_on = true;
  return MS_OK;
}

int ms_shard_peer_set_pointers(ms_ctx* c, void* const* recv_slabs, void* const* flag_words) {
  if (!c || !recv_slabs || !flag_words) return MS_ERR_INVALID;
  int rc = peer_alloc(c);
  if (rc) return rc;
  const int W = c->shard_count;
  c->peer_slabs.assign((size_t)W, nullptr);
  c->peer_flags.assign((size_t)W, nullptr);
  for (int r = 0; r < W; ++r) {
    c->peer_slabs[(size_t)r] = static_cast<double*>(recv_slabs[r]);
    c->peer_flags[(size_t)r] = static_cast<unsigned long long*>(flag_words[r]);
  }
  if (c->peer_slabs[(size_t)c->shard_rank] != c->d_peer_slab)
    return fail(c, MS_ERR_INVALID, "ms_shard_peer_set_pointers: the own entry must be ms_shard_peer_local's");
  rc = peer_flag_table(c);
  if (rc) return rc;
  c->peer_on = true;
  return MS_OK;
}

int ms_shard_peer_set_barrier(ms_ctx* c, ms_barrier_fn fn, void* user) {
  if (!c) return MS_ERR_INVALID;
  c->peer_barrier = fn;
  c->peer_barrier_user = user;
  return MS_OK;
}

int64_t ms_shard_exchange_count(const ms_ctx* c) { return c ? (int64_t)c->sh_exchanges : 0; }
int ms_shard_chain_stats(const ms_ctx* c, int64_t stats[8]) {
  if (!c || !stats) return MS_ERR_INVALID;
  stats[0] = c->sh_chained;
  stats[1] = c->sh_chain_ran;
  stats[2] = c->sh_chain_adopted;
  stats[3] = c->sh_chain_dropped;
  stats[4] = stats[5] = stats[6] = stats[7] = 0;  // reserved
  return MS_OK;
}

int ms_shard_peer_memory_kind(const ms_ctx* c) { return (c && c->d_peer_slab) ? c->peer_mem_kind : -1; }

int ms_shard_comm_ranks(ms_ctx* c) {
  if (!c || !c->comm || !g_rccl.CommCount) return 0;
  int n = 0;
  return g_rccl.CommCount(c->comm, &n) == 0 ? n : 0;
}

// The control flow of parallel.ShardedStepper.step (itself a restatement of ms_step).
int ms_shard_step(ms_ctx* c, const ms_stepper_params* sp, double step_size, double tol, ms_step_result* out) {
  if (!c || !sp || !out) return fail(c, MS_ERR_INVALID, "ms_shard_step: NULL argument");
  const uint32_t mods = c->params.modules;
  if (mods & MS_ANY_TILT_MODS) return fail(c, MS_ERR_STATE, "the tilt modules are not sharded yet (single GPU only)");
  if (mods & MS_MOD_AREA_PENALTY) return fail(c, MS_ERR_STATE, "the body_area_penalty module is not sharded (single GPU only)");
  for (const EdgeTerm& t : kEdgeTerms)  // (MS_MOD_LINE_TENSION, MS_MOD_EDGE_LENGTH_PENALTY)
    if (mods & t.bit) return fail(c, MS_ERR_STATE, edge_not_sharded(t));
  if (sp->precondition) return fail(c, MS_ERR_STATE, "ConjugateGradient(precondition=True) is not sharded (single GPU only)");
  // (line_search.py:428-487: every trial projected onto the target volume -- the projection is not sharded; running the
  // plain lane instead would be a different trajectory, silently)
  if (sp->enforce_volume)
    return fail(c, MS_ERR_STATE, "volume_projection_during_minimization (the enforcer lane of the line search) is not sharded (single GPU only)");
  if (sp->enforce_pins || pins_set(c))
    return fail(c, MS_ERR_STATE, "pin_to_plane / pin_to_circle are not sharded (single GPU only)");
  if (sp->enforce_area || area_con_set(c) || c->area_row)
    return fail(c, MS_ERR_STATE, "the body_area / global_area constraints are not sharded (single GPU only)");
  if (sp->enforce_fixed_plane || sp->enforce_perimeter || fplane_set(c) || perimeter_set(c))
    return fail(c, MS_ERR_STATE, "the fixed_plane / perimeter constraints are not sharded (single GPU only)");
  c->precond = false;
  memset(out, 0, sizeof(*out));
  const bool cg = sp->stepper == MS_STEPPER_CG;
  const int restart = sp->restart_interval > 0 ? sp->restart_interval : 10;
  const bool use_history = cg && c->carry.cg_have_history && (c->carry.cg_iter_count % restart != 0);
  const bool bend = (mods & MS_MOD_BENDING) != 0;
  const bool constraint = (mods & MS_CON_VOLUME) != 0;
  const bool penalty = (mods & MS_MOD_VOLUME_PENALTY) != 0;
  const bool carry_mode = sp->reuse_energy0 >= 2;
  const int fbufs[2] = {MS_BUF_FK, MS_BUF_FA};
  const int n_fb = bend ? 2 : 0;
  const int dbuf[2] = {MS_BUF_D, MS_BUF_G};
  bool carried = carry_mode && c->sh_carry_valid;
  int rc;
  bool implicit_restart = false, fused = false;
  // the gradient + direction pass of this x and its exchange were queued behind the decision that accepted it
  bool adopt = false;
  if (c->sh_chain.valid) {
    c->sh_chain.valid = false;
    adopt = carried && !c->sh_grad_valid && !constraint && c->sh_chain.stepper == sp->stepper &&
            c->sh_chain.use_history == use_history;
    if (!adopt) {
      // the caller wants another pass than the one that ran (stepper reset or changed in between): let its exchange
      // finish -- every rank does -- and start over; the ordinary path below overwrites G and D
      rc = shard_exchange_take(c, c->sh_chain.xticket, 0u, false);
      if (rc) return rc;
      ++c->sh_chain_dropped;
    }
  }
  if (!carried) {
    rc = phase_energy(c, mods, false, 0.0, false, false, true);
    if (rc) return rc;
    rc = shard_exchange(c, n_fb, fbufs, SH_ENERGY, penalty);
    if (rc) return rc;
    c->sh_grad_valid = false;
  }
  if (adopt) {
    rc = shard_exchange_take(c, c->sh_chain.xticket, SH_DIR, false);
    if (rc) return rc;
    ++c->sh_chain_adopted;
    fused = true;
    c->carry.last_g = c->buf[MS_BUF_G];
    c->carry.dir_implicit = false;
    c->sh_maxg2_valid = true;  // (the fused epilogue reduced max|g_i|^2 as well, and G's boundary rows went along)
  } else if (carried && c->sh_grad_valid && !constraint && !use_history && c->sh_maxg2_valid) {
    // steepest-descent restart on an unchanged gradient: d = -g.  The last direction exchange carried the
    // finalized gradient rows as well, so G is valid on every row this rank reads and the scalars follow from
    // the ones already folded -- no kernel and, above all, no exchange
    c->carry.dir_implicit = true;
    c->sh_scal[MS_S_GDOTD] = -c->sh_scal[MS_S_GNORM2];
    c->sh_scal[MS_S_MAXD2] = c->sh_scal[MS_S_MAXG2];
    implicit_restart = true;
    rc = MS_OK;
  } else if (carried && c->sh_grad_valid && !constraint) {
    rc = phase_direction(c, sp->stepper, use_history, /*g_finalized=*/true);
  } else if (constraint) {
    rc = phase_gradient(c, mods, c->buf[MS_BUF_G], false);
    if (rc) return rc;
    rc = shard_exchange(c, 0, nullptr, SH_GRAD, true);
    if (rc) return rc;
    rc = phase_direction(c, sp->stepper, use_history);
  } else {
    const int dir_mode = (cg && use_history) ? 2 : 1;
    rc = phase_gradient(c, mods, c->buf[MS_BUF_G], false, dir_mode);
    fused = true;  // (its epilogue also reduced max|g_i|^2)
  }
  if (rc) return rc;
  if (!implicit_restart && !adopt) {
    // without a constraint row the fused pass has just finalized G: send its boundary rows along with D's, so a
    // steepest-descent restart after a failed search needs no exchange of its own
    const bool with_g = !constraint;
    rc = shard_exchange(c, with_g ? 2 : 1, dbuf, SH_DIR, false);
    if (rc) return rc;
    c->sh_maxg2_valid = with_g && fused;
  }
  c->sh_carry_valid = carry_mode;
  c->sh_grad_valid = carry_mode && !constraint;
  const double E_eval = shard_energy(c);
  const double grad_norm = std::sqrt(c->sh_scal[MS_S_GNORM2]);
  const double g_dot_d = c->sh_scal[MS_S_GDOTD];
  const double max_dir = std::sqrt(c->sh_scal[MS_S_MAXD2]);
  out->energy_eval = E_eval;
  out->grad_norm = grad_norm;
  out->g_dot_d = g_dot_d;
  out->volume = c->sh_scal[MS_S_VOL];
  out->next_step = step_size;
  out->energy = E_eval;
  if (grad_norm < tol) {
    out->converged = out->success = 1;
    return MS_OK;
  }
  double energy0 = E_eval;
  if (sp->reuse_energy0 == 0) {
    rc = phase_energy(c, mods, false, 0.0, false, false, false);
    if (rc) return rc;
    rc = shard_exchange(c, 0, nullptr, SH_ENERGY, false);
    if (rc) return rc;
    energy0 = shard_energy(c);
  }
  const double min_edge = c->til.nf > 0 ? std::sqrt(c->sh_scal[MS_S_MINEDGE2]) : 0.0;
  out->energy = energy0;
  const double safe_limit = min_edge > 0.0 ? 0.3 * min_edge : INFINITY;
  if (g_dot_d >= 0.0) return MS_OK;
  double alpha = step_size;
  if (sp->edge_fraction > 0.0 && min_edge > 0.0 && max_dir > 0.0)
    alpha = std::min(alpha, sp->edge_fraction * min_edge / max_dir);
  const double alpha_max = sp->alpha_max_factor * step_size;
  const int max_iter = sp->max_iter > 0 ? sp->max_iter : 10;
  // line-search history (same bookkeeping as ms_step: prediction only)
  double min_rejected = INFINITY, a_hi, r_lo;
  ms_ctx::LsHist& lh = c->ls[use_history ? 1 : 0];
  ls_bounds(lh, a_hi, r_lo);
  auto remember = [&](double alpha_acc) {
    lh.acc[lh.n % ms_ctx::LS_HIST] = alpha_acc;
    lh.rej[lh.n % ms_ctx::LS_HIST] = min_rejected;
    ++lh.n;
  };
  // ---- the chain behind a trial's exchange (see ms_ctx::shard_chain_enable) ---------------------------------------------
  const bool chain_ok = c->shard_chain_enable && c->peer_on && !c->peer_barrier &&
                        c->d_peer_flagtab != nullptr && carry_mode && !constraint && !penalty && sp->edge_fraction <= 0.0;
  bool chained = false;            // the exchange in flight has the chain behind it
  unsigned long long chain_ticket = 0;
  bool chain_next_hist = false;
  const int pbufs[4] = {MS_BUF_FK, MS_BUF_FA, SH_BUF_FK2, SH_BUF_FA2};
  auto chain_buffers = [&]() -> int {
    if (c->d_sh_dec) return MS_OK;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_sh_dec), sizeof(uint32_t) * MS_DEC_STRIDE * 2));
    HIPCHK(c, hipMemset(c->d_sh_dec, 0, sizeof(uint32_t) * MS_DEC_STRIDE * 2));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_sh_post), sizeof(unsigned long long) * 4, hipHostMallocMapped));
    for (int k = 0; k < 4; ++k) c->h_sh_post[k] = 0;
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_h_sh_post), c->h_sh_post, 0));
    return MS_OK;
  };
  // stage records: a launch gated on a decision word of the chain (nullptr: ungated) ...
  auto gated_stage = [](const uint32_t* gate) {
    StageCtl st;
    st.cur_gate = gate;
    st.cur_gate_want = DEC_ACCEPT_MAIN;
    st.cur_check_ran = true;
    return st;
  };
  // ... and the pair launch: the other trial's fold goes to the SH_ALT slots of the device scalars and travels in the
  // exchange header (the driver waits on neither of the side set's mailboxes: parity stays 0)
  auto pair_stage = [&](double alpha0) {
    StageCtl st = gated_stage(nullptr);
    st.pair_on = 2;
    st.pair_alpha[0] = alpha0;
    st.pair_scal2 = c->d_scal + SH_ALT;
    return st;
  };
  auto slab_of = [&](unsigned long long peer_ticket) {
    return c->d_peer_slab + (size_t)(peer_ticket % PEER_SLABS) * c->shard_count * c->peer_stride;
  };
  // queue a trial's exchange and, when chain: the device-side decision and what an acceptance of the MAIN trial is
  // followed by; then take the exchange's headers.
  auto trial_exchange = [&](int nb, const int* bufs, bool fold_alt, double a_main, double a_alt, bool chain) -> int {
    unsigned long long tk = 0;
    int r2 = MS_OK;
    chained = false;
    if (!chain) {
      r2 = shard_exchange_queue(c, nb, bufs, &tk);
      if (r2) return r2;
    }
    if (chain) {
      r2 = chain_buffers();
      if (r2) return r2;
      c->sh_widx ^= 1;
      ShardDecideArgs da;
      da.recv = slab_of(c->peer_ticket + 1);  // (the exchange queued below; its unpack kernel takes the decision)
      da.stride = c->peer_stride;
      da.world = c->shard_count;
      da.has_alt = fold_alt ? 1 : 0;
      da.alt_off = SH_ALT;
      da.slot_a = (mods & MS_MOD_SURFACE) ? (int)MS_S_ESURF : -1;
      da.slot_b = bend ? (int)MS_S_EBEND : -1;
      da.rhs_alt = energy0 + sp->c * a_alt * g_dot_d;
      da.rhs_main = energy0 + sp->c * a_main * g_dot_d;
      da.dec_out = c->d_sh_dec + (size_t)MS_DEC_STRIDE * c->sh_widx;
      da.post = c->d_h_sh_post + 2 * c->sh_widx;
      da.ticket = ++c->sh_post_ticket;
      c->sh_post_expect[c->sh_widx] = da.ticket;
      r2 = shard_exchange_queue(c, nb, bufs, &tk, nullptr, 0, &da);
      if (r2) return r2;
      const uint32_t* gate = c->d_sh_dec + (size_t)MS_DEC_STRIDE * c->sh_widx;
      // (a) the commit: x <- x + alpha d on the rows this rank reads (ms_phase_commit_trial's launch)
      const Tiling& t = c->til;
      const int64_t rows_per = (int64_t)t.tiles_per_shard * t.own;
      HIPCHK(c, launch_axpy_rows(c->shard_rank * rows_per, (c->shard_rank + 1) * rows_per, c->d_halo_rows, c->n_halo_rows,
                                 c->d_vflags, c->buf[MS_BUF_X], trial_dir(c), trial_alpha(c, a_main), c->stream, gate,
                                 DEC_ACCEPT_MAIN));
      // (b) the gradient + direction pass in the state the acceptance produces (CG history swapped, the trial's
      // factors valid), every change of the context undone afterwards; (c) its exchange
      // (of the carried state the pass writes last_g, dir_implicit and dir_unwritten -- false before and after: no
      // sharded pass leaves D unstored -- and the exchange nothing, so the record is copied out and back whole)
      chain_next_hist = next_use_history(c, cg, restart);
      const CarryState s_carry = c->carry;
      if (cg) {
        std::swap(c->buf[MS_BUF_G], c->buf[MS_BUF_PG]);
        std::swap(c->buf[MS_BUF_D], c->buf[MS_BUF_PD]);
        c->carry.pd_neg_pg = c->carry.dir_implicit;
      }
      c->carry.factors_valid = true;
      {
        StageScope scope(c, gated_stage(gate));
        r2 = phase_gradient(c, mods, c->buf[MS_BUF_G], false, chain_next_hist ? 2 : 1);
      }
      if (r2 == MS_OK) r2 = shard_exchange_queue(c, 2, dbuf, &chain_ticket, gate, DEC_ACCEPT_MAIN);
      if (cg) {
        std::swap(c->buf[MS_BUF_G], c->buf[MS_BUF_PG]);
        std::swap(c->buf[MS_BUF_D], c->buf[MS_BUF_PD]);
      }
      c->carry = s_carry;
      if (r2) return r2;
      chained = true;
      ++c->sh_chained;
    }
    return shard_exchange_take(c, tk, SH_ENERGY, false, fold_alt);
  };
  // the device's decision against the host's (the chain ran iff the code says the main trial was accepted)
  auto verify_chain = [&](uint32_t host_code) -> int {
    if (!chained) return MS_OK;
    const unsigned long long* box = c->h_sh_post + 2 * c->sh_widx;
    const unsigned long long want = c->sh_post_expect[c->sh_widx];
    unsigned long long bits = 0;
    bool ok = false;
    for (long spin = 0; spin < 20000000L && !ok; ++spin) {
      bits = __atomic_load_n(&box[0], __ATOMIC_ACQUIRE);
      ok = (bits ^ __atomic_load_n(&box[1], __ATOMIC_ACQUIRE)) == want;
      if (!ok) __builtin_ia32_pause();
    }
    if (!ok) {
      HIPCHK(c, hipStreamSynchronize(S(c)));
      bits = __atomic_load_n(&box[0], __ATOMIC_ACQUIRE);
      if ((bits ^ __atomic_load_n(&box[1], __ATOMIC_ACQUIRE)) != want)
        return fail(c, MS_ERR_STATE, "sharded step: the device-side decision of a trial never arrived");
    }
    return verify_decision(c, host_code, (uint32_t)bits, "a sharded trial (shard_decide)");
  };
  auto accepted = [&](double alpha_acc, double E_t) -> int {
    int r2;
    if (chained) {
      // the commit ran behind the device's decision: only the bookkeeping of ms_phase_commit_trial is left, and the
      // next step finds its gradient + direction pass queued
      std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);
      r2 = ms_phase_accept(c, cg ? 1 : 0);
      c->sh_chain.valid = true;
      c->sh_chain.stepper = sp->stepper;
      c->sh_chain.use_history = chain_next_hist;
      c->sh_chain.xticket = chain_ticket;
      ++c->sh_chain_ran;
    } else {
      r2 = ms_phase_commit_trial(c, alpha_acc, cg ? 1 : 0);
    }
    if (r2) return r2;
    c->sh_grad_valid = false;
    if (carry_mode) {
      c->carry.factors_valid = true;
      if (penalty)
        HIPCHK(c, hipMemcpyAsync(c->d_scal, c->sh_scal, sizeof(double) * MS_NSCAL, hipMemcpyHostToDevice,
                                 S(c)));
      c->sh_carry_valid = true;
    }
    out->success = 1;
    out->alpha = alpha_acc;
    out->energy = E_t;
    out->volume = c->sh_scal[MS_S_VOL];
    out->next_step = std::min(alpha_acc * sp->gamma, alpha_max);
    remember(alpha_acc);
    return MS_OK;
  };
  int it0 = 0;
  // pair launch (DESIGN.md section 4): trial 0 is expected to fail -> trials 0 and 1 in one energy launch and ONE
  // exchange (both trials' scalars in the header, both factor sets' boundary rows behind it)
  const bool pair = c->pair_enable && carry_mode && bend && !penalty && max_iter >= 2 &&
                    alpha * max_dir < safe_limit && alpha * sp->beta >= 1e-8 &&
                    (c->pair_force || (lh.n >= 2 && alpha > 1.05 * a_hi && r_lo < INFINITY));
  if (pair) {
    rc = spec_prepare(c);
    if (rc) return rc;
    const double alpha0 = alpha, alpha1 = alpha * sp->beta;
    {
      StageScope scope(c, pair_stage(alpha0));
      rc = phase_energy(c, mods, true, alpha1, false, false, true);
      if (rc) return rc;
    }
    c->sh_carry_valid = false;
    rc = trial_exchange(4, pbufs, /*fold_alt=*/true, alpha1, alpha0, chain_ok);
    if (rc) return rc;
    ++out->trials;
    const double E0 = shard_energy_of(c, c->sh_scal2);
    {
      const double E1p = shard_energy(c);
      rc = verify_chain(E0 <= energy0 + sp->c * alpha0 * g_dot_d ? DEC_ACCEPT_SIDE
                        : (E1p <= energy0 + sp->c * alpha1 * g_dot_d ? DEC_ACCEPT_MAIN : DEC_CONTINUE));
      if (rc) return rc;
    }
    if (E0 <= energy0 + sp->c * alpha0 * g_dot_d) {
      chained = false;  // (the chain stayed out: it follows the MAIN trial only)
      // the unexpected case: trial 0's factors (boundary rows included) are in the second set
      const size_t nvp = (size_t)c->til.nvp;
      HIPCHK(c, hipMemcpyAsync(c->buf[MS_BUF_FK], c->fK2, sizeof(double) * 3 * nvp, hipMemcpyDeviceToDevice, S(c)));
      HIPCHK(c, hipMemcpyAsync(c->buf[MS_BUF_FA], c->fA2, sizeof(double) * 2 * nvp, hipMemcpyDeviceToDevice, S(c)));
      for (int sl : {(int)MS_S_ESURF, (int)MS_S_VOL, (int)MS_S_EBEND, (int)MS_S_MINEDGE2}) c->sh_scal[sl] = c->sh_scal2[sl];
      return accepted(alpha0, E0);
    }
    min_rejected = alpha0;
    ++out->trials;
    const double E1 = shard_energy(c);
    if (E1 <= energy0 + sp->c * alpha1 * g_dot_d) return accepted(alpha1, E1);
    chained = false;
    min_rejected = alpha1;
    alpha = alpha1 * sp->beta;
    it0 = 2;
    if (alpha < 1e-8) it0 = max_iter;
  }
  for (int it = it0; it < max_iter; ++it) {
    const bool safe_small = alpha * max_dir < safe_limit;
    rc = phase_energy(c, mods, true, alpha, false, !safe_small, carry_mode);
    if (rc) return rc;
    if (carry_mode) c->sh_carry_valid = false;  // the factor buffers now belong to the trial point
    rc = trial_exchange(carry_mode ? n_fb : 0, fbufs, false, alpha, 0.0, chain_ok && safe_small);
    if (rc) return rc;
    if (chained) {
      rc = verify_chain(shard_energy(c) <= energy0 + sp->c * alpha * g_dot_d ? DEC_ACCEPT_MAIN : DEC_CONTINUE);
      if (rc) return rc;
    }
    if (!safe_small && c->sh_scal[MS_S_GUARD] > 0.0) {
      ++out->guard_rejects;
      min_rejected = alpha;
      alpha *= sp->beta;
      if (alpha < 1e-8) break;
      continue;
    }
    ++out->trials;
    const double E_t = shard_energy(c);
    if (E_t <= energy0 + sp->c * alpha * g_dot_d) return accepted(alpha, E_t);
    chained = false;
    min_rejected = alpha;
    alpha *= sp->beta;
    if (alpha < 1e-8) break;
  }
  out->next_step = std::max(std::max(alpha * sp->beta, 0.0), step_size * sp->beta);
  return MS_OK;
}
