// The one-workgroup interpreter (included at the end of ms_kernels.hip, inside namespace ms: it instantiates the device
// bodies defined there).  See ms_internal.h, "the one-workgroup interpreter", for what it is for.
//
// Pack layout (the kernel-argument block of one k_exec launch):
//   ExecPackHead { n_cmds, bytes, T, DeviceMesh m[EXEC_MESHES] } | record 0 | record 1 | ...
//   record = ExecCmdHead | the kernel's argument struct (tile kernels: without its leading DeviceMesh)
// Everything the interpreter reads from the pack is a scalar load from the constant address space: the argument values
// stay in SGPRs exactly as they do in the ordinary kernels.  Each body runs in a function of its own (noinline): the
// interpreter kernel itself is a loop over a switch, and a body is compiled once.

typedef const __attribute__((address_space(4))) unsigned char* exec_kptr;
// (attribute hook of the body functions; empty: amdgpu_flat_work_group_size applies to kernels only)
#define MS_EXEC_FN

// The pack's address.  Only the KERNEL may ask for its argument segment (inside a callable function the compiler folds
// __builtin_amdgcn_kernarg_segment_ptr() to null): the body functions get the address as an ordinary argument -- which
// arrives in vector registers -- and make it uniform again, so that everything read through it is a scalar load.
__device__ __forceinline__ exec_kptr exec_uniform_ptr(exec_kptr p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(v >> 32));
  return (exec_kptr)(((unsigned long long)hi << 32) | lo);
}
// a trivially copyable struct from the pack; SKIP leading bytes of the destination are left alone
template <int SKIP, typename A>
__device__ __forceinline__ void exec_load(A& dst, exec_kptr src) {
  static_assert(SKIP % 8 == 0 && sizeof(A) % 8 == 0, "8-byte granules");
  typedef const __attribute__((address_space(4))) unsigned long long* q8;
  unsigned long long w[(sizeof(A) - SKIP) / 8];
#pragma unroll
  for (int i = 0; i < (int)((sizeof(A) - SKIP) / 8); ++i) w[i] = ((q8)src)[i];
  __builtin_memcpy(reinterpret_cast<char*>(&dst) + SKIP, w, sizeof(A) - SKIP);
}
__device__ __forceinline__ int exec_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

static_assert(offsetof(EnergyArgs, m) == 0 && offsetof(GradientArgs, m) == 0 && offsetof(TiltArgs, m) == 0 &&
                  offsetof(BtArgs, m) == 0 && offsetof(TsArgs, m) == 0,
              "the tile kernels' argument structs start with their DeviceMesh");
static_assert(sizeof(DeviceMesh) % 8 == 0, "DeviceMesh is a whole number of 8-byte granules");

// arguments of a tile kernel: the mesh from the pack head, the rest from the record
template <typename A>
__device__ __forceinline__ void exec_tile_args(A& a, ExecCmdHead& h, exec_kptr base, int off) {
  exec_load<0>(h, base + off);
  const int mi = h.mesh;
  // (selected with constant indices: the three meshes are ~0.5 KB of scalar loads, only one is kept)
  DeviceMesh m;
  exec_load<0>(m, base + offsetof(ExecPackHead, m) + (size_t)mi * sizeof(DeviceMesh));
  a.m = m;
  exec_load<(int)sizeof(DeviceMesh)>(a, base + off + sizeof(ExecCmdHead));
}
template <typename A>
__device__ __forceinline__ void exec_plain_args(A& a, ExecCmdHead& h, exec_kptr base, int off) {
  exec_load<0>(h, base + off);
  exec_load<0>(a, base + off + sizeof(ExecCmdHead));
}

// ---- one function per body ------------------------------------------------------------------------------------------
// A record of a tile kernel: body(a, h, lds, b) for block 0 .. h.grid-1 in turn, a barrier after each.  Instantiated once
// per body (every lambda below is a type of its own), never inlined.
template <typename A, typename Body>
__device__ __noinline__ MS_EXEC_FN void exec_tile(exec_kptr base_v, int off_v, double* lds, Body body) {
  const exec_kptr base = exec_uniform_ptr(base_v);
  const int off = exec_uniform(off_v);
  A a;
  ExecCmdHead h;
  exec_tile_args(a, h, base, off);
  for (int b = 0; b < h.grid; ++b) {
    body(a, h, lds, b);
    __syncthreads();
  }
}
// A record of a stream kernel.  EXEC_PER_BLOCK: as above; EXEC_BLOCKS: the blocks touch disjoint rows, one barrier
// after the last; EXEC_ONCE: body(a, h, h.grid) covers the whole launch itself.
enum ExecLoop { EXEC_PER_BLOCK, EXEC_BLOCKS, EXEC_ONCE };
template <typename A, ExecLoop LOOP, typename Body>
__device__ __noinline__ MS_EXEC_FN void exec_plain(exec_kptr base_v, int off_v, Body body) {
  const exec_kptr base = exec_uniform_ptr(base_v);
  const int off = exec_uniform(off_v);
  A a;
  ExecCmdHead h;
  exec_plain_args(a, h, base, off);
  if constexpr (LOOP == EXEC_ONCE) {
    body(a, h, h.grid);
  } else {
    for (int b = 0; b < h.grid; ++b) {
      body(a, h, b);
      if constexpr (LOOP == EXEC_PER_BLOCK) __syncthreads();
    }
  }
  if constexpr (LOOP != EXEC_PER_BLOCK) __syncthreads();
}

// one record (ExecRecorder::push has refused an energy / gradient instance that visit_instance<true> does not have)
__device__ __forceinline__ void exec_dispatch(exec_kptr base, int off, double* lds) {
  ExecCmdHead h;
  exec_load<0>(h, base + off);
  switch (h.kind) {
    case CK_ENERGY:
      visit_instance<true>(EnergyInst::from_code(h.inst), [&](auto tag) {
        using I = decltype(tag);
        exec_tile<EnergyArgs>(base, off, lds, [](const EnergyArgs& a, const ExecCmdHead& h, double* lds, int b) {
          EnergyArgs c = a;  // (energy_body changes its arguments: every block starts from the record's)
          energy_body<I::d.bend, I::d.guard, 256, 0, I::d.atomic, 0, I::d.area>(c, h.cap, h.max_ent, lds, b);
        });
      });
      break;
    case CK_GRADIENT:
      visit_instance<true>(GradientInst::from_code(h.inst), [&](auto tag) {
        using I = decltype(tag);
        exec_tile<GradientArgs>(base, off, lds, [](const GradientArgs& a, const ExecCmdHead& h, double* lds, int b) {
          gradient_body<I::d.mode, I::d.volrow, I::d.fast ? 256 : 0, 0, I::d.atomic, I::d.lean, I::d.area>(a, h.cap, h.max_ent, lds, b);
        });
      });
      break;
    case CK_TILT:
      pick_int<0, 1, 2, 3, 4, 5>(h.mode, [&](auto M) {
        exec_tile<TiltArgs>(base, off, lds, [](const TiltArgs& a, const ExecCmdHead& h, double* lds, int b) {
          tilt_body<decltype(M)::value>(a, h.cap, h.max_ent, lds, b);
        });
      });
      break;
    case CK_BT:
      pick_int<0, 1, 2, 3>(h.mode, [&](auto M) {
        exec_tile<BtArgs>(base, off, lds, [](const BtArgs& a, const ExecCmdHead& h, double* lds, int b) {
          bt_body<decltype(M)::value>(a, h.cap, h.max_ent, lds, b);
        });
      });
      break;
    case CK_TS:
      pick_int<0, 1, 2>(h.mode, [&](auto M) {
        exec_tile<TsArgs>(base, off, lds, [](const TsArgs& a, const ExecCmdHead& h, double* lds, int b) {
          ts_body<decltype(M)::value>(a, h.cap, h.max_ent, lds, b);
        });
      });
      break;
    case CK_TSEARCH:
      pick_int<1, 2>(h.mode, [&](auto NF) {
        exec_tile<TsearchArgs>(base, off, lds, [](const TsearchArgs& a, const ExecCmdHead& h, double* lds, int b) {
          tsearch_body<decltype(NF)::value, 1>(a, h.cap, lds, b);
        });
      });
      break;
    case CK_TVEC:
      exec_plain<TvecArgs, EXEC_PER_BLOCK>(base, off, [](const TvecArgs& a, const ExecCmdHead&, int b) { tvec_body(a, b); });
      break;
    case CK_DISK:
      exec_plain<DiskTargetArgs, EXEC_PER_BLOCK>(
          base, off, [](const DiskTargetArgs& a, const ExecCmdHead& h, int b) { disk_target_body(a, h.mode, b); });
      break;
    case CK_REDUCE:
      // (one tile: every task of the fold at once, thread t = task t; ExecRecorder only exists for one-tile contexts)
      exec_plain<FoldArgs, EXEC_ONCE>(base, off, [](const FoldArgs& a, const ExecCmdHead&, int grid) { reduce_one_tile(a, grid); });
      break;
    case CK_DIRECTION:
      exec_plain<DirectionArgs, EXEC_PER_BLOCK>(base, off, [](const DirectionArgs& a, const ExecCmdHead&, int b) { direction_body(a, b); });
      break;
    case CK_ROWDOT:
      exec_plain<RowDotArgs, EXEC_PER_BLOCK>(base, off, [](const RowDotArgs& a, const ExecCmdHead&, int b) { row_dot_body(a, b); });
      break;
    case CK_AXPY_MASKED:
      exec_plain<AxpyMaskedArgs, EXEC_BLOCKS>(base, off, [](const AxpyMaskedArgs& a, const ExecCmdHead&, int b) { axpy_masked_body(a, b); });
      break;
    case CK_MEMSET:
      exec_plain<ExecMemsetArgs, EXEC_ONCE>(base, off, [](const ExecMemsetArgs& a, const ExecCmdHead&, int) {
        for (int64_t i = threadIdx.x; i < a.n; i += blockDim.x) a.p[i] = 0.0;
      });
      break;
    case CK_PIN_ENFORCE:
      // (both pin bodies are one workgroup of 256 threads with fixed-order trees in 3 * 256 doubles of the block's LDS)
      exec_plain<PinEnforceArgs, EXEC_ONCE>(base, off, [lds](const PinEnforceArgs& a, const ExecCmdHead&, int) {
        pin_dev::pin_enforce_body(a, reinterpret_cast<double(*)[pin_dev::PB]>(lds));
      });
      break;
    case CK_PIN_GRAD:
      exec_plain<PinGradArgs, EXEC_ONCE>(base, off, [lds](const PinGradArgs& a, const ExecCmdHead&, int) {
        pin_dev::pin_grad_body(a, reinterpret_cast<double(*)[pin_dev::PB]>(lds));
      });
      break;
    default: break;  // (CK_RELAX / CK_RELAX_FUSED: k_exec runs them itself)
  }
}

// a list of n records from byte `off` of the pack
// one record, timed when the pack carries a stamp buffer (ms_exec_trace)
__device__ __forceinline__ void exec_run_one(exec_kptr base, int off, double* lds) {
  unsigned long long* const stamps = reinterpret_cast<unsigned long long*>(
      *(const __attribute__((address_space(4))) unsigned long long*)(base + offsetof(ExecPackHead, stamps)));
  if (stamps == nullptr) {
    exec_dispatch(base, off, lds);
    return;
  }
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  exec_dispatch(base, off, lds);
  __syncthreads();
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    ExecCmdHead h;
    exec_load<0>(h, base + off);
    const unsigned long long idx = atomicAdd(stamps, 1ull);
    if (idx + 1 < (unsigned long long)EXEC_STAMP_CAP) {
      stamps[1 + 2 * idx] = ((unsigned long long)h.kind << 32) | (unsigned int)(h.mode & 0xffff) | ((unsigned long long)(h.inst & 0xffu) << 16);
      stamps[2 + 2 * idx] = t1 - t0;
    }
  }
}
__device__ __forceinline__ void exec_run_list(exec_kptr base, int off, int n, double* lds) {
  for (int i = 0; i < n; ++i) {
    exec_run_one(base, off, lds);
    off += (int)((const __attribute__((address_space(4))) unsigned short*)(base + off))[1];
  }
}

// CK_RELAX (ms_internal.h: ExecRelaxHead): relax_fields of ms_api.cpp, statement for statement, with the scalars read
// from the device and the pointer swap of an acceptance expressed as the parity of the lists that run next.  Every
// thread walks the same control flow on the same values (agent-scope loads of what the lists' folds stored).
__device__ __noinline__ void exec_relax(exec_kptr base_v, int off_v, double* lds) {
  const exec_kptr base = exec_uniform_ptr(base_v);
  const int off = exec_uniform(off_v);
  ExecRelaxHead r;
  ExecCmdHead h;
  exec_plain_args(r, h, base, off);
  int par = 0, iters = 0, evals = 0;
  auto energy = [&]() {
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < r.n_e) e += ld_agent(r.scal + r.e_slot[k]);
    return e;
  };
  double gnorm = 0.0, rz = 0.0, E0 = 0.0;
  auto grad_at = [&](double& rz_out) {
    exec_run_list(base, par ? r.off_grad[1] : r.off_grad[0], par ? r.n_grad[1] : r.n_grad[0], lds);
    ++evals;
    E0 = energy();
    double g2 = 0.0, z = 0.0;
    g2 += ld_agent(r.scal + r.s_gn2[0]);
    z += ld_agent(r.scal + r.s_rz[0]);
    if (r.nf > 1) {
      g2 += ld_agent(r.scal + r.s_gn2[1]);
      z += ld_agent(r.scal + r.s_rz[1]);
    }
    gnorm = sqrt(g2);
    rz_out = z;
  };
  // backtracking on E(P(t + step * src)) <= E0, at most 12 halvings (:330-347 / :918-973)
  auto search = [&](double sign) {
    double step = r.step_size;
    for (int bt = 0; bt < 12; ++bt) {
      if (threadIdx.x == 0) st_agent(r.cells, sign * step);
      __syncthreads();
      exec_run_list(base, par ? r.off_trial[1] : r.off_trial[0], par ? r.n_trial[1] : r.n_trial[0], lds);
      ++evals;
      const double E1 = energy();
      if (E1 <= E0) {
        par ^= 1;  // tilts <-> trial
        return true;
      }
      step *= 0.5;
      if (step < 1e-16) break;
    }
    return false;
  };
  const double tol = r.tol > 0.0 ? r.tol : 0.0;
  auto small = [&]() { return gnorm == 0.0 || (tol > 0.0 && gnorm < tol); };
  if (r.solver == 0) {  // gradient descent (:312-351 / :892-1058)
    for (int it = 0; it < r.max_iters; ++it) {
      grad_at(rz);
      if (small()) break;
      const bool acc = search(-1.0);
      ++iters;
      if (!acc) break;
    }
  } else {  // (preconditioned) Fletcher-Reeves CG (:352-421 / :1059-1398)
    double rz_old = 0.0;
    grad_at(rz_old);
    if (!small()) {
      exec_run_list(base, r.off_dir0, r.n_dir0, lds);
      for (int it = 0; it < r.max_iters; ++it) {
        if (small()) break;
        const bool acc = search(1.0);
        ++iters;
        if (!acc) break;
        double rz_new = 0.0;
        grad_at(rz_new);
        if (small()) break;
        if (rz_old == 0.0) break;
        const double beta = rz_new / rz_old;
        if (threadIdx.x == 0) st_agent(r.cells + 1, beta);
        __syncthreads();
        exec_run_list(base, r.off_dir1, r.n_dir1, lds);
        rz_old = rz_new;
      }
    }
  }
  if (threadIdx.x == 0 && r.host_box != nullptr) {
    post_entry(r.host_box, 0, (unsigned long long)iters, r.ticket);
    post_entry(r.host_box, 1, (unsigned long long)evals, r.ticket);
    post_entry(r.host_box, 2, (unsigned long long)par, r.ticket);
    post_entry(r.host_box, 3, 1ull, r.ticket);
  }
  __syncthreads();
}

#include "ms_relax_fused.inc"

template <int NB>
struct ExecPackArg {
  unsigned char b[NB];
};
// blockDim.x = T = 256 (= BLOCK: the stream bodies assume it)
template <int NB>
__global__ __launch_bounds__(256) void k_exec(ExecPackArg<NB> pack) {
  extern __shared__ double lds[];
  (void)pack;  // (read through the kernel-argument segment pointer, with scalar loads at uniform offsets)
  const exec_kptr base = (exec_kptr)__builtin_amdgcn_kernarg_segment_ptr();
  typedef const __attribute__((address_space(4))) int* qi;
  const int n = ((qi)base)[0];
  int off = (int)sizeof(ExecPackHead);
  for (int i = 0; i < n; ++i) {
    ExecCmdHead h;
    exec_load<0>(h, base + off);
    if (h.kind == CK_RELAX) {
      exec_relax(base, off, lds);
      off += h.pad;  // (the record and its lists)
    } else if (h.kind == CK_RELAX_FUSED) {
      exec_relax_fused(base, off, lds);
      off += (int)h.bytes;
    } else {
      exec_run_one(base, off, lds);
      off += (int)h.bytes;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {
constexpr int EXEC_SLOTS = 32;
std::atomic<ExecRecorder*> g_exec_slots[EXEC_SLOTS];
std::atomic<int> g_exec_count{0};
bool same_mesh(const DeviceMesh& a, const DeviceMesh& b) {
  return a.nv == b.nv && a.T == b.T && a.n_tiles == b.n_tiles && a.own == b.own && a.has_boundary == b.has_boundary &&
         a.tile_facet_off == b.tile_facet_off && a.tile_facets == b.tile_facets && a.tile_facets32 == b.tile_facets32 &&
         a.tile_facets_lean == b.tile_facets_lean &&
         a.no_fast == b.no_fast && a.tf_gamma == b.tf_gamma && a.gamma_uniform == b.gamma_uniform &&
         a.kc_uniform == b.kc_uniform && a.gamma_const == b.gamma_const && a.kappa_const == b.kappa_const &&
         a.c0_const == b.c0_const && a.tile_halo_off == b.tile_halo_off && a.halo_ids == b.halo_ids &&
         a.tile_ent_off == b.tile_ent_off && a.tile_voff == b.tile_voff && a.vent == b.vent && a.vflags == b.vflags &&
         a.kappa == b.kappa && a.c0 == b.c0;
}
}  // namespace

ExecRecorder* exec_find(hipStream_t s) {
  if (g_exec_count.load(std::memory_order_acquire) == 0) return nullptr;
  for (int i = 0; i < EXEC_SLOTS; ++i) {
    ExecRecorder* r = g_exec_slots[i].load(std::memory_order_acquire);
    if (r != nullptr && r->stream == s) return r;
  }
  return nullptr;
}
void exec_attach(ExecRecorder* r) {
  for (int i = 0; i < EXEC_SLOTS; ++i) {
    ExecRecorder* expected = nullptr;
    if (g_exec_slots[i].compare_exchange_strong(expected, r)) {
      g_exec_count.fetch_add(1, std::memory_order_release);
      return;
    }
  }
  // (no slot: the context simply runs launch by launch)
}
void exec_detach(ExecRecorder* r) {
  for (int i = 0; i < EXEC_SLOTS; ++i) {
    ExecRecorder* expected = r;
    if (g_exec_slots[i].compare_exchange_strong(expected, nullptr)) g_exec_count.fetch_sub(1, std::memory_order_release);
  }
}

hipError_t ExecRecorder::push(uint16_t kind, int mode, int cap, int max_ent, int grid, uint32_t inst, size_t lds_bytes,
                              const void* args, size_t bytes, const DeviceMesh* mesh) {
  const size_t skip = mesh ? sizeof(DeviceMesh) : 0;
  const size_t rec = sizeof(ExecCmdHead) + ((bytes - skip + 7) & ~(size_t)7);
  if (sizeof(ExecPackHead) + rec > (size_t)EXEC_PACK_BYTES) return hipErrorInvalidValue;
  // (an instance exec_dispatch does not have would run nothing)
  if (kind == CK_ENERGY && !EnergyInst::from_code(inst).in_exec()) return hipErrorInvalidValue;
  if (kind == CK_GRADIENT && !GradientInst::from_code(inst).in_exec()) return hipErrorInvalidValue;
  const size_t limit = capture ? (size_t)EXEC_PACK_BIG : (size_t)EXEC_PACK_BYTES;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (buf.empty()) {
      buf.assign(sizeof(ExecPackHead), 0);
      n_mesh = 0;
      lds = 0;
    }
    int mi = -1;
    ExecPackHead* ph = reinterpret_cast<ExecPackHead*>(buf.data());
    if (mesh) {
      for (int k = 0; k < n_mesh && mi < 0; ++k)
        if (same_mesh(ph->m[k], *mesh)) mi = k;
      if (mi < 0 && n_mesh < EXEC_MESHES) {
        mi = n_mesh++;
        ph->m[mi] = *mesh;
      }
    } else {
      mi = 0;
    }
    if (mi >= 0 && buf.size() + rec <= limit) {
      ExecCmdHead h;
      memset(&h, 0, sizeof(h));
      h.kind = kind;
      h.bytes = (uint16_t)rec;
      h.mode = mode;
      h.cap = cap;
      h.max_ent = max_ent;
      h.grid = grid;
      h.inst = inst;
      h.mesh = mi;
      const size_t at = buf.size();
      buf.resize(at + rec, 0);
      memcpy(buf.data() + at, &h, sizeof(h));
      memcpy(buf.data() + at + sizeof(h), static_cast<const unsigned char*>(args) + skip, bytes - skip);
      ph = reinterpret_cast<ExecPackHead*>(buf.data());
      ph->n_cmds += 1;
      lds = std::max(lds, lds_bytes);
      ++cmds;
      return hipSuccess;
    }
    if (capture) return hipErrorInvalidValue;  // (a program that does not fit: the caller falls back)
    const hipError_t e = flush();  // full (or a fourth mesh): launch what there is, start a new pack
    if (e != hipSuccess) return e;
  }
  return hipErrorInvalidValue;
}

hipError_t ExecRecorder::flush() {
  if (capture || buf.empty()) return hipSuccess;
  ExecPackHead* ph = reinterpret_cast<ExecPackHead*>(buf.data());
  if (ph->n_cmds == 0) {
    buf.clear();
    return hipSuccess;
  }
  std::vector<unsigned char> pack;
  pack.swap(buf);
  return launch_pack(pack, lds);
}

namespace {
template <int NB>
hipError_t exec_launch_n(const std::vector<unsigned char>& pack, size_t need, int T, hipStream_t stream) {
  static ExecPackArg<NB> arg;  // (the tail of the block is never read: no need to clear it; copied at launch)
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  memcpy(arg.b, pack.data(), pack.size());
  // (the LDS attribute is raised once per size class, not looked at on every launch)
  static size_t lds_allowed = 48 * 1024;
  if (need > lds_allowed) {
    const size_t want = std::max(need, (size_t)152 * 1024);
    hipError_t e = ensure_lds(k_exec<NB>, want);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      e = ensure_lds(k_exec<NB>, need);
      if (e != hipSuccess) return e;
      lds_allowed = need;
    } else {
      lds_allowed = want;
    }
  }
  hipLaunchKernelGGL((k_exec<NB>), dim3(1), dim3(T), need, stream, arg);
  return hipGetLastError();
}
}  // namespace

// MS_EXEC_TIMING=1: host time spent inside launch_pack (pack copy + hipLaunchKernelGGL), reported at process exit
namespace {
struct ExecHostTiming {
  bool on = getenv("MS_EXEC_TIMING") != nullptr && atoi(getenv("MS_EXEC_TIMING")) != 0;
  double sum_us = 0.0, max_us = 0.0;
  long n = 0;
  ~ExecHostTiming() {
    if (on && n > 0)
      fprintf(stderr, "[ms exec timing] %ld k_exec launches: %.2f us of host time per launch on average (max %.1f)\n", n,
              sum_us / n, max_us);
  }
} g_exec_timing;
}  // namespace

hipError_t ExecRecorder::launch_pack(const std::vector<unsigned char>& pack_in, size_t lds_bytes) {
  struct timespec ts0;
  if (g_exec_timing.on) clock_gettime(CLOCK_MONOTONIC, &ts0);
  struct Lap {
    const struct timespec* t0;
    ~Lap() {
      if (!g_exec_timing.on) return;
      struct timespec t1;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      const double us = 1e6 * (double)(t1.tv_sec - t0->tv_sec) + 1e-3 * (double)(t1.tv_nsec - t0->tv_nsec);
      g_exec_timing.sum_us += us;
      g_exec_timing.max_us = std::max(g_exec_timing.max_us, us);
      ++g_exec_timing.n;
    }
  } lap{&ts0};
  std::vector<unsigned char> pack = pack_in;
  ExecPackHead* ph = reinterpret_cast<ExecPackHead*>(pack.data());
  ph->bytes = (int32_t)pack.size();
  ph->T = T;
  ph->stamps = d_stamps;
  const size_t need = std::max<size_t>(lds_bytes, 64);
  ++launches;
  if (pack.size() <= (size_t)EXEC_PACK_BYTES) return exec_launch_n<EXEC_PACK_BYTES>(pack, need, T, stream);
  if (pack.size() <= (size_t)EXEC_PACK_MID) return exec_launch_n<EXEC_PACK_MID>(pack, need, T, stream);
  if (pack.size() <= (size_t)EXEC_PACK_BIG) return exec_launch_n<EXEC_PACK_BIG>(pack, need, T, stream);
  return hipErrorInvalidValue;
}

size_t relax_fused_lds_bytes(int cap, int max_ent, int max_tile_facets) {
  const size_t nfs = ((size_t)max_tile_facets + 1) & ~(size_t)1;
  size_t b = sizeof(double) * (15 * (size_t)cap + 16 * nfs + 9 * 256 + 12 * 16);
  b += 2 * (256 + 2 + (((size_t)max_ent + 3) & ~(size_t)3));
  b += sizeof(TileFacet) * nfs;
  b += (((size_t)cap + 15) / 16) * 16;
  return b + 64;
}
