// Host side of the "wg" mapping (tick_wg.hip.h): owns the instance-major HBM state of the batch,
// computes the batch-wide scalars of each tick (t, dtau) and launches one kernel per control tick.
#pragma once
#include <vector>
#include "ctx_common.hip.h"
#include "stage_own.hip.h"
#include "tick_wave.hip.h"
#include "tick_wg.hip.h"
#include "wg_plan.hip.h"
#include "ctx_host.hip.h"

namespace cgm {

template <class T>
__global__ void replicate_rows_im(T* __restrict__ dst, size_t dst_pitch, const T* __restrict__ src, int B, int n,
                                  int reps, int bcast) {
  // dst[b][rep*n + j] = src[(bcast ? 0 : b)*n + j]
  const int b = blockIdx.y;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n * reps; q += gridDim.x * blockDim.x)
    if (b < B) dst[size_t(b) * dst_pitch + q] = src[size_t(bcast ? 0 : b) * n + (q % n)];
}

template <class M, class T>
struct CtxWg final : CtxHost<M, T, CtxWg<M, T>> {
  using Host = CtxHost<M, T, CtxWg<M, T>>;
  using Host::cfg, Host::nx, Host::nu, Host::np, Host::L, Host::stream, Host::dalloc, Host::grow, Host::init_common;
  using Host::t, Host::dtau_of, Host::stage, Host::stage_n, Host::stage2, Host::stage2_n, Host::x_dev, Host::u_dev;
  WgParams<T> P{};
  int ks_all = 0;
  WgPlanResult plan{};  // what plan_wg (wg_plan.hip.h) decided for this batch
  void (*k_tick)(WgParams<T>) = nullptr;
  void (*k_hook)(WgParams<T>) = nullptr;
  // control() through host pointers on a small batch (a single Cgmres<Model> object: batch 1): x and u travel through
  // host-mapped pinned buffers the kernel reads / writes directly — one launch + one stream synchronisation per tick
  // instead of copy, launch, copy, synchronise (each hipMemcpyAsync costs ~8 us of host time)
  T *pin_x = nullptr, *pin_u = nullptr, *pin_x_dev = nullptr, *pin_u_dev = nullptr;
  static constexpr int kPinnedIoMaxBatch = 1024;
  ~CtxWg() override {
    (void)hipSetDevice(cfg.device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (pin_x) (void)hipHostFree(pin_x);
    if (pin_u) (void)hipHostFree(pin_u);
  }
  // The Krylov rows in HBM follow the ownership of the kernel that wrote them last: the row-parallel Newton kernel keeps
  // its vectors by stage (stage_own.hip.h), every other kernel of this context — the white-box hooks included — by rows
  // (WgCtx::load_vec).  get_krylov un-permutes accordingly.
  bool v_by_stage = false;
  int* perm_dev = nullptr;   // placement of the next fused launch (bin_by_count_kernel)
  PlantSeqs<T>* pin_dev = nullptr;  // plant inputs of the next fused launch (closed_loop)
  bool have_counts = false;  // n_ax holds the counts of a finished tick
  using Tr = WgTraits<M, T>;
  const char* variant_name() const override { return wg_variant_name(plan); }

  // WgKernelId -> the kernel instantiations, in one place.  The `if constexpr` guards keep kernels from being
  // instantiated for models that cannot use them (plan_wg goes by the same traits).
  void pick(const WgKernelId& k) {
    if (k.ipw == 16 && k.maxm == 10) pick_wg<16, 10>(k);
    if (k.ipw == 16 && k.maxm == 20) pick_wg<16, 20>(k);
    if (k.ipw == 8 && k.maxm == 10) pick_wg<8, 10>(k);
    if (k.ipw == 8 && k.maxm == 20) pick_wg<8, 20>(k);
    // variant 4 ("wave", tick_wave.hip.h): one wavefront per controller; the tick kernel changes, the HBM state, the
    // white-box hooks and everything else of this context stay those of the wg mapping
    if constexpr (Tr::kWave) {
      if (k.wave) k_tick = tick_wave_kernel<M, T, Tr::kWaveKmax, Tr::kWaveWpb>;
    }
    if constexpr (Tr::kRowScan) {
      if (k.nwt == 2) k_tick = tick_wg_kernel<M, T, 16, 10, false, 0, 2>;
    }
    if constexpr (Tr::kRowNewton) {
      if (k.nwt == 1) k_tick = tick_wg_kernel<M, T, 16, 10, false, 1, 1>;
    }
  }
  // (IPW, MAXM) instantiations: 16 or 8 instances per workgroup, vectors up to 160 or 320 elements; the lean LDS plan
  // (two workgroups per CU) and the chunk-parallel costate sweeps exist for 16 instances per workgroup
  template <int IPW, int MAXM>
  void pick_wg(const WgKernelId& k) {
    k_tick = tick_wg_kernel<M, T, IPW, MAXM>;
    if constexpr (IPW == 16) {
      if (k.lean) k_tick = tick_wg_kernel<M, T, IPW, MAXM, true>;
      if constexpr (Tr::template kParCostate<MAXM>) {
        if (k.par == 1 && !k.lean) k_tick = tick_wg_kernel<M, T, IPW, MAXM, false, 1>;
      }
      if constexpr (Tr::kPar2) {
        if (k.par == 2) k_tick = k.lean ? tick_wg_kernel<M, T, IPW, MAXM, true, 2> : tick_wg_kernel<M, T, IPW, MAXM, false, 2>;
      }
    }
    k_hook = hook_wg_kernel<M, T, IPW, MAXM>;
  }

  int init() override {
    if (int rc = init_common()) return rc;
    nx = M::NX, nu = M::NU, np = M::NP;
    L = nu * cfg.dv;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg.device));
    std::string why;
    if (int rc = plan_wg<M, T>(cfg, cus, &plan, &why)) return fail(rc, "%s", why.c_str());
    cfg.variant = plan.variant;
    const int ipw = plan.k.ipw;
    pick(plan.k);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tick), hipFuncAttributeMaxDynamicSharedMemorySize,
                                int(plan.lds_bytes_tick)));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_hook), hipFuncAttributeMaxDynamicSharedMemorySize,
                                int(plan.lds_bytes_hook)));
    const int k1 = cfg.k_max + 1;
    ks_all = k1 * k1 + k1 + 3 * cfg.k_max;
    P.B = cfg.batch, P.dv = cfg.dv, P.kmax = cfg.k_max, P.L = L, P.fh_hbm = plan.fh_hbm, P.lds_bytes = int(plan.lds_bytes);
    P.cs_chunks = plan.cs_chunks;
    for (int k = 0; k < 8; ++k) P.base_off[k] = plan.base_off[k];
    P.Lp = L | 1, P.Lg = (L + 15) / 16 * 16, P.Lv = plan.k.nwt == 1 ? StageOwn::LV : 16 * plan.k.maxm, P.Pp = (np * (cfg.dv + 1)) | 1, P.Hp = Tr::pitch_H(cfg.k_max);
    P.h = T(cfg.h), P.dt = T(cfg.dt), P.tol = T(cfg.tol);
    P.wave_dbg = ((cfg.flags & CGMRES_HIP_FLAG_WAVE_FRESH_TRIG) ? 1 : 0) | ((cfg.flags & CGMRES_HIP_FLAG_WAVE_SERIAL_SWEEPS) ? 2 : 0);
    P.inv_h = T(1.0) / P.h;
    P.one_m_zh = (1 - T(cfg.zeta) * P.h);
    const size_t B = cfg.batch, Lg = P.Lg, wgs = grid().x;
    int rc = 0;
    if ((rc = dalloc(&P.U, B * Lg)) || (rc = dalloc(&P.dUdt, B * Lg)) || (rc = dalloc(&P.Fh, B * Lg)) ||
        (rc = dalloc(&P.V, B * k1 * size_t(P.Lv))) || (rc = dalloc(&P.xdxh, B * nx)) ||
        (rc = dalloc(&P.ptau, B * size_t(np) * (cfg.dv + 1))) || (rc = dalloc(&P.kry, B * ks_all)) ||
        (rc = dalloc(&P.scr, wgs * Tr::scr_count(ipw, cfg.dv))) ||
        (rc = dalloc(&P.pT, plan.k.lean ? wgs * (cfg.dv + 1) * (np ? np : 1) * ipw : 1)) ||
        (rc = dalloc(&P.park, wgs * ipw * P.Lv)) ||  // (every kernel family parks the solution vector now)
        (rc = dalloc(&P.n_ax, B)) || (rc = dalloc(&P.reason, B)) || (rc = dalloc(&x_dev, B * nx)) ||
        (rc = dalloc(&u_dev, B * nu)) || (rc = dalloc(&perm_dev, B)) || (rc = dalloc(&pin_dev, 1)))
      return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  dim3 grid() const { return dim3((cfg.batch + plan.k.ipw - 1) / plan.k.ipw); }
  dim3 block() const { return dim3(plan.k.ipw * 16); }

  // host [B][n] <-> device rows with pitch
  int rows_h2d(T* dst, size_t pitch, const void* src, int n) {
    HIP_TRY(hipMemcpy2DAsync(dst, pitch * sizeof(T), src, size_t(n) * sizeof(T), size_t(n) * sizeof(T), cfg.batch,
                             hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int rows_d2h(void* dst, const T* src, size_t pitch, int n, size_t rows) {
    if (!dst) return 0;
    HIP_TRY(hipMemcpy2DAsync(dst, size_t(n) * sizeof(T), src, pitch * sizeof(T), size_t(n) * sizeof(T), rows,
                             hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  // host [B or 1][n] -> device rows with pitch, every row's n values repeated reps times (0: once)
  int upload(T* dst, size_t pitch, const void* src, int n, int reps, int per_instance) {
    const size_t cnt = size_t(per_instance ? cfg.batch : 1) * n;
    if (int rc = grow(&stage, &stage_n, cnt)) return rc;
    HIP_TRY(hipMemcpyAsync(stage, src, cnt * sizeof(T), hipMemcpyHostToDevice, stream));
    replicate_rows_im<T><<<dim3(4, cfg.batch), 256, 0, stream>>>(dst, pitch, stage, cfg.batch, n, reps ? reps : 1, !per_instance);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  size_t pitch_U() const { return P.Lg; }
  void horizon_views(HorizonView<const T>* U, HorizonView<const T>* ptau, int* rows) const {
    *U = {P.U, size_t(P.Lg), 1}, *ptau = {P.ptau, size_t(np) * (cfg.dv + 1), 1}, *rows = 1;  // instance-major rows
  }
  int spread_u0(const T* du) {
    replicate_rows_im<T><<<dim3(4, cfg.batch), 256, 0, stream>>>(P.U, P.Lg, du, cfg.batch, nu, cfg.dv, 0);
    HIP_TRY(hipGetLastError());
    return 0;
  }

  // n consecutive ticks in one launch (n > 1 needs the on-device plant: x_next != nullptr)
  int launch_ticks(T* u_out, const T* x_in, T* x_next, int n) {
    P.mode = WG_TICK;
    P.x_in = x_in, P.u_out = u_out, P.x_next = x_next;
    P.n_ticks = n;
    for (int k = 0; k < n; ++k) {
      P.dtau_tab[2 * k] = dtau_of(t + P.h);  // cgmres.hpp:88
      P.dtau_tab[2 * k + 1] = dtau_of(t);    // cgmres.hpp:91
      t = t + P.dt;                          // cgmres.hpp:107
    }
    P.dtau_h = P.dtau_tab[0], P.dtau_0 = P.dtau_tab[1];
    v_by_stage = !plan.k.wave && plan.k.nwt == 1;
    if (plan.k.wave)
      k_tick<<<dim3((cfg.batch + Tr::kWaveWpb - 1) / Tr::kWaveWpb), dim3(64 * Tr::kWaveWpb), plan.lds_bytes_tick, stream>>>(P);
    else
      k_tick<<<grid(), block(), plan.lds_bytes_tick, stream>>>(P);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  int launch_tick(T* u_out, const T* x_in, T* x_next) { return launch_ticks(u_out, x_in, x_next, 1); }
  // all four members are set together or not at all: a failure half-way leaves no buffer behind
  int alloc_pinned(size_t bx, size_t bu) {
    void *hx = nullptr, *hu = nullptr, *dx = nullptr, *du = nullptr;
    hipError_t e = hipHostMalloc(&hx, bx, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostMalloc(&hu, bu, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dx, hx, 0);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&du, hu, 0);
    if (e != hipSuccess) {
      if (hx) (void)hipHostFree(hx);
      if (hu) (void)hipHostFree(hu);
      return fail(e == hipErrorOutOfMemory ? CGMRES_HIP_ENOMEM : CGMRES_HIP_ERUNTIME, "control: pinned buffers: %s", hipGetErrorString(e));
    }
    pin_x = static_cast<T*>(hx), pin_u = static_cast<T*>(hu), pin_x_dev = static_cast<T*>(dx), pin_u_dev = static_cast<T*>(du);
    return 0;
  }
  int control_host(void* u, const void* x) override {
    if (cfg.batch > kPinnedIoMaxBatch) return Host::control_host(u, x);  // the staged path
    const size_t bx = size_t(cfg.batch) * nx * sizeof(T), bu = size_t(cfg.batch) * nu * sizeof(T);
    if (!pin_x)
      if (int rc = alloc_pinned(bx, bu)) return rc;
    std::memcpy(pin_x, x, bx);
    if (int rc = launch_tick(pin_u_dev, pin_x_dev, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    std::memcpy(u, pin_u, bu);
    return 0;
  }
  int closed_loop(void* x, void* u, int n_ticks, const LoopSeqs& sq) override {
    const int all = np * (cfg.dv + 1);
    // a loop with a preview (LoopSeqs::preview_fill): the sequence is the ring of this context, one row per instance and
    // tick of a launch, filled in front of every launch; row i of the loop is row i - (the launch's first tick) of the ring
    const bool pv = sq.preview_fill != nullptr && all && n_ticks > 0;
    const int per_instance = pv ? 1 : sq.ptau_per_instance;
    const size_t per_tick = size_t(per_instance ? cfg.batch : 1) * all;
    if (pv)
      if (int rc = grow(&this->pv_ring, &this->pv_ring_n, size_t(CGM_FUSE_MAX) * per_tick)) return rc;
    const T* seq = pv ? Host::pv_ring : all ? static_cast<const T*>(sq.ptau) : nullptr;
    int first = 0;  // the first tick of the launch the ring holds
    auto row = [&](int i) { return seq + size_t(pv ? i - first : i) * per_tick; };
    P.pseq_tick = per_tick, P.pseq_inst = per_instance ? all : 0;
    // plant inputs (cgmres_hip_closed_loop_device_ex): d and v, [n_ticks][batch or 1][nx]
    PlantSeqs<T> ps{static_cast<const T*>(sq.dist), static_cast<const T*>(sq.meas),
                    size_t(sq.dist_per_instance ? cfg.batch : 1) * nx, size_t(sq.meas_per_instance ? cfg.batch : 1) * nx,
                    sq.dist_per_instance ? nx : 0, sq.meas_per_instance ? nx : 0};
    // a loop with a plant of its own (LoopSeqs::plant_step): one tick per launch, no plant step in the tick kernel and no
    // PlantSeqs record; the controller is shown y = x + v, which the plant kernel leaves in plant_y
    const bool own_plant = sq.plant_step != nullptr;
    const bool plant_in = !own_plant && (ps.dist || ps.meas);
    const T* x_seen = static_cast<const T*>(x);
    if (own_plant && ps.meas && n_ticks > 0) {
      if (int rc = grow(&this->plant_y, &this->plant_y_n, size_t(cfg.batch) * nx)) return rc;
      x_seen = Host::plant_y;
    }
    // stage 0 of the horizon tick i is given: row i of the sequence, or the handle's ptau
    auto p_of = [&](int i) {
      return seq ? HorizonView<const T>{row(i), size_t(per_instance ? all : 0), 1}
                 : HorizonView<const T>{P.ptau, size_t(all), 1};
    };
    // (a lambda, so that a failed launch check leaves through the line below it, which takes the per-launch pointers off
    // the handle: a later control() must not meet a stale sequence or PlantSeqs record)
    auto launches = [&]() -> int {
      // the launch sizes: today's cut, or with a record the cut of record_plan.hip.h (every recorded tick ends a launch)
      RecordCut cut(n_ticks, sq.rec_take ? sq.rec_stride : 0, own_plant ? 1 : CGM_FUSE_MAX);
      if (own_plant && x_seen != x)
        if (int rp = Host::plant_tick(sq, -1, n_ticks, x, u, p_of(0))) return rp;
      while (!cut.done()) {
        const int i = cut.i;
        bool rec = false;
        const int n = cut.next(&rec);
        if (pv) {
          first = i;
          if (int rv = Host::preview_rows(sq, n)) return rv;
        }
        P.ptau_seq = seq ? row(i) : nullptr;  // the kernel reloads ptau at the top of every tick
        if (plant_in) {  // this launch's rows, through the device-resident record the kernel reads (stream-ordered)
          PlantSeqs<T> q = ps;
          q.dist = ps.dist ? ps.dist + size_t(i) * ps.dist_tick : nullptr;
          q.meas = ps.meas ? ps.meas + size_t(i) * ps.meas_tick : nullptr;
          set_plant_seqs_kernel<T><<<1, 1, 0, stream>>>(pin_dev, q);
          HIP_TRY(hipGetLastError());
          P.pin = pin_dev;
        }
        if (plan.binning && have_counts) {
          bin_by_count_kernel<0><<<1, 1024, 0, stream>>>(perm_dev, P.n_ax, cfg.batch, cfg.k_max);
          HIP_TRY(hipGetLastError());
          P.perm = perm_dev;
        }
        T t_last = t;  // the time of the launch's last control(), by the statements of launch_ticks
        for (int k = 1; k < n; ++k) t_last = t_last + P.dt;
        const int rc = launch_ticks(static_cast<T*>(u), x_seen, own_plant ? nullptr : static_cast<T*>(x), n);
        P.perm = nullptr;
        have_counts = true;
        if (rc) return rc;
        if (own_plant)
          if (int rp = Host::plant_tick(sq, i, n_ticks, x, u, p_of(i))) return rp;
        if (rec)
          if (int rr = Host::record(sq, cut.i / sq.rec_stride - 1, x, u, t_last)) return rr;
      }
      return 0;
    };
    const int rc = launches();
    P.ptau_seq = nullptr, P.pin = nullptr, P.perm = nullptr;  // control() and the hooks take none of them
    if (!rc && seq && n_ticks > 0) {  // the handle keeps the last tick's ptau, as set_ptau would (cgmres.hpp:36-39)
      replicate_rows_im<T><<<dim3(4, cfg.batch), 256, 0, stream>>>(P.ptau, all, row(n_ticks - 1),
                                                                    cfg.batch, all, 1, !per_instance);
      HIP_TRY(hipGetLastError());
    }
    return rc;
  }

  int get_state(double* tt, void* U, void* dUdt) override {
    if (tt) *tt = double(t);
    if (int rc = rows_d2h(U, P.U, P.Lg, L, cfg.batch)) return rc;
    return rows_d2h(dUdt, P.dUdt, P.Lg, L, cfg.batch);
  }
  int set_state(double tt, const void* U, const void* dUdt) override {
    t = T(tt);
    if (U)
      if (int rc = rows_h2d(P.U, P.Lg, U, L)) return rc;
    if (dUdt)
      if (int rc = rows_h2d(P.dUdt, P.Lg, dUdt, L)) return rc;
    return 0;
  }
  int state_rows(void** U, void** dUdt, int32_t* pitch) override {
    *U = P.U, *dUdt = P.dUdt, *pitch = P.Lg;
    return 0;
  }
  int get_krylov(void* V, void* H, void* rho, void* g) override {
    const int k1 = cfg.k_max + 1;
    if (V) {  // rows are pair-interleaved on the device (WgCtx::load_vec): element r + 16 m sits at (m/2)*32 + 2r + (m&1);
              // rows written by the row-parallel Newton kernel: element 12 r + i at (i/2)*32 + 2r + (i&1) (StageOwn)
      const size_t rows = size_t(cfg.batch) * k1;
      std::vector<T> tmp(rows * P.Lv);
      HIP_TRY(hipMemcpyAsync(tmp.data(), P.V, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      T* dst = static_cast<T*>(V);
      for (size_t q = 0; q < rows; ++q)
        for (int e = 0; e < L; ++e) {
          const int rr = e & 15, m = e >> 4;
          const int pos = v_by_stage ? StageOwn::hbm_pos_of_elem(e) : (m >> 1) * 32 + 2 * rr + (m & 1);
          dst[q * L + e] = tmp[q * P.Lv + pos];
        }
    }
    if (H)
      if (int rc = rows_d2h(H, P.kry, ks_all, k1 * k1, cfg.batch)) return rc;
    if (rho)
      if (int rc = rows_d2h(rho, P.kry + k1 * k1, ks_all, k1, cfg.batch)) return rc;
    if (g)
      if (int rc = rows_d2h(g, P.kry + k1 * k1 + k1, ks_all, 3 * cfg.k_max, cfg.batch)) return rc;
    return 0;
  }

  // ---- white-box hooks: same device functions, selected by P.mode ---------------------------------
  int run_hook(int mode, const void* in0, const void* in1, void* out, const void* x, T dtau) {
    const size_t n = size_t(cfg.batch) * L;
    if (int rc = grow(&stage2, &stage2_n, 3 * n)) return rc;
    T *d0 = stage2, *d1 = stage2 + n, *dout = stage2 + 2 * n;
    if (in0) HIP_TRY(hipMemcpyAsync(d0, in0, n * sizeof(T), hipMemcpyHostToDevice, stream));
    if (in1) HIP_TRY(hipMemcpyAsync(d1, in1, n * sizeof(T), hipMemcpyHostToDevice, stream));
    if (x) HIP_TRY(hipMemcpyAsync(x_dev, x, size_t(cfg.batch) * nx * sizeof(T), hipMemcpyHostToDevice, stream));
    P.mode = mode;
    P.hook_in0 = d0, P.hook_in1 = d1, P.hook_out = out ? dout : nullptr, P.hook_dtau = dtau;
    P.x_in = x ? x_dev : nullptr, P.u_out = nullptr, P.x_next = nullptr;
    P.dtau_h = dtau_of(t + P.h);
    P.dtau_0 = dtau_of(t);
    if (mode == WG_HOOK_GMRES) v_by_stage = false;
    const int keep = P.fh_hbm;
    P.fh_hbm = plan.fh_hbm_hook, P.lds_bytes = int(plan.lds_bytes_hook);  // the hook kernels use the full / fh_hbm plan
    k_hook<<<grid(), block(), plan.lds_bytes_hook, stream>>>(P);
    P.fh_hbm = keep, P.lds_bytes = int(plan.lds_bytes);
    HIP_TRY(hipGetLastError());
    if (out) HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int hook_F(void* ret, const void* U, const void* x, double tt) override {
    return run_hook(WG_HOOK_F, U, nullptr, ret, x, dtau_of(T(tt)));
  }
  int hook_prepare(void* b, const void* x) override {
    return run_hook(WG_HOOK_PREPARE, nullptr, nullptr, b, x, T(0));
  }
  int hook_Ax(void* out, const void* v) override {
    return run_hook(WG_HOOK_AX, v, nullptr, out, nullptr, T(0));
  }
  int hook_gmres(void* x, const void* b) override {
    return run_hook(WG_HOOK_GMRES, x, b, x, nullptr, T(0));
  }
};

}  // namespace cgm
