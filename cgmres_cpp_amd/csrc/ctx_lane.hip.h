// Host side of the "lane" mapping (tick_lane.hip.h): element-major HBM state, one kernel per tick.
#pragma once
#include "ctx_common.hip.h"
#include "tick_lane.hip.h"
#include "ctx_host.hip.h"

namespace cgm {

template <class M, class T>
struct CtxLane final : CtxHost<M, T, CtxLane<M, T>> {
  using Host = CtxHost<M, T, CtxLane<M, T>>;
  using Host::cfg, Host::nx, Host::nu, Host::np, Host::L, Host::stream, Host::dalloc, Host::grow, Host::init_common;
  using Host::t, Host::dtau_of, Host::stage, Host::stage_n, Host::stage2, Host::stage2_n, Host::x_dev, Host::u_dev;
  TickParams<T> P{};
  int ldb = 0;

  const char* variant_name() const override { return "lane"; }

  int init() override {
    if (int rc = init_common()) return rc;
    cfg.variant = 1;
    nx = M::NX, nu = M::NU, np = M::NP;
    L = nu * cfg.dv;
    ldb = (cfg.batch + 63) / 64 * 64;
    const size_t ld = ldb, k1 = cfg.k_max + 1;
    P.B = cfg.batch, P.ldb = ldb, P.dv = cfg.dv, P.kmax = cfg.k_max, P.L = L;
    P.h = T(cfg.h), P.dt = T(cfg.dt), P.tol = T(cfg.tol);
    P.inv_h = T(1.0) / P.h;
    P.one_m_zh = (1 - T(cfg.zeta) * P.h);
    int rc = 0;
    if ((rc = dalloc(&P.U, L * ld)) || (rc = dalloc(&P.dUdt, L * ld)) || (rc = dalloc(&P.Fh, L * ld)) ||
        (rc = dalloc(&P.bvec, L * ld)) || (rc = dalloc(&P.V, L * k1 * ld)) || (rc = dalloc(&P.H, k1 * k1 * ld)) ||
        (rc = dalloc(&P.g, 3 * cfg.k_max * ld)) || (rc = dalloc(&P.rho, k1 * ld)) || (rc = dalloc(&P.xdxh, nx * ld)) ||
        (rc = dalloc(&P.ptau, size_t(np) * (cfg.dv + 1) * ld)) || (rc = dalloc(&P.traj, size_t(nx) * cfg.dv * ld)) ||
        (rc = dalloc(&P.trig, size_t(M::NC) * cfg.dv * ld)) || (rc = dalloc(&P.n_ax, ld)) ||
        (rc = dalloc(&P.reason, ld)) || (rc = dalloc(&x_dev, size_t(cfg.batch) * nx)) ||
        (rc = dalloc(&u_dev, size_t(cfg.batch) * nu)))
      return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  dim3 lane_grid() const { return dim3((cfg.batch + 63) / 64); }
  // host instance-major [B or 1][n] -> device element-major [n*reps][ldb] (the pitch of every such array is ldb)
  int upload(T* dst, size_t, const void* src, int n, int reps, int per_instance) {
    const size_t cnt = size_t(per_instance ? cfg.batch : 1) * n;
    if (int rc = grow(&stage, &stage_n, cnt)) return rc;
    HIP_TRY(hipMemcpyAsync(stage, src, cnt * sizeof(T), hipMemcpyHostToDevice, stream));
    dim3 grid((cfg.batch + 255) / 256, n * (reps ? reps : 1));
    if (reps)
      replicate_stages<T><<<grid, 256, 0, stream>>>(dst, stage, cfg.batch, ldb, n, reps, !per_instance);
    else
      to_element_major<T><<<grid, 256, 0, stream>>>(dst, stage, cfg.batch, ldb, n, !per_instance);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));  // the host buffer may be reused by the caller right away
    return 0;
  }
  int download(void* dst, const T* src, int n) {
    if (!dst) return 0;
    const size_t cnt = size_t(cfg.batch) * n;
    if (int rc = grow(&stage, &stage_n, cnt)) return rc;
    dim3 grid((cfg.batch + 255) / 256, n);
    to_instance_major<T><<<grid, 256, 0, stream>>>(stage, src, cfg.batch, ldb, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, stage, cnt * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  size_t pitch_U() const { return ldb; }
  void horizon_views(HorizonView<const T>* U, HorizonView<const T>* ptau, int* rows) const {
    *U = {P.U, 1, size_t(ldb)}, *ptau = {P.ptau, 1, size_t(ldb)}, *rows = 0;  // element-major
  }
  int spread_u0(const T* du) {
    dim3 grid((cfg.batch + 255) / 256, nu * cfg.dv);
    replicate_stages<T><<<grid, 256, 0, stream>>>(P.U, du, cfg.batch, ldb, nu, cfg.dv, 0);
    HIP_TRY(hipGetLastError());
    return 0;
  }

  int launch_tick(T* u_out, const T* x_in, T* x_next) {
    P.x_in = x_in, P.u_out = u_out, P.x_next = x_next;
    P.dtau_h = dtau_of(t + P.h);  // cgmres.hpp:88
    P.dtau_0 = dtau_of(t);        // cgmres.hpp:91
    tick_lane_kernel<M, T><<<lane_grid(), 64, 0, stream>>>(P);
    HIP_TRY(hipGetLastError());
    t = t + P.dt;  // cgmres.hpp:107
    return 0;
  }
  int closed_loop(void* x, void* u, int n_ticks, const LoopSeqs& sq) override {
    const int all = np * (cfg.dv + 1), per_instance = sq.ptau_per_instance;
    const size_t per_tick = size_t(per_instance ? cfg.batch : 1) * all;
    // plant inputs (cgmres_hip_closed_loop_device_ex): d and v, [n_ticks][batch or 1][nx]
    const T *dseq = static_cast<const T*>(sq.dist), *mseq = static_cast<const T*>(sq.meas);
    const size_t d_tick = size_t(sq.dist_per_instance ? cfg.batch : 1) * nx, m_tick = size_t(sq.meas_per_instance ? cfg.batch : 1) * nx;
    P.dist_inst = sq.dist_per_instance ? nx : 0, P.meas_inst = sq.meas_per_instance ? nx : 0;
    int rc = 0;
    // a loop with a plant of its own (LoopSeqs::plant_step): no plant step and no d / v in the tick kernel; the controller
    // is shown y = x + v, which the plant kernel leaves in plant_y
    const bool own_plant = sq.plant_step != nullptr;
    const T* x_seen = static_cast<const T*>(x);
    if (own_plant && mseq && n_ticks > 0) {
      if ((rc = grow(&this->plant_y, &this->plant_y_n, size_t(cfg.batch) * nx))) return rc;
      x_seen = Host::plant_y;
    }
    // a loop with a preview (LoopSeqs::preview_fill): a ring of one row, filled in front of every tick and set as a row of
    // a ptau sequence is
    const bool pv = sq.preview_fill != nullptr && all && n_ticks > 0;
    if (pv)
      if ((rc = grow(&this->pv_ring, &this->pv_ring_n, size_t(cfg.batch) * all))) return rc;
    const HorizonView<const T> p0{P.ptau, 1, size_t(ldb)};  // (the handle's ptau holds this tick's horizon: set below)
    RecordCut cut(n_ticks, sq.rec_take ? sq.rec_stride : 0, 1);  // (one tick per launch: the cut only says where a record is due)
    while (!cut.done() && !rc) {
      const int i = cut.i;
      bool rec = false;
      cut.next(&rec);
      const T t_tick = t;
      if (pv) {
        if ((rc = Host::preview_rows(sq, 1))) break;
        dim3 grid((cfg.batch + 255) / 256, all);
        to_element_major<T><<<grid, 256, 0, stream>>>(P.ptau, Host::pv_ring, cfg.batch, ldb, all, 0);
        HIP_TRY(hipGetLastError());
      } else if (sq.ptau && all) {  // set_ptau before this tick (cgmres.hpp:36-39), device to device
        dim3 grid((cfg.batch + 255) / 256, all);
        to_element_major<T><<<grid, 256, 0, stream>>>(P.ptau, static_cast<const T*>(sq.ptau) + i * per_tick, cfg.batch,
                                                       ldb, all, !per_instance);
        HIP_TRY(hipGetLastError());
      }
      if (own_plant) {
        if (i == 0 && x_seen != x) rc = Host::plant_tick(sq, -1, n_ticks, x, u, p0);
        if (!rc) rc = launch_tick(static_cast<T*>(u), x_seen, nullptr);
        if (!rc) rc = Host::plant_tick(sq, i, n_ticks, x, u, p0);
      } else {
        P.dist = dseq ? dseq + size_t(i) * d_tick : nullptr;
        P.meas = mseq ? mseq + size_t(i) * m_tick : nullptr;
        rc = launch_tick(static_cast<T*>(u), static_cast<const T*>(x), static_cast<T*>(x));
      }
      if (!rc && rec) rc = Host::record(sq, cut.i / sq.rec_stride - 1, x, u, t_tick);
    }
    P.dist = nullptr, P.meas = nullptr;  // control() and the hooks take neither
    return rc;
  }

  int get_state(double* tt, void* U, void* dUdt) override {
    if (tt) *tt = double(t);
    if (int rc = download(U, P.U, L)) return rc;
    return download(dUdt, P.dUdt, L);
  }
  int set_state(double tt, const void* U, const void* dUdt) override {
    t = T(tt);
    if (U)
      if (int rc = upload(P.U, ldb, U, L, 0, 1)) return rc;
    if (dUdt)
      if (int rc = upload(P.dUdt, ldb, dUdt, L, 0, 1)) return rc;
    return 0;
  }
  int get_krylov(void* V, void* H, void* rho, void* g) override {
    const int k1 = cfg.k_max + 1;
    int rc;
    if ((rc = download(V, P.V, L * k1)) || (rc = download(H, P.H, k1 * k1)) || (rc = download(rho, P.rho, k1)) ||
        (rc = download(g, P.g, 3 * cfg.k_max)))
      return rc;
    return 0;
  }

  // ---- white-box hooks -------------------------------------------------------------------------
  int hook_F(void* ret, const void* U, const void* x, double tt) override {
    const size_t ld = ldb;
    if (int rc = grow(&stage2, &stage2_n, 2 * size_t(L) * ld)) return rc;
    T *Uem = stage2, *Rem = stage2 + size_t(L) * ld;
    if (int rc = upload(Uem, ldb, U, L, 0, 1)) return rc;
    HIP_TRY(hipMemcpyAsync(x_dev, x, size_t(cfg.batch) * nx * sizeof(T), hipMemcpyHostToDevice, stream));
    P.x_in = x_dev;
    hook_F_kernel<M, T><<<lane_grid(), 64, 0, stream>>>(P, Uem, Rem, dtau_of(T(tt)));
    HIP_TRY(hipGetLastError());
    return download(ret, Rem, L);
  }
  int hook_prepare(void* b, const void* x) override {
    HIP_TRY(hipMemcpyAsync(x_dev, x, size_t(cfg.batch) * nx * sizeof(T), hipMemcpyHostToDevice, stream));
    P.x_in = x_dev;
    P.dtau_h = dtau_of(t + P.h);
    P.dtau_0 = dtau_of(t);
    hook_prepare_kernel<M, T><<<lane_grid(), 64, 0, stream>>>(P);
    HIP_TRY(hipGetLastError());
    return download(b, P.bvec, L);
  }
  int hook_Ax(void* out, const void* v) override {
    const size_t ld = ldb;
    if (int rc = grow(&stage2, &stage2_n, 2 * size_t(L) * ld)) return rc;
    T *Vem = stage2, *Oem = stage2 + size_t(L) * ld;
    if (int rc = upload(Vem, ldb, v, L, 0, 1)) return rc;
    P.dtau_h = dtau_of(t + P.h);
    hook_Ax_kernel<M, T><<<lane_grid(), 64, 0, stream>>>(P, Vem, Oem);
    HIP_TRY(hipGetLastError());
    return download(out, Oem, L);
  }
  int hook_gmres(void* x, const void* b) override {
    const size_t ld = ldb;
    if (int rc = grow(&stage2, &stage2_n, 2 * size_t(L) * ld)) return rc;
    T *Xem = stage2, *Bem = stage2 + size_t(L) * ld;
    if (int rc = upload(Xem, ldb, x, L, 0, 1)) return rc;
    if (int rc = upload(Bem, ldb, b, L, 0, 1)) return rc;
    P.dtau_h = dtau_of(t + P.h);
    hook_gmres_kernel<M, T><<<lane_grid(), 64, 0, stream>>>(P, Xem, Bem);
    HIP_TRY(hipGetLastError());
    return download(x, Xem, L);
  }
};

}  // namespace cgm
