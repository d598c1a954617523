// What the host side of the two kernel mappings has in common (ctx_lane.hip.h, ctx_wg.hip.h): the time of the batch,
// the staged host-pointer tick, the solver status, the start-up Newton solve and the argument handling of set_ptau /
// init_u0.  The device and the pointers of a call are checked where it enters the library (capi.hip: ENTER); a
// context selects the device in init_common() and in its destructor only.
//
// D is the mapping's context (CRTP, no new virtual).  It provides
//   P                                       its kernel parameters; both name the status arrays n_ax and reason
//   launch_tick(u_out, x_in, x_next)        one control tick on the stream, advancing t
//   upload(dst, pitch, src, n, reps, per_instance)
//                                           host [B or 1][n] -> the mapping's device layout, every instance's n values
//                                           repeated reps times (0: copied once, no repetition kernel)
//   spread_u0(du)                           device [B][nu] -> P.U, repeated over the horizon
//   pitch_U()                               what upload() takes as the pitch of P.U
//   horizon_views(U, ptau, rows)            strided views of P.U and P.ptau for horizon(); *rows: instance-major rows
#pragma once
#include "ctx_common.hip.h"
#include "horizon.hip.h"
#include "record_plan.hip.h"
#include "util_kernels.hip.h"

namespace cgm {

template <class M, class T, class D>
struct CtxHost : cgmres_hip_ctx {
  T t = T(0);
  T *stage = nullptr, *stage2 = nullptr;  // device staging, grown on demand: upload(), and init_u0_newton / the hooks
  size_t stage_n = 0, stage2_n = 0;
  T *x_dev = nullptr, *u_dev = nullptr;  // [B][nx], [B][nu] staging for the host-pointer entry points
  T* hz = nullptr;                       // scratch of horizon(), grown on demand
  size_t hz_n = 0;

  D& self() { return static_cast<D&>(*this); }

  T dtau_of(T tt) const {  // cgmres.hpp:32-34, evaluated once per tick on the host for the whole batch
    return cgm::dtau_of<T>(cfg, tt);
  }
  double time() const override { return double(t); }

  int set_ptau(const void* p, int per_instance, bool repeat) override {
    if (np == 0) return 0;  // semiactive: ptau is a zero-length array (semiactive_damper/main.cpp:45-47)
    const int all = np * (cfg.dv + 1);
    return repeat ? self().upload(self().P.ptau, all, p, np, cfg.dv + 1, per_instance)
                  : self().upload(self().P.ptau, all, p, all, 0, per_instance);
  }
  int init_u0(const void* u0, int per_instance) override {
    return self().upload(self().P.U, self().pitch_U(), u0, nu, cfg.dv, per_instance);
  }
  int init_u0_newton(void* u0, const void* x0, const void* p0, int n_loop) override {
    const size_t B = cfg.batch;
    if (int rc = grow(&stage2, &stage2_n, B * (nu + nx + np))) return rc;
    T *du = stage2, *dx = du + B * nu, *dp = dx + B * nx;
    HIP_TRY(hipMemcpyAsync(du, u0, B * nu * sizeof(T), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(dx, x0, B * nx * sizeof(T), hipMemcpyHostToDevice, stream));
    if (np) HIP_TRY(hipMemcpyAsync(dp, p0, B * np * sizeof(T), hipMemcpyHostToDevice, stream));
    newton_u0_kernel<M, T><<<dim3((B + 63) / 64), 64, 0, stream>>>(du, dx, dp, cfg.batch, n_loop);
    HIP_TRY(hipGetLastError());
    if (int rc = self().spread_u0(du)) return rc;  // cgmres.hpp:75
    HIP_TRY(hipMemcpyAsync(u0, du, B * nu * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  int control_device(void* u, const void* x, void* x_next) override {
    return self().launch_tick(static_cast<T*>(u), static_cast<const T*>(x), static_cast<T*>(x_next));
  }
  int control_host(void* u, const void* x) override {  // staged: copy in, launch, copy out, synchronise
    HIP_TRY(hipMemcpyAsync(x_dev, x, size_t(cfg.batch) * nx * sizeof(T), hipMemcpyHostToDevice, stream));
    if (int rc = self().launch_tick(u_dev, x_dev, nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(u, u_dev, size_t(cfg.batch) * nu * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  // cgmres_hip_horizon_device (horizon.hip.h): F_func(ret, U, x, t) of cgmres.hpp:113-162 with the handle's U, ptau and t,
  // keeping xtau, ltau, F and ||F||; on the stream, no copy, no synchronise.  Not a virtual: the translation unit or plugin
  // that made the context calls it on the concrete type (factory_impl.hip.h: horizon_variant).  Outputs the caller does
  // not take and the costate sweep needs go to the scratch `hz`: element-major [n][ldh], like the lane mapping's arrays.
  int horizon(const void* x, const cgmres_hip_horizon_out* o) {
    constexpr HorizonPlan pl = horizon_plan_of<M, T>();
    if (!pl.fits)
      return fail(CGMRES_HIP_EINVAL, "horizon_device: one stage of this model (dim_x %d, dim_u %d, dim_p %d) exceeds the kernel's LDS",
                  nx, nu, np);
    const size_t ldh = size_t(cfg.batch + kHorizonLanes - 1) / kHorizonLanes * kHorizonLanes;
    const size_t n_x = size_t(nx) * (cfg.dv + 1), n_t = size_t(M::NC) * cfg.dv, n_F = size_t(L);
    const bool back = o->ltau_dev || o->F_dev || o->fnorm_dev;
    const bool own_x = !o->xtau_dev, own_t = back && n_t, own_F = o->fnorm_dev && !o->F_dev;
    if (int rc = grow(&hz, &hz_n, ((own_x ? n_x : 0) + (own_t ? n_t : 0) + (own_F ? n_F : 0)) * ldh)) return rc;
    HorizonParams<T> H{};
    H.B = cfg.batch, H.dv = cfg.dv, H.back = back;
    H.dtau = dtau_of(t);  // cgmres.hpp:127
    H.x = static_cast<const T*>(x);
    int rows = 0;  // U and ptau are instance-major rows: the chunk loads run along the rows
    self().horizon_views(&H.U, &H.ptau, &rows);
    T* s = hz;
    H.xtau = own_x ? HorizonView<T>{s, 1, ldh} : HorizonView<T>{static_cast<T*>(o->xtau_dev), n_x, 1};
    if (own_x) s += n_x * ldh;
    H.trig = own_t ? HorizonView<T>{s, 1, ldh} : HorizonView<T>{nullptr, 0, 0};
    if (own_t) s += n_t * ldh;
    H.F = own_F ? HorizonView<T>{s, 1, ldh} : HorizonView<T>{static_cast<T*>(o->F_dev), n_F, 1};
    H.ltau = static_cast<T*>(o->ltau_dev), H.fnorm = static_cast<T*>(o->fnorm_dev);
    const dim3 grid(unsigned(ldh / kHorizonLanes));
    if (rows)
      horizon_kernel<M, T, true><<<grid, kHorizonLanes, 0, stream>>>(H);
    else
      horizon_kernel<M, T, false><<<grid, kHorizonLanes, 0, stream>>>(H);
    HIP_TRY(hipGetLastError());
    return 0;
  }

  int get_status(int32_t* n_ax, int32_t* reason) override {
    if (n_ax) HIP_TRY(hipMemcpyAsync(n_ax, self().P.n_ax, size_t(cfg.batch) * 4, hipMemcpyDeviceToHost, stream));
    if (reason) HIP_TRY(hipMemcpyAsync(reason, self().P.reason, size_t(cfg.batch) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int status_dev(const int32_t** n_ax, const int32_t** reason) override {
    *n_ax = self().P.n_ax, *reason = self().P.reason;
    return 0;
  }
  // Record j of a recorded closed loop, on the stream behind the launch that ended its stride window.  x, u, n_ax and
  // reason are in caller order and instance-major in every mapping, so the record has no per-mapping code.
  int record(const LoopSeqs& sq, int j, const void* x, const void* u, T t_tick) {
    return sq.rec_take(sq.rec, this, j, x, u, self().P.n_ax, self().P.reason, double(t_tick));
  }
  // The plant of a loop that brings its own (LoopSeqs::plant_step), on the stream behind the launch of tick k of n_ticks:
  // x <- Phi(x, u) + d_k and, while a tick follows, y <- x + v_{k+1}.  p: stage 0 of the horizon tick k was given, in
  // the mapping's layout.  k = -1: no step, the first tick's measurement y <- x + v_0.
  T* plant_y = nullptr;  // [B][nx], grown on demand: what the controller is shown when v is given
  size_t plant_y_n = 0;
  int plant_tick(const LoopSeqs& sq, int k, int n_ticks, void* x, const void* u, HorizonView<const T> p) {
    const T *dseq = static_cast<const T*>(sq.dist), *mseq = static_cast<const T*>(sq.meas);
    const size_t d_tick = size_t(sq.dist_per_instance ? cfg.batch : 1) * nx, m_tick = size_t(sq.meas_per_instance ? cfg.batch : 1) * nx;
    PlantCall c;
    c.x = x, c.u = u;
    c.theta = sq.plant_theta, c.theta_inst = sq.plant_theta_inst;
    c.p = p.p, c.p_inst = p.sb, c.p_elem = p.se;
    c.integrator = sq.plant_integrator, c.substeps = k < 0 ? 0 : sq.plant_substeps;
    if (k >= 0 && dseq) c.d = dseq + size_t(k) * d_tick, c.d_inst = sq.dist_per_instance ? nx : 0;
    if (mseq && k + 1 < n_ticks) c.v = mseq + size_t(k + 1) * m_tick, c.v_inst = sq.meas_per_instance ? nx : 0, c.y = plant_y;
    return sq.plant_step(this, c);
  }
  // The rows of a loop with a preview (LoopSeqs::preview_fill): a ring of the mapping's ticks per launch, grown on demand,
  // rewritten in front of every launch on the stream (so behind the launch that read it last) and freed with the handle.
  T* pv_ring = nullptr;  // [ticks per launch][B][np * (dv+1)], caller layout
  size_t pv_ring_n = 0;
  // fills the ring's first n rows for the n ticks from the handle's time on
  int preview_rows(const LoopSeqs& sq, int n) {
    T tab[2 * CGMRES_HIP_TICKS_PER_LAUNCH];
    tick_clock<T>(cfg, t, n, tab);
    PreviewCall c;
    c.s = &sq.preview, c.rows = pv_ring, c.n = n, c.tab = tab;
    return sq.preview_fill(this, c);
  }
};

}  // namespace cgm
