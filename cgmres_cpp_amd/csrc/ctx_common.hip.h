// Host-side plumbing shared by the kernel mappings: error reporting, the type-erased controller batch
// behind a cgmres_hip_handle, stream/event ownership and device allocations.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cgmres_hip.h"
#include "models.hip.h"

namespace cgm {

inline thread_local std::string g_err;

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess)                                                                                    \
      return ::cgm::fail(e_ == hipErrorOutOfMemory ? CGMRES_HIP_ENOMEM : CGMRES_HIP_ERUNTIME, "%s: %s (%s:%d)", \
                         #expr, hipGetErrorString(e_), __FILE__, __LINE__);                                  \
  } while (0)

}  // namespace cgm

struct cgmres_hip_ctx;
namespace cgm {
// One launch of plant_kernel (plant.hip.h) on a context's stream: device pointers in the handle's dtype, caller order.
// The context that runs a loop fills p (stage 0 of the horizon its tick was given, in its own layout); a null p is filled
// from the handle's ptau by who knows the context's concrete type (factory_impl.hip.h: plant_variant).
struct PlantCall {
  void* x = nullptr;        // [B][nx] in/out
  const void* u = nullptr;  // [B][nu]
  const void* theta = nullptr;  // [B or 1][n_theta]; null = nominal
  int theta_inst = 0;           // n_theta per instance, 0 for one broadcast row
  const void* p = nullptr;      // element j of instance b at p[b * p_inst + j * p_elem]
  size_t p_inst = 0, p_elem = 0;
  const void* d = nullptr;  // this tick's rows, [nx] at b * d_inst; null = absent
  int d_inst = 0;
  const void* v = nullptr;  // the NEXT tick's rows
  int v_inst = 0;
  void* y = nullptr;     // [B][nx] = x + v; null = not wanted
  int integrator = 0;    // CGMRES_HIP_PLANT_*
  int substeps = 1;      // 0: measure only (y = x + v, x untouched)
};
// The sampled reference signal of a loop with a preview (cgmres_hip_loop_preview, validated by capi.hip) and one launch of
// preview_kernel (preview.hip.h) on a context's stream: rows [n][batch][dim_p*(dv+1)] of the n <= CGMRES_HIP_TICKS_PER_LAUNCH
// ticks whose (t_k, dtau_k) the host array tab [2n] holds, in the handle's dtype.
struct PreviewSig {
  const void* sig = nullptr;  // [batch or 1][n_samples][dim_p], handle dtype
  int per_instance = 0, n_samples = 0, interp = 0;
  double t0 = 0, ts = 1;
};
struct PreviewCall {
  const PreviewSig* s = nullptr;
  void* rows = nullptr;
  int n = 0;
  const void* tab = nullptr;
};
// Per-tick input sequences of the closed loop (cgmres_hip_loop_inputs, validated by capi.hip): device pointers,
// [n_ticks][batch or 1][...]; null = absent
struct LoopSeqs {
  const void* ptau = nullptr;  // set_ptau before every tick (cgmres.hpp:36-39)
  int ptau_per_instance = 0;
  const void* dist = nullptr;  // d: added to the plant step
  int dist_per_instance = 0;
  const void* meas = nullptr;  // v: added to the state the controller is shown
  int meas_per_instance = 0;
  // The record of cgmres_hip_closed_loop_device_rec (record.hip.h): null rec_take = none.  A context cuts its launches by
  // RecordCut(n_ticks, rec_stride, its ticks per launch) and, behind the launch that ends stride window j, calls
  //   rec_take(rec, this, j, x, u, its n_ax, its reason, the handle's time when the window's last control() ran)
  // A pointer, not a name: the function lives in the library, the context of a user model in its plugin.
  int rec_stride = 0;
  int (*rec_take)(void* rec, cgmres_hip_ctx* c, int j, const void* x, const void* u, const int32_t* n_ax,
                  const int32_t* reason, double t) = nullptr;
  void* rec = nullptr;
  // The plant of cgmres_hip_closed_loop_device_plant (plant.hip.h): null plant_step = the fused plant block of the tick
  // kernels.  A context that is given one cuts to one tick per launch, launches the tick without a plant step and calls
  // plant_step behind it.  A pointer like rec_take: for a user model the function lives in its plugin.
  int (*plant_step)(cgmres_hip_ctx* c, const PlantCall& call) = nullptr;
  int plant_integrator = 0, plant_substeps = 1;
  const void* plant_theta = nullptr;
  int plant_theta_inst = 0;
  // The preview of cgmres_hip_closed_loop_device_preview (preview.hip.h): null preview_fill = none.  A context that is given
  // one fills, in front of every launch of its cut, the rows of that launch's ticks in a ring it owns and points the tick
  // kernel's ptau sequence at them.  A pointer like rec_take: the function lives in the library, whatever made the context.
  int (*preview_fill)(cgmres_hip_ctx* c, const PreviewCall& call) = nullptr;
  PreviewSig preview;
};
// The clock of a handle in its dtype T, stated once: dtau(t) (cgmres.hpp:32-34) and, in tick_clock, the (t_k, dtau_k) of
// the n ticks from t on as control() advances it (t += dt, cgmres.hpp:107).  Evaluated on the host for the whole batch.
template <class T>
inline T dtau_of(const cgmres_hip_config& cfg, T tt) {
  return T(cfg.Tf) * (1 - std::exp(-T(cfg.alpha) * tt)) / T(cfg.dv);
}
template <class T>
inline void tick_clock(const cgmres_hip_config& cfg, T t, int n, T* tab) {
  for (int k = 0; k < n; ++k) {
    tab[2 * k] = t, tab[2 * k + 1] = dtau_of(cfg, t);
    t = t + T(cfg.dt);
  }
}
}  // namespace cgm

// Type-erased controller batch: what a cgmres_hip_handle points to.
struct cgmres_hip_ctx {
  cgmres_hip_config cfg{};
  int nx = 0, nu = 0, np = 0, L = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<void*> owned;
  // workgroup partials of the record kernels (record.hip.h), grown on demand by the library, never by a context
  double* rec_scratch = nullptr;
  size_t rec_scratch_n = 0;

  virtual ~cgmres_hip_ctx() {
    (void)hipSetDevice(cfg.device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : owned) (void)hipFree(p);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
  int init_common() {
    HIP_TRY(hipSetDevice(cfg.device));
    if (cfg.stream) {
      stream = static_cast<hipStream_t>(cfg.stream);
    } else {
      HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      own_stream = true;
    }
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    return 0;
  }
  template <class Q>
  int dalloc(Q** p, size_t n) {  // zero-filled, freed with the context
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, (n ? n : 1) * sizeof(Q)));
    HIP_TRY(hipMemsetAsync(q, 0, (n ? n : 1) * sizeof(Q), stream));
    owned.push_back(q);
    *p = static_cast<Q*>(q);
    return 0;
  }
  // staging buffer that only grows; kept in `owned`
  template <class Q>
  int grow(Q** buf, size_t* have, size_t need) {
    if (*have >= need) return 0;
    HIP_TRY(hipStreamSynchronize(stream));
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, need * sizeof(Q)));
    if (*buf) {
      for (auto& o : owned)
        if (o == *buf) o = q;
      HIP_TRY(hipFree(*buf));
    } else {
      owned.push_back(q);
    }
    *buf = static_cast<Q*>(q);
    *have = need;
    return 0;
  }

  virtual const char* variant_name() const = 0;
  virtual int init() = 0;
  virtual int set_ptau(const void*, int per_instance, bool repeat) = 0;
  virtual int init_u0(const void*, int per_instance) = 0;
  virtual int init_u0_newton(void*, const void*, const void*, int) = 0;
  virtual int control_host(void*, const void*) = 0;
  virtual int control_device(void*, const void*, void* x_next) = 0;
  virtual int closed_loop(void* x, void* u, int n_ticks, const cgm::LoopSeqs& seqs) = 0;
  virtual double time() const = 0;
  virtual int get_state(double*, void*, void*) = 0;
  virtual int set_state(double, const void*, const void*) = 0;
  virtual int state_rows(void** U, void** dUdt, int32_t* pitch) {  // mappings without instance-major state rows: none
    *U = nullptr, *dUdt = nullptr, *pitch = 0;
    return 0;
  }
  virtual int get_status(int32_t*, int32_t*) = 0;
  virtual int get_krylov(void*, void*, void*, void*) = 0;
  virtual int hook_F(void*, const void*, const void*, double) = 0;
  virtual int hook_prepare(void*, const void*) = 0;
  virtual int hook_Ax(void*, const void*) = 0;
  virtual int hook_gmres(void*, const void*) = 0;
  // device addresses of what get_status copies: [batch] each, caller order, in every mapping
  virtual int status_dev(const int32_t** n_ax, const int32_t** reason) = 0;
};
