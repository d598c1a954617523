// The plant of a closed loop that is NOT the controller's model stepped by one forward-Euler step
// (cgmres_hip_closed_loop_device_plant, cgmres_hip_plant_step_device): one tick of a plant of its own,
//     x <- Phi(x, u; theta, p) + d        y <- x + v
// Phi = `steps` steps of length hh = dt / steps of forward Euler or classical RK4 on the model's state equation, with u, p
// and theta held over the tick (zero-order hold).  theta replaces the compile-time constants the state equation reads
// (models.hip.h: dxdt_theta, NTHETA values per instance or one broadcast row); absent, a built-in model's own dxdt runs.
// A user model (NTHETA = 0) runs its dxdt(x, u, p) with p = stage 0 of the horizon its controller was given.
//
// A kernel of its own, launched BETWEEN the tick launches on the handle's stream like the record kernels (record.hip.h):
// no tick kernel, parameter struct or kernel argument knows about it.  One lane per instance, caller order, instance-major
// x [B][NX] and u [B][NU]; everything of an instance lives in registers (the arrays are indexed by unrolled constants: no
// scratch), so the substep loop touches no memory.  d, v and y are optional: the null checks are wave-uniform and sit in
// front of the loads.  A lane past the batch returns before its first load.  steps = 0 measures only: y = x + v.
#pragma once
#include <hip/hip_runtime.h>

#include "models.hip.h"
#include "tick_common.hip.h"

namespace cgm {

constexpr int kPlantBlock = 64;  // lanes of a workgroup = instances it covers

template <class T>
struct PlantArgs {
  int B, steps, rk4;
  T hh;  // dt / steps
  T* x;  // [B][NX] in/out
  const T* u;  // [B][NU]
  const T* theta;  // [B or 1][NTHETA], or null = nominal
  int theta_inst;
  const T* p;  // element j of instance b at p[b * p_inst + j * p_elem] (models whose dxdt reads p)
  size_t p_inst, p_elem;
  const T *d, *v;  // [NX] at b * d_inst / b * v_inst, or null
  int d_inst, v_inst;
  T* y;  // [B][NX] or null
};

// the state equation of the plant: the user's dxdt(x, u, p), the parametrised form of a built-in model, or its own dxdt
template <class M, class T, bool THETA>
__device__ __forceinline__ void plant_rhs(T* f, const T* x, const T* u, const T* p, const T* th, const typename M::Math& mc) {
  if constexpr (DxdtUsesP<M, T>::value) {
    M::dxdt_p(f, x, u, p);
  } else if constexpr (THETA) {
    M::dxdt_theta(f, x, u, th, mc);
  } else {
    T tr[M::NC > 0 ? M::NC : 1];
    M::dxdt(f, x, u, tr, mc);
  }
}

template <class M, class T, bool THETA>
__device__ __forceinline__ void plant_integrate(T* x, const T* u, const T* p, const T* th, int steps, bool rk4, T hh,
                                                const typename M::Math& mc) {
  constexpr int NX = M::NX;
  if (rk4) {
    const T half = T(0.5) * hh, sixth = hh / T(6.0);
    for (int s = 0; s < steps; ++s) {
      T k1[NX], k2[NX], k3[NX], k4[NX], xt[NX];
      plant_rhs<M, T, THETA>(k1, x, u, p, th, mc);
#pragma unroll
      for (int c = 0; c < NX; ++c) xt[c] = x[c] + k1[c] * half;
      plant_rhs<M, T, THETA>(k2, xt, u, p, th, mc);
#pragma unroll
      for (int c = 0; c < NX; ++c) xt[c] = x[c] + k2[c] * half;
      plant_rhs<M, T, THETA>(k3, xt, u, p, th, mc);
#pragma unroll
      for (int c = 0; c < NX; ++c) xt[c] = x[c] + k3[c] * hh;
      plant_rhs<M, T, THETA>(k4, xt, u, p, th, mc);
#pragma unroll
      for (int c = 0; c < NX; ++c) x[c] = x[c] + (((k1[c] + T(2.0) * k2[c]) + T(2.0) * k3[c]) + k4[c]) * sixth;
    }
  } else {
    for (int s = 0; s < steps; ++s) {
      T f[NX];
      plant_rhs<M, T, THETA>(f, x, u, p, th, mc);
#pragma unroll
      for (int c = 0; c < NX; ++c) x[c] = x[c] + f[c] * hh;  // the statement of the fused plant block (tick_wg.hip.h)
    }
  }
}

template <class M, class T>
__global__ __launch_bounds__(kPlantBlock) void plant_kernel(PlantArgs<T> A) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
  const int b = blockIdx.x * kPlantBlock + threadIdx.x;
  if (b >= A.B) return;
  T* xb = A.x + size_t(b) * NX;
  T x[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) x[c] = xb[c];
  if (A.steps > 0) {
    T u[NU], p[NP > 0 ? NP : 1];
#pragma unroll
    for (int j = 0; j < NU; ++j) u[j] = A.u[size_t(b) * NU + j];
    if constexpr (DxdtUsesP<M, T>::value) {
#pragma unroll
      for (int j = 0; j < NP; ++j) p[j] = A.p[size_t(b) * A.p_inst + size_t(j) * A.p_elem];
    }
    typename M::Math mc;
    mc.init();
    bool stepped = false;
    if constexpr (M::NTHETA > 0) {
      if (A.theta) {
        T th[M::NTHETA];
#pragma unroll
        for (int j = 0; j < M::NTHETA; ++j) th[j] = A.theta[size_t(b) * A.theta_inst + j];
        plant_integrate<M, T, true>(x, u, p, th, A.steps, A.rk4 != 0, A.hh, mc);
        stepped = true;
      }
    }
    if (!stepped) plant_integrate<M, T, false>(x, u, p, nullptr, A.steps, A.rk4 != 0, A.hh, mc);
    if (A.d) {
      const T* db = A.d + size_t(b) * A.d_inst;
#pragma unroll
      for (int c = 0; c < NX; ++c) x[c] = x[c] + db[c];
    }
#pragma unroll
    for (int c = 0; c < NX; ++c) xb[c] = x[c];
  }
  if (A.y) {
    if (A.v) {
      const T* vb = A.v + size_t(b) * A.v_inst;
#pragma unroll
      for (int c = 0; c < NX; ++c) x[c] = x[c] + vb[c];
    }
#pragma unroll
    for (int c = 0; c < NX; ++c) A.y[size_t(b) * NX + c] = x[c];
  }
}

}  // namespace cgm
