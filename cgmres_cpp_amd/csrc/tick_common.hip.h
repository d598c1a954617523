// What the tick kernels of every mapping (lane, wg, wave) and the operator kernels share and no kernel owns: the output
// modes of the optimality residual, the trait of a state equation that reads p, and scalar helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace cgm {

// Optimality residual F(U [+ h v], x, t) — cgmres.hpp:113-162 (+ :168-174 when PERTURB / F_AX).
//   F_PLAIN: out = F                                   (cgmres.hpp:88)
//   F_RHS  : out = (F*(1-zeta*h) - Fh) * (1/h)         (cgmres.hpp:91-96)
//   F_AX   : out = (F - Fh) * (1/h)                    (cgmres.hpp:173-174)
enum FOut { F_PLAIN = 0, F_RHS = 1, F_AX = 2 };

// Does the state equation read p?  The built-in models do not read the time-varying parameter p in dxdt; a
// user model compiled through the plugin path (user_model.hip.h) may (Model::dxdt(ret, x, u, p), */model.hpp:36).
template <class M, class T, class = void>
struct DxdtUsesP : std::false_type {};
template <class M, class T>
struct DxdtUsesP<M, T, std::enable_if_t<M::DXDT_USES_P>> : std::true_type {};

template <class T>
__device__ __forceinline__ T sqrt_t(T a);
template <>
__device__ __forceinline__ double sqrt_t<double>(double a) {
  return ::sqrt(a);
}
template <>
__device__ __forceinline__ float sqrt_t<float>(float a) {
  return ::sqrtf(a);
}
// neither NaN nor +-Inf (one v_cmp_class on the hardware)
__device__ __forceinline__ bool finite_t(double a) { return __builtin_isfinite(a); }
__device__ __forceinline__ bool finite_t(float a) { return __builtin_isfinite(a); }
template <class T>
__device__ __forceinline__ T quiet_nan();
template <>
__device__ __forceinline__ double quiet_nan<double>() { return __builtin_nan(""); }
template <>
__device__ __forceinline__ float quiet_nan<float>() { return __builtin_nanf(""); }

}  // namespace cgm
