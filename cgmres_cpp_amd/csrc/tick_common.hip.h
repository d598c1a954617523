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
// The Householder column of gmres.hpp:71-90, the one statement of its arithmetic for every mapping: the callers differ in
// where the words live (LDS with or without look-ahead, lane-selected registers, strided HBM) and in who stores which
// component, never in these expressions or their association.
// :78-83 the reflector that turns (a, c) into (sigma, 0)
template <class T>
struct Reflector {
  T g0, g1, g2, sigma;
};
template <class T>
__device__ __forceinline__ Reflector<T> reflector_make(T a, T c) {
  const T sigma = -(a < T(0.0) ? T(-1.0) : T(1.0)) * sqrt_t<T>(a * a + c * c);
  const T g0 = a - sigma, g1 = c;
  const T g2 = T(2.0) / (g0 * g0 + g1 * g1);
  return {g0, g1, g2, sigma};
}
// :71-77 a stored reflector (g0, g1, g2) applied to the pair (a, c).  The common factor is formed where this is
// constructed, a component where the caller asks for it: one that only the storing lanes need is then computed in their
// branch, where the callers had it when they spelled this out — an instruction's place decides the schedule and the
// register allocation around it, and the kernels are held to the code they had.
template <class T>
struct ReflectorApply {
  T beta, a, c, g0, g1;
  __device__ __forceinline__ ReflectorApply(T g0_, T g1_, T g2, T a_, T c_)
      : beta((g0_ * a_ + g1_ * c_) * g2), a(a_), c(c_), g0(g0_), g1(g1_) {}
  __device__ __forceinline__ T first() const { return a - beta * g0; }
  __device__ __forceinline__ T second() const { return c - beta * g1; }
};
// :86-90 the residual pair under the new reflector, e_k -> (e_k', e_(k+1)), in the same form
template <class T>
struct ResidualRotate {
  T beta, ek, g0, g1;
  __device__ __forceinline__ ResidualRotate(T g0_, T g1_, T g2, T ek_) : beta(g0_ * ek_ * g2), ek(ek_), g0(g0_), g1(g1_) {}
  __device__ __forceinline__ T first() const { return ek - beta * g0; }
  __device__ __forceinline__ T second() const { return -beta * g1; }
};
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
