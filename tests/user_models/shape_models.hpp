// A FAMILY of user models in the reference's Model concept (<example>/model.hpp:7-76), written for this repository's
// tests: one class template over (dim_x, dim_u, dim_p), so that the kernels a plugin carries can be held to the oracle
// at the shapes where their code takes another path (tests/user_kernel_classes.py has the list and the reasons).
//
//   x_i' = -a_i x_i + c_i x_n - b_i x_i^2 x_n + sum_j B_ij u_j + d_i p[i mod dim_p]        n = (i + 1) mod dim_x
//   L    = 1/2 sum_i q_i (x_i - w_i p[i mod dim_p])^2 + 1/2 sum_j r_j u_j^2 + e/2 (sum_j u_j)^2
//   Phi  = 1/2 sum_i s_i (x_i - w_i p[i mod dim_p])^2
//
// (the terms with p drop out for dim_p = 0).  The state equation is nonlinear in x, so the Jacobian differs from stage
// to stage; B is dense, so every component of dH/du depends on the costate; dxdt and the cost both read p; dHdx and
// dHdu are affine in the costate, as for every H = L + lambda^T f.  Every constant is a closed formula of its indices.
// No input constraint: ddHduu = diag(r) + e is constant and positive definite.
// L and Phi are not part of the Model concept (the plugin glue ignores them): tests/user_models/shape_deriv_check.cpp
// differences them to check the hand-written derivatives below.
#pragma once
#include <cmath>
#include <cstdint>

template <int NX, int NU, int NP>
class ShapeModel {
 public:
  static constexpr uint16_t dim_x = NX;
  static constexpr uint16_t dim_u = NU;
  static constexpr uint16_t dim_p = NP;
  static constexpr double dt = 0.001;
  static constexpr double h = 0.002;
  static constexpr double zeta = 1000.0;
  static constexpr uint16_t dv = 30;
  static constexpr double Tf = 0.5;
  static constexpr double alpha = 0.5;
  static constexpr double tol = 1e-6;
  static constexpr uint16_t k_max = 5;

  static void dxdt(double* ret, const double* x, const double* u, const double* p) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int n = (i + 1) % NX;
      double f = -a(i) * x[i] + c(i) * x[n] - b(i) * x[i] * x[i] * x[n];
#pragma unroll
      for (int j = 0; j < NU; ++j) f += B(i, j) * u[j];
      if constexpr (NP > 0) f += d(i) * p[i % NP];
      ret[i] = f;
    }
  }
  static void dPhidx(double* ret, const double* x, const double* p) {
#pragma unroll
    for (int i = 0; i < NX; ++i) ret[i] = s(i) * (x[i] - xref(i, p));
  }
  static void dHdx(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
#pragma unroll
    for (int i = 0; i < NX; ++i) ret[i] = q(i) * (x[i] - xref(i, p));
#pragma unroll
    for (int i = 0; i < NX; ++i) {  // row i of the state equation: its derivatives by x_i and by x_n (n = i for dim_x = 1)
      const int n = (i + 1) % NX;
      ret[i] += lmd[i] * (-a(i) - 2.0 * b(i) * x[i] * x[n]);
      ret[n] += lmd[i] * (c(i) - b(i) * x[i] * x[i]);
    }
  }
  static void dHdu(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
    double su = 0.0;
#pragma unroll
    for (int j = 0; j < NU; ++j) su += u[j];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      double g = r(j) * u[j] + e() * su;
#pragma unroll
      for (int i = 0; i < NX; ++i) g += lmd[i] * B(i, j);
      ret[j] = g;
    }
  }
  // column-major dim_u x dim_u (symmetric)
  static void ddHduu(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
#pragma unroll
    for (int k = 0; k < NU; ++k)
#pragma unroll
      for (int j = 0; j < NU; ++j) ret[NU * k + j] = e() + (j == k ? r(j) : 0.0);
  }

  // stage cost and terminal cost
  static double L(const double* x, const double* u, const double* p) {
    double v = 0.0, su = 0.0;
    for (int i = 0; i < NX; ++i) v += 0.5 * q(i) * (x[i] - xref(i, p)) * (x[i] - xref(i, p));
    for (int j = 0; j < NU; ++j) v += 0.5 * r(j) * u[j] * u[j], su += u[j];
    return v + 0.5 * e() * su * su;
  }
  static double Phi(const double* x, const double* p) {
    double v = 0.0;
    for (int i = 0; i < NX; ++i) v += 0.5 * s(i) * (x[i] - xref(i, p)) * (x[i] - xref(i, p));
    return v;
  }

 private:
  static constexpr double a(int i) { return 0.5 + 0.1 * i; }
  static constexpr double b(int i) { return 0.3 + 0.05 * i; }
  static constexpr double c(int i) { return 0.8 - 0.15 * i; }
  static constexpr double d(int i) { return 0.2 + 0.1 * i; }
  static constexpr double B(int i, int j) { return ((i + j) % 2 ? -1.0 : 1.0) * (0.3 + 0.1 * ((2 * i + 3 * j) % 5)); }
  static constexpr double q(int i) { return 1.0 + 0.5 * i; }
  static constexpr double s(int i) { return 2.0 + 0.3 * i; }
  static constexpr double r(int j) { return 0.5 + 0.1 * j; }
  static constexpr double w(int i) { return 1.0 - 0.2 * i; }
  static constexpr double e() { return 0.05; }
  static constexpr double xref(int i, const double* p) {
    if constexpr (NP > 0) return w(i) * p[i % NP];
    return 0.0;
  }
};
using Shape110 = ShapeModel<1, 1, 0>;
using Shape321 = ShapeModel<3, 2, 1>;
using Shape262 = ShapeModel<2, 6, 2>;
using Shape431 = ShapeModel<4, 3, 1>;
using Shape521 = ShapeModel<5, 2, 1>;
