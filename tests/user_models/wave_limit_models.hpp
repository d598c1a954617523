// Two USER models in the reference's Model concept (<example>/model.hpp:7-76), written for this repository's tests of
// the wave mapping's limits (tests/test_user_model_wave.py): both must be REFUSED by an explicit variant = 4 with
// CGMRES_HIP_EINVAL, never faulted.
//   Chain5Model     five states (dim_x = 5): one above the wave mapping's dim_x limit (csrc/tick_wave.hip.h).
//   NonAffineModel  a dHdx that is NOT affine in the costate (a lmd^2 term): the generated stage split of the wg and
//                   wave mappings does not exist for it (user_affinity_kernel), only the lane mapping serves it.
#pragma once
#include <cmath>
#include <cstdint>

class Chain5Model {
 public:
  static constexpr uint16_t dim_x = 5;
  static constexpr uint16_t dim_u = 1;
  static constexpr uint16_t dim_p = 1;  // (unused)
  static constexpr double dt = 0.001;
  static constexpr double h = 0.002;
  static constexpr double zeta = 1000.0;
  static constexpr uint16_t dv = 50;
  static constexpr double Tf = 0.5;
  static constexpr double alpha = 0.5;
  static constexpr double tol = 1e-6;
  static constexpr uint16_t k_max = 5;

  static void dxdt(double* ret, const double* x, const double* u, const double* p) {
    ret[0] = x[1];
    ret[1] = -x[0] + x[2] - 0.1 * x[1] + u[0];
    ret[2] = x[3];
    ret[3] = x[0] - 2.0 * x[2] + x[4];
    ret[4] = -x[4];
  }
  static void dPhidx(double* ret, const double* x, const double* p) {
    for (int i = 0; i < 5; ++i) ret[i] = x[i];
  }
  static void dHdx(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
    ret[0] = x[0] - lmd[1] + lmd[3];
    ret[1] = x[1] + lmd[0] - 0.1 * lmd[1];
    ret[2] = x[2] + lmd[1] - 2.0 * lmd[3];
    ret[3] = x[3] + lmd[2];
    ret[4] = x[4] + lmd[3] - lmd[4];
  }
  static void dHdu(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
    ret[0] = u[0] + lmd[1];
  }
  static void ddHduu(double* ret, const double* x, const double* u, const double* p, const double* lmd) { ret[0] = 1.0; }
};

class NonAffineModel {
 public:
  static constexpr uint16_t dim_x = 2;
  static constexpr uint16_t dim_u = 1;
  static constexpr uint16_t dim_p = 1;  // (unused)
  static constexpr double dt = 0.001;
  static constexpr double h = 0.002;
  static constexpr double zeta = 1000.0;
  static constexpr uint16_t dv = 20;
  static constexpr double Tf = 0.5;
  static constexpr double alpha = 0.5;
  static constexpr double tol = 1e-6;
  static constexpr uint16_t k_max = 5;

  static void dxdt(double* ret, const double* x, const double* u, const double* p) {
    ret[0] = x[1];
    ret[1] = -x[0] + u[0];
  }
  static void dPhidx(double* ret, const double* x, const double* p) {
    ret[0] = x[0];
    ret[1] = x[1];
  }
  static void dHdx(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
    ret[0] = x[0] - lmd[1] + 0.5 * lmd[0] * lmd[0];
    ret[1] = x[1] + lmd[0];
  }
  static void dHdu(double* ret, const double* x, const double* u, const double* p, const double* lmd) {
    ret[0] = u[0] + lmd[1];
  }
  static void ddHduu(double* ret, const double* x, const double* u, const double* p, const double* lmd) { ret[0] = 1.0; }
};
