// ROW-form twins of the operators of gmres_ops.hpp (csrc/user_operator.hip.h: `static double Ax_row(int i, ...)` is
// element i of A x, evaluated on all lanes of the wavefront that owns a system).  Every row body is the body of the
// loop of its serial twin, operation for operation (tests/test_user_gmres_row.py checks the two bit for bit on the
// host), so the reference fixtures of the serial operators hold for these as well.
#pragma once

struct SpdTridiagRowOp {  // ONLY the row form
  static constexpr int len = 24, n_params = 1;
  static double Ax_row(int i, const double* x, const double* p) {
    double a = (2.0 + p[0]) * x[i];
    if (i > 0) a = a - x[i - 1];
    if (i + 1 < len) a = a - x[i + 1];
    return a;
  }
};

struct ConvDiffRowOp {  // ONLY the row form
  static constexpr int len = 40, n_params = 2;
  static double Ax_row(int i, const double* x, const double* p) {
    double a = (2.0 + p[0] + 0.01 * i) * x[i];
    if (i > 0) a = a - (1.0 + p[1]) * x[i - 1];
    if (i + 1 < len) a = a - (1.0 - p[1]) * x[i + 1];
    a = a + 0.05 * x[(i * 7 + 3) % len];
    return a;
  }
};

template <int N>
struct ConvDiffRowOpN {  // BOTH forms: the device takes Ax_row, a host subclass's Ax_func calls Ax
  static constexpr int len = N, n_params = 2;
  static double Ax_row(int i, const double* x, const double* p) {
    double a = (2.0 + p[0] + 0.01 * i) * x[i];
    if (i > 0) a = a - (1.0 + p[1]) * x[i - 1];
    if (i + 1 < len) a = a - (1.0 - p[1]) * x[i + 1];
    a = a + 0.05 * x[(i * 7 + 3) % len];
    return a;
  }
  static void Ax(double* Ax, const double* x, const double* p) {
    for (int i = 0; i < len; ++i) Ax[i] = Ax_row(i, x, p);
  }
};
using ConvDiffRowOp150 = ConvDiffRowOpN<150>;
using ConvDiffRowOp300 = ConvDiffRowOpN<300>;
// one element, one element per lane, one lane with two elements; beyond one wave's LDS at k_max >= 21 (20 for a serial operator)
using ConvDiffRowOp1 = ConvDiffRowOpN<1>;
using ConvDiffRowOp64 = ConvDiffRowOpN<64>;
using ConvDiffRowOp65 = ConvDiffRowOpN<65>;
using ConvDiffRowOp840 = ConvDiffRowOpN<840>;

struct NeitherFormOp {  // no product at all: the glue refuses it at compile time
  static constexpr int len = 8, n_params = 0;
};
