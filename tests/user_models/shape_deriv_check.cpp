// TEST INFRASTRUCTURE: the hand-written derivatives of tests/user_models/shape_models.hpp against central differences of
// the model's own H = L + lambda^T f and Phi, at three fixed points per alias.
//   g++ -O1 -std=c++17 -ffp-contract=off tests/user_models/shape_deriv_check.cpp -o shape_deriv_check && ./shape_deriv_check
// Bound: 1e-7 * max(1, |.|).  With step 1e-5 on functions of order 1 the truncation error is ~1e-10 and the rounding
// error eps/step ~ 1e-11 (second differences for ddHduu difference dHdu, not H, so they carry the same figures).
// Prints one line per alias and quantity (worst error / bound) and returns the number of misses.
#include <cmath>
#include <cstdio>

#include "shape_models.hpp"

namespace {
constexpr double STEP = 1e-5, BOUND = 1e-7;

template <class M>
double H(const double* x, const double* u, const double* p, const double* l) {
  double f[M::dim_x], v = M::L(x, u, p);
  M::dxdt(f, x, u, p);
  for (int i = 0; i < M::dim_x; ++i) v += l[i] * f[i];
  return v;
}

struct Worst {
  double v = 0.0;
  void see(double got, double want) {
    const double e = std::fabs(got - want) / (BOUND * std::fmax(1.0, std::fabs(want)));
    v = (e > v || e != e) ? e : v;
  }
};

template <class M>
int check(const char* name) {
  constexpr int NX = M::dim_x, NU = M::dim_u, NP = M::dim_p;
  Worst wx, wu, wuu, wphi;
  for (int pt = 0; pt < 3; ++pt) {
    double x[NX], u[NU], p[NP > 0 ? NP : 1], l[NX];
    for (int i = 0; i < NX; ++i) x[i] = 0.37 + 0.211 * i - 0.53 * pt, l[i] = -0.45 + 0.31 * i + 0.27 * pt;
    for (int j = 0; j < NU; ++j) u[j] = 0.29 - 0.173 * j + 0.41 * pt;
    for (int j = 0; j < NP; ++j) p[j] = 0.13 + 0.07 * j - 0.05 * pt;
    double hx[NX], hu[NU], huu[NU * NU], phix[NX];
    M::dHdx(hx, x, u, p, l);
    M::dHdu(hu, x, u, p, l);
    M::ddHduu(huu, x, u, p, l);
    M::dPhidx(phix, x, p);
    for (int i = 0; i < NX; ++i) {
      const double x0 = x[i];
      x[i] = x0 + STEP;
      const double hp = H<M>(x, u, p, l), pp = M::Phi(x, p);
      x[i] = x0 - STEP;
      const double hm = H<M>(x, u, p, l), pm = M::Phi(x, p);
      x[i] = x0;
      wx.see(hx[i], (hp - hm) / (2 * STEP));
      wphi.see(phix[i], (pp - pm) / (2 * STEP));
    }
    for (int j = 0; j < NU; ++j) {
      const double u0 = u[j];
      double gp[NU], gm[NU];
      u[j] = u0 + STEP;
      const double hp = H<M>(x, u, p, l);
      M::dHdu(gp, x, u, p, l);
      u[j] = u0 - STEP;
      const double hm = H<M>(x, u, p, l);
      M::dHdu(gm, x, u, p, l);
      u[j] = u0;
      wu.see(hu[j], (hp - hm) / (2 * STEP));
      for (int k = 0; k < NU; ++k) {  // column j of the (column-major) Hessian; symmetric, so the transposed entry too
        wuu.see(huu[NU * j + k], (gp[k] - gm[k]) / (2 * STEP));
        wuu.see(huu[NU * k + j], (gp[k] - gm[k]) / (2 * STEP));
      }
    }
  }
  printf("%s dHdx %.3g dHdu %.3g ddHduu %.3g dPhidx %.3g (worst error / bound)\n", name, wx.v, wu.v, wuu.v, wphi.v);
  return !(wx.v <= 1.0) + !(wu.v <= 1.0) + !(wuu.v <= 1.0) + !(wphi.v <= 1.0);
}
}  // namespace

int main() {
  return check<Shape110>("Shape110") + check<Shape321>("Shape321") + check<Shape262>("Shape262") +
         check<Shape431>("Shape431") + check<Shape521>("Shape521");
}
