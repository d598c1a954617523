// The reference's `class Gmres` (include/gmres.hpp) around the convection-diffusion stencil at len = 840: a solve beyond
// one wavefront's LDS for a serial operator at k_max >= 20 and for a row-form operator at k_max >= 21, so the device
// serves it with the one-lane-per-system kernel (gmres_op_kernel).  Source-compatible with the reference's include/
// like gmres_main.cpp; built against it (host solver, -ffp-contract=off) its output IS the fixture
// tests/golden/user_gmres_convdiff840.txt:
//   ./gmres_lane_main        ->  one line per (k_max, instance): i k_max tol | x[0..840) in %.17g   (tol = 0)
//   ./gmres_lane_main hsub   ->  one line per (k_max, instance): i k_max | h(k+1,k), k = 0..k_max-1, of that run
// The second form is what entitles the fixture to a 1e-9 comparison: every sub-diagonal entry far above the rounding
// floor means the Arnoldi process neither broke down nor ran into noise, on any build.
// Scenario of instance i: the one of the other user_gmres_* fixtures (tests/test_user_gmres.py: scenario).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

// Zero-filled heap (the reference reads v_mat / h_mat before writing parts of them) that remembers the latest array
// allocations: the reference's constructor makes five (v_mat, h_mat, rho_e_vec, g_vec, U_buf, in this order) and keeps
// them private; g_vec[3 k + 1] holds h(k+1,k) after a solve (gmres.hpp:82).
static void* g_last[5];
void* operator new[](std::size_t n) {
  void* p = std::calloc(n ? n : 1, 1);
  if (!p) throw std::bad_alloc();
  for (int j = 0; j < 4; ++j) g_last[j] = g_last[j + 1];
  g_last[4] = p;
  return p;
}
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

#include "gmres.hpp"
#include "gmres_row_ops.hpp"

using Op = ConvDiffRowOp840;

class Solver : public Gmres {
 public:
  Solver(uint16_t k_max, double tol, const double* p) : Gmres(Op::len, k_max, tol), p_(p) {
    g_vec_ = static_cast<const double*>(g_last[3]);
  }
  void solve(double* x, const double* b) { gmres(x, b); }
  const double* g_vec_;

 private:
  void Ax_func(double* Ax, const double* x) override { Op::Ax(Ax, x, p_); }
  const double* p_;
};

int main(int argc, char** argv) {
  constexpr int L = Op::len;
  const bool hsub = argc > 1 && !strcmp(argv[1], "hsub");
  const int kmaxs[2] = {20, 21};
  static double x[L], b[L];
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 2; ++i) {
      double p[2] = {0.4 + 0.07 * i, 0.35 - 0.02 * i};
      for (int e = 0; e < L; ++e) b[e] = std::sin(0.3 * e + 0.5 * i) + 0.1 * e, x[e] = 0.01 * (e - i);
      Solver s(kmaxs[c], 0.0, p);
      s.solve(x, b);
      if (hsub) {
        printf("%d %d", i, kmaxs[c]);
        for (int k = 0; k < kmaxs[c]; ++k) printf(" %.17g", s.g_vec_[3 * k + 1]);
      } else {
        printf("%d %d %.17g", i, kmaxs[c], 0.0);
        for (int e = 0; e < L; ++e) printf(" %.17g", x[e]);
      }
      printf("\n");
    }
  return 0;
}
