// TEST INFRASTRUCTURE: the oracle's generic controller (oracle/cgmres_oracle.hpp, pinned against the reference for the
// shipped models) instantiated for a user model header, closed loop with the model's own state equation as the plant.
//   g++ -O2 -std=c++17 -ffp-contract=off -I<repo> -DMODEL_HEADER='"tests/user_models/chain4_model.hpp"' -DMODEL_CLASS=Chain4Model
//       tests/user_models/user_oracle.cpp -o user_oracle && ./user_oracle B ticks dv k_max tol
// Scenario of instance b (deterministic, no RNG): x_i = 0.3 + 0.05 b - 0.11 i, p_j = 0.2 + 0.03 b + 0.01 j, u0 = 0.1.
// Prints one line per tick: b t k u[0..NU) x[0..NX) in %.17g; with a sixth argument "state" the line continues with the
// controller state the tick STARTED from — t, U[0..L), dUdt[0..L) — for teacher-forced comparisons.
// Sixth argument "full": the "state" line continues with the exit reason and the controller state AFTER the tick —
// t', U'[0..L), dUdt'[0..L).  A seventh argument then names a file holding the "full" output of another build of this
// program for the same B, ticks and sizes: every tick is TEACHER-FORCED from that file's t, U, dUdt and x (the contracted
// build stepped from the plain build's states, tools/user_case_admission.py).
// Sixth argument "hooks" (ticks is ignored): per instance, after the Newton start, one control() and the plant step,
//   b 0 L, then four lines of L values: F(U, x, t) | the right-hand side b the next tick would solve |
//   Ax(v) for v_i = sin(0.7 i + b) | v;   then a line  t U[0..L) dUdt[0..L) x[0..NX)  — the state the four were taken at.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "oracle/cgmres_oracle.hpp"
#include MODEL_HEADER

struct M : MODEL_CLASS {
  static constexpr oracle::Tuning tuning() { return {dt, h, zeta, Tf, alpha}; }
};

static void print_vec(const std::vector<double>& v, const char* end = "") {
  for (double a : v) printf(" %.17g", a);
  printf("%s", end);
}

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 4, ticks = argc > 2 ? atoi(argv[2]) : 20;
  const int dv = argc > 3 ? atoi(argv[3]) : M::dv, kmax = argc > 4 ? atoi(argv[4]) : M::k_max;
  const double tol = argc > 5 ? atof(argv[5]) : M::tol;
  const bool with_state = argc > 6;
  const bool full = argc > 6 && !strcmp(argv[6], "full"), hooks = argc > 6 && !strcmp(argv[6], "hooks");
  FILE* forced = full && argc > 7 ? fopen(argv[7], "r") : nullptr;
  if (full && argc > 7 && !forced) return 2;
  constexpr int NX = M::dim_x, NU = M::dim_u, NP = M::dim_p;
  const int L = NU * dv;
  for (int b = 0; b < B; ++b) {
    double x[NX], p[NP > 0 ? NP : 1], u0[NU];
    for (int i = 0; i < NX; ++i) x[i] = 0.3 + 0.05 * b - 0.11 * i;
    for (int j = 0; j < NP; ++j) p[j] = 0.2 + 0.03 * b + 0.01 * j;
    for (int j = 0; j < NU; ++j) u0[j] = 0.1;
    oracle::Controller<M, double> c(dv, kmax, tol);
    c.set_ptau_repeat(p);
    c.init_u0(u0);
    c.init_u0_newton(u0, x, p, 10);
    if (hooks) {
      double u[NU], f[NX];
      c.control(u, x);
      M::dxdt(f, x, u, p);
      for (int i = 0; i < NX; ++i) x[i] = x[i] + f[i] * M::dt;
      const double h = M::h, t = c.t();
      std::vector<double> F0(L), rhs(L), v(L), ax(L);
      c.F(F0.data(), c.U().data(), x, t);
      // the pre-solve part of control() (oracle/cgmres_oracle.hpp), statement for statement
      std::vector<double>&xh = c.xh(), &Fh = c.Fh();
      M::dxdt(xh.data(), x, &c.U()[0], &c.ptau()[0]);
      for (int i = 0; i < NX; ++i) xh[i] = xh[i] * h;
      for (int i = 0; i < NX; ++i) xh[i] = xh[i] + x[i];
      c.F(Fh.data(), c.U().data(), xh.data(), t + h);
      c.F(rhs.data(), c.U().data(), x, t);
      const double cc = 1 - M::zeta * h, inv_h = 1.0 / h;
      for (int i = 0; i < L; ++i) rhs[i] = rhs[i] * cc;
      for (int i = 0; i < L; ++i) rhs[i] = rhs[i] - Fh[i];
      for (int i = 0; i < L; ++i) rhs[i] = rhs[i] * inv_h;
      for (int i = 0; i < L; ++i) v[i] = std::sin(0.7 * i + b);
      c.Ax(ax.data(), v.data());
      printf("%d 0 %d\n", b, L);
      print_vec(F0, "\n"), print_vec(rhs, "\n"), print_vec(ax, "\n"), print_vec(v, "\n");
      printf(" %.17g", t);
      print_vec(c.U()), print_vec(c.dUdt());
      for (int i = 0; i < NX; ++i) printf(" %.17g", x[i]);
      printf("\n");
      continue;
    }
    for (int t = 0; t < ticks; ++t) {
      double u[NU], f[NX];
      if (forced) {  // columns of a "full" line: b t k u x | t U dUdt | ...
        double skip;
        bool ok = true;
        for (int i = 0; i < 3 + NU; ++i) ok = ok && fscanf(forced, "%lf", &skip) == 1;
        for (int i = 0; i < NX; ++i) ok = ok && fscanf(forced, "%lf", &x[i]) == 1;
        ok = ok && fscanf(forced, "%lf", &c.t()) == 1;
        for (int i = 0; i < L; ++i) ok = ok && fscanf(forced, "%lf", &c.U()[i]) == 1;
        for (int i = 0; i < L; ++i) ok = ok && fscanf(forced, "%lf", &c.dUdt()[i]) == 1;
        for (int i = 0; i < 2 + 2 * L; ++i) ok = ok && fscanf(forced, "%lf", &skip) == 1;
        if (!ok) return 3;
      }
      const double t_before = c.t();
      const std::vector<double> U_before = c.U(), d_before = c.dUdt();
      c.control(u, x);
      printf("%d %d %d", b, t, c.n_ax());
      for (int j = 0; j < NU; ++j) printf(" %.17g", u[j]);
      for (int i = 0; i < NX; ++i) printf(" %.17g", x[i]);
      if (with_state) {
        printf(" %.17g", t_before);
        for (double v : U_before) printf(" %.17g", v);
        for (double v : d_before) printf(" %.17g", v);
      }
      if (full) {
        printf(" %d %.17g", c.exit_reason(), c.t());
        print_vec(c.U()), print_vec(c.dUdt());
      }
      printf("\n");
      M::dxdt(f, x, u, p);
      for (int i = 0; i < NX; ++i) x[i] = x[i] + f[i] * M::dt;
    }
  }
  if (forced) fclose(forced);
  return 0;
}
