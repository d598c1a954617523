// CgmresBatch::closed_loop_device(x, u, n, cgmres_hip_loop_inputs) against the direct C call on a second batch:
// prints the largest difference over x and u (tests/test_gpu_loop_inputs.py expects 0).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../examples/models.hpp"
#include "cgmres_batch.hpp"

using M = examples::PendulumModel<50, 10>;
constexpr int B = 20, N = 12;

static double* to_dev(cgmres_hip_handle h, const std::vector<double>& v) {
  void* d = nullptr;
  cgmres_detail::check(cgmres_hip_malloc(h, &d, sizeof(double) * v.size()), "malloc");
  cgmres_detail::check(cgmres_hip_memcpy_h2d(h, d, v.data(), sizeof(double) * v.size()), "h2d");
  return static_cast<double*>(d);
}

int main() {
  std::vector<double> x0(B * 4), u0(B * 3), p(B * 2), d(N * B * 4), v(N * B * 4), out[2];
  for (int b = 0; b < B; ++b) {
    const double x[4] = {3.1 + 0.01 * b, 3.2 - 0.01 * b, 0.02, -0.01}, u[3] = {0.0, 3.0, 0.01};
    for (int c = 0; c < 4; ++c) x0[4 * b + c] = x[c];
    for (int j = 0; j < 3; ++j) u0[3 * b + j] = u[j];
    p[2 * b] = 0.7 + 0.01 * b, p[2 * b + 1] = 0.0;
  }
  for (size_t i = 0; i < d.size(); ++i) d[i] = 1e-3 * std::sin(0.37 * i), v[i] = 1e-3 * std::cos(0.23 * i);
  for (int direct = 0; direct < 2; ++direct) {
    CgmresBatch<M> c(B);
    std::vector<double> u(u0);
    c.set_ptau_repeat(p.data());
    c.init_u0(u.data());
    c.init_u0_newton(u.data(), x0.data(), p.data(), 10);
    cgmres_hip_handle h = c.native_handle();
    double *xd = to_dev(h, x0), *ud = to_dev(h, u0), *dd = to_dev(h, d), *vd = to_dev(h, v);
    const cgmres_hip_loop_inputs in = {int32_t(sizeof(cgmres_hip_loop_inputs)), 1, 1, 1, nullptr, dd, vd};
    if (direct)
      cgmres_detail::check(cgmres_hip_closed_loop_device_ex(h, xd, ud, N, &in), "closed_loop_device_ex");
    else
      c.closed_loop_device(xd, ud, N, in);
    c.synchronize();
    out[direct].resize(B * 7);
    cgmres_detail::check(cgmres_hip_memcpy_d2h(h, out[direct].data(), xd, sizeof(double) * B * 4), "d2h");
    cgmres_detail::check(cgmres_hip_memcpy_d2h(h, out[direct].data() + B * 4, ud, sizeof(double) * B * 3), "d2h");
    for (double* q : {xd, ud, dd, vd}) cgmres_hip_free(h, q);
  }
  double worst = 0.0, moved = 0.0;
  for (size_t i = 0; i < out[0].size(); ++i) {
    const double e = std::fabs(out[0][i] - out[1][i]);
    worst = (e > worst || e != e) ? e : worst;
  }
  for (int i = 0; i < B * 4; ++i) moved = std::fmax(moved, std::fabs(out[0][i] - x0[i]));
  printf("max_diff %.17g moved %.6g\n", worst, moved);
  return 0;
}
