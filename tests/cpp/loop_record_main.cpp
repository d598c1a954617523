// CgmresBatch::closed_loop_device(x, u, n, in, cgmres_hip_loop_record) and ensemble_device against the direct C calls on
// a second batch: prints the largest difference over the final x, u, the logs and the ensemble of the final row
// (tests/test_gpu_loop_record.py expects 0), how far the state moved, and the number of counting instances.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../examples/models.hpp"
#include "cgmres_batch.hpp"

using M = examples::PendulumModel<50, 10>;
constexpr int B = 20, N = 12, STRIDE = 4, NREC = N / STRIDE, NC = 7, KM = 10;

static double* to_dev(cgmres_hip_handle h, const std::vector<double>& v) {
  void* d = nullptr;
  cgmres_detail::check(cgmres_hip_malloc(h, &d, sizeof(double) * v.size()), "malloc");
  cgmres_detail::check(cgmres_hip_memcpy_h2d(h, d, v.data(), sizeof(double) * v.size()), "h2d");
  return static_cast<double*>(d);
}
template <class Q>
static Q* dev_alloc(cgmres_hip_handle h, size_t n) {
  void* d = nullptr;
  cgmres_detail::check(cgmres_hip_malloc(h, &d, sizeof(Q) * n), "malloc");
  return static_cast<Q*>(d);
}
template <class Q>
static void append(cgmres_hip_handle h, std::vector<double>* out, const Q* dev, size_t n) {
  std::vector<Q> tmp(n);
  cgmres_detail::check(cgmres_hip_memcpy_d2h(h, tmp.data(), dev, sizeof(Q) * n), "d2h");
  for (Q v : tmp) out->push_back(double(v));
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
  double counting = 0.0;
  for (int direct = 0; direct < 2; ++direct) {
    CgmresBatch<M> c(B);
    std::vector<double> u(u0);
    c.set_ptau_repeat(p.data());
    c.init_u0(u.data());
    c.init_u0_newton(u.data(), x0.data(), p.data(), 10);
    cgmres_hip_handle h = c.native_handle();
    double *xd = to_dev(h, x0), *ud = to_dev(h, u0), *dd = to_dev(h, d), *vd = to_dev(h, v);
    double *xl = dev_alloc<double>(h, NREC * B * 4), *ul = dev_alloc<double>(h, NREC * B * 3);
    double *ml = dev_alloc<double>(h, NREC * NC * 4), *me = dev_alloc<double>(h, NC * 4);
    int32_t *kl = dev_alloc<int32_t>(h, NREC * B), *rl = dev_alloc<int32_t>(h, NREC * B);
    int32_t *cl = dev_alloc<int32_t>(h, NREC * (KM + 7)), *ce = dev_alloc<int32_t>(h, KM + 7);
    std::vector<double> t(NREC, -1.0);
    const cgmres_hip_loop_inputs in = {int32_t(sizeof(cgmres_hip_loop_inputs)), 1, 1, 1, nullptr, dd, vd};
    cgmres_hip_loop_record rec = {};
    rec.struct_size = int32_t(sizeof rec), rec.stride = STRIDE;
    rec.x_log_dev = xl, rec.u_log_dev = ul, rec.n_ax_log_dev = kl, rec.reason_log_dev = rl, rec.t_host = t.data();
    rec.moments_log_dev = ml, rec.counts_log_dev = cl;
    cgmres_hip_ensemble_out ens = {int32_t(sizeof(cgmres_hip_ensemble_out)), 0, nullptr, me, ce};
    if (direct) {
      cgmres_detail::check(cgmres_hip_closed_loop_device_rec(h, xd, ud, N, &in, &rec), "closed_loop_device_rec");
      cgmres_detail::check(cgmres_hip_ensemble_device(h, xd, ud, &ens), "ensemble_device");
    } else {
      c.closed_loop_device(xd, ud, N, &in, rec);
      c.ensemble_device(xd, ud, ens);
    }
    c.synchronize();
    std::vector<double>& o = out[direct];
    append(h, &o, xd, B * 4), append(h, &o, ud, B * 3), append(h, &o, xl, NREC * B * 4), append(h, &o, ul, NREC * B * 3);
    append(h, &o, kl, NREC * B), append(h, &o, rl, NREC * B), append(h, &o, ml, NREC * NC * 4), append(h, &o, cl, NREC * (KM + 7));
    append(h, &o, me, NC * 4), append(h, &o, ce, KM + 7);
    counting = o.back();
    for (double tt : t) o.push_back(tt);
    for (double* q : {xd, ud, dd, vd, xl, ul, ml, me}) cgmres_hip_free(h, q);
    for (int32_t* q : {kl, rl, cl, ce}) cgmres_hip_free(h, q);
  }
  double worst = out[0].size() == out[1].size() ? 0.0 : 1.0, moved = 0.0;
  for (size_t i = 0; i < out[0].size() && i < out[1].size(); ++i) {
    const double e = std::fabs(out[0][i] - out[1][i]);
    worst = (e > worst || e != e) ? e : worst;
  }
  for (int i = 0; i < B * 4; ++i) moved = std::fmax(moved, std::fabs(out[0][i] - x0[i]));
  printf("max_diff %.17g moved %.6g counting %g t_last %.17g\n", worst, moved, counting, out[0].back());
  return 0;
}
