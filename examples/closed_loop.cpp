// Closed-loop example programs on the MI355X path, one binary:
//
//   closed_loop pendulum   [ticks] [out_prefix]   arm-type inverted pendulum  (shipped sizes dv=25, k_max=5)
//   closed_loop msd        [ticks] [out_prefix]   two-mass spring damper      (dv=50, k_max=5)
//   closed_loop semiactive [ticks] [out_prefix]   semi-active damper          (dv=50, k_max=5)
//   closed_loop multiple   [ticks] [out_prefix]   msd + pendulum stepped in one loop (two controllers)
//   ... --device-loop                              (the four above, anywhere on the line) the loop runs in ONE call of
//                                                  the device-resident closed loop with a stride-1 record, and the two
//                                                  files are written from its logs: same lines, no host call per tick
//   ... --device-loop --plant euler|rk4:N          the device loop against a plant of its own: N substeps of dt/N of forward
//                                                  Euler or RK4 on the model's state equation, nominal parameters
//                                                  (cgmres_hip_closed_loop_device_plant; euler:1 is the mains' plant)
//   ... --device-loop --preview                    (pendulum, msd) the set point follows a slow sinusoid, sampled once per
//                                                  tick; the device loop previews it into every tick's parameter horizon
//                                                  (cgmres_hip_closed_loop_device_preview)
//   closed_loop batch <B>  [ticks]                B perturbed pendulum controllers, dv=50, k_max=10, CgmresBatch
//   closed_loop sharded <B> <dev,dev,...> [ticks]  the same batch owned shard by shard on the listed devices
//                                                  (CgmresBatchSharded; a device may be listed twice), checked against
//                                                  one unsharded CgmresBatch on the first device
//
// The first four follow the reference's example mains step by step (<example>/main.cpp: initial state and guess
// :35-52, controller setup :54-57, loop :63-85 = control, forward-Euler plant via mul/add, one text line per tick)
// and write the same files: <prefix>_x.txt / <prefix>_u.txt, "%f" time then "\t%f" per component, and
// "Elapsed time = %f" (accumulated wall time of control() only) at the end.
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>
#include <sys/time.h>

#include <string>
#include <vector>

#include "cgmres.hpp"
#include "cgmres_batch.hpp"
#include "matrix.hpp"
#include "models.hpp"

static double now_s() {
  struct timeval tv;
  gettimeofday(&tv, NULL);
  return double(tv.tv_sec) + double(tv.tv_usec) * 1e-6;
}

// one controller + its plant + its two trajectory files
template <class Model, class Plant>
struct Loop {
  Cgmres<Model> controller;
  std::vector<double> x, u, f;
  FILE *fx, *fu;
  Loop(const std::string& prefix, const double* x0, const double* u0, const double* p)
      : x(x0, x0 + Model::dim_x), u(u0, u0 + Model::dim_u), f(Model::dim_x, 0.0) {
    std::vector<double> pt(Model::dim_p * (Model::dv + 1) + 1, 0.0);
    for (int s = 0; s <= Model::dv; ++s)
      for (int j = 0; j < Model::dim_p; ++j) pt[Model::dim_p * s + j] = p[j];
    controller.set_ptau(pt.data());
    controller.init_u0(u.data());
    controller.init_u0_newton(u.data(), x.data(), pt.data(), 10);
    fx = fopen((prefix + "_x.txt").c_str(), "w");
    fu = fopen((prefix + "_u.txt").c_str(), "w");
    if (!fx || !fu) {
      perror("fopen");
      exit(1);
    }
  }
  ~Loop() {
    fclose(fx);
    fclose(fu);
  }
  void control() { controller.control(u.data(), x.data()); }
  void plant_and_log(int tick) {
    Plant::rhs(f.data(), x.data(), u.data());
    mul(f.data(), f.data(), Model::dt, Model::dim_x);  // x = x + dxdt * dt, as two passes like the reference
    add(x.data(), x.data(), f.data(), Model::dim_x);
    fprintf(fx, "%f", Model::dt * tick);
    fprintf(fu, "%f", Model::dt * tick);
    for (double v : x) fprintf(fx, "\t%f", v);
    for (double v : u) fprintf(fu, "\t%f", v);
    fprintf(fx, "\n");
    fprintf(fu, "\n");
  }
};

static const double kPi = 3.14159265358979;  // the literal of the example mains
static const double kPendX0[4] = {kPi, kPi, 0.0, 0.0}, kPendU0[3] = {0.0, 3.0, 0.01}, kPendP[2] = {kPi / 4.0, 0.0};
static const double kMsdX0[4] = {2.0, 2.0, 0.0, 0.0}, kMsdU0[6] = {0.0, 0.0, 10.0, 10.0, 5e-4, 5e-4}, kMsdP[2] = {1, -1};
static const double kSemiX0[2] = {2.0, 0.0}, kSemiU0[3] = {0.028393761456740, 0.166095020295846, 0.030103250483332};

static bool g_device_loop = false;  // --device-loop
static cgmres_hip_loop_plant g_plant = {};  // --plant euler|rk4:N (struct_size 0: none given)
static bool g_preview = false;              // --preview
template <class Model>
static int run_single_device(const char* prefix, int ticks, const double* x0, const double* u0, const double* p);

template <class Model, class Plant>
static int run_single(const char* prefix, int ticks, const double* x0, const double* u0, const double* p) {
  if (g_device_loop) return run_single_device<Model>(prefix, ticks, x0, u0, p);
  Loop<Model, Plant> loop(prefix, x0, u0, p);
  double t_all = 0;
  for (int i = 0; i < ticks; ++i) {
    const double t0 = now_s();
    loop.control();
    t_all += now_s() - t0;
    loop.plant_and_log(i);
  }
  printf("Elapsed time = %f\n", t_all);
  return 0;
}

// --device-loop: the same controller as a batch of one whose loop never leaves the GPU.  One call records every tick
// (cgmres_hip_closed_loop_device_rec, stride 1): x after the plant step, the u that produced it and the time of the
// tick's control() — the three things a line of the files holds.  The plant is the model's own dxdt, as in the mains.
template <class Model>
struct DeviceLoop {
  CgmresBatch<Model> controller{1};
  std::vector<double> x, u, t;
  double *x_dev = nullptr, *u_dev = nullptr, *x_log = nullptr, *u_log = nullptr, *sig_dev = nullptr;
  int32_t n_samples = 0;
  std::string prefix;
  int ticks;
  DeviceLoop(const std::string& prefix_, int ticks_, const double* x0, const double* u0, const double* p)
      : x(x0, x0 + Model::dim_x), u(u0, u0 + Model::dim_u), t(ticks_ > 0 ? ticks_ : 1), prefix(prefix_), ticks(ticks_) {
    std::vector<double> pt(Model::dim_p * (Model::dv + 1) + 1, 0.0);
    for (int s = 0; s <= Model::dv; ++s)
      for (int j = 0; j < Model::dim_p; ++j) pt[Model::dim_p * s + j] = p[j];
    controller.set_ptau(pt.data());
    controller.init_u0(u.data());
    controller.init_u0_newton(u.data(), x.data(), pt.data(), 10);
    const cgmres_hip_handle h = controller.native_handle();
    const size_t n = size_t(ticks > 0 ? ticks : 1);
    double** bufs[4] = {&x_dev, &u_dev, &x_log, &u_log};
    const size_t bytes[4] = {sizeof(double) * Model::dim_x, sizeof(double) * Model::dim_u, sizeof(double) * Model::dim_x * n,
                             sizeof(double) * Model::dim_u * n};
    for (int i = 0; i < 4; ++i) cgmres_detail::check(cgmres_hip_malloc(h, reinterpret_cast<void**>(bufs[i]), bytes[i]), "malloc");
    cgmres_detail::check(cgmres_hip_memcpy_h2d(h, x_dev, x.data(), bytes[0]), "memcpy_h2d");
    cgmres_detail::check(cgmres_hip_memcpy_h2d(h, u_dev, u.data(), bytes[1]), "memcpy_h2d");
    if (g_preview && Model::dim_p > 0) {  // p(t) = p * (1 + 0.1 sin(2 pi t / 4 s)) in component 0, one sample per tick
      n_samples = int32_t(n) + 1;
      std::vector<double> sig(size_t(n_samples) * Model::dim_p);
      for (int32_t j = 0; j < n_samples; ++j)
        for (int c = 0; c < Model::dim_p; ++c)
          sig[size_t(j) * Model::dim_p + c] = c == 0 ? p[c] * (1.0 + 0.1 * sin(2.0 * kPi * Model::dt * j / 4.0)) : p[c];
      cgmres_detail::check(cgmres_hip_malloc(h, reinterpret_cast<void**>(&sig_dev), sizeof(double) * sig.size()), "malloc");
      cgmres_detail::check(cgmres_hip_memcpy_h2d(h, sig_dev, sig.data(), sizeof(double) * sig.size()), "memcpy_h2d");
    }
  }
  ~DeviceLoop() {
    for (double* q : {x_dev, u_dev, x_log, u_log, sig_dev})
      if (q) cgmres_hip_free(controller.native_handle(), q);
  }
  void enqueue() {
    cgmres_hip_loop_record rec = {};
    rec.struct_size = int32_t(sizeof rec), rec.stride = 1;
    rec.x_log_dev = x_log, rec.u_log_dev = u_log, rec.t_host = t.data();
    if (sig_dev) {
      cgmres_hip_loop_preview pv = {};
      pv.struct_size = int32_t(sizeof pv), pv.interp = CGMRES_HIP_PREVIEW_LINEAR, pv.n_samples = n_samples;
      pv.t0 = 0.0, pv.ts = Model::dt, pv.sig_dev = sig_dev;
      controller.closed_loop_device(x_dev, u_dev, ticks, nullptr, &rec, g_plant.struct_size ? &g_plant : nullptr, pv);
    } else if (g_plant.struct_size)
      controller.closed_loop_device(x_dev, u_dev, ticks, nullptr, &rec, g_plant);
    else
      controller.closed_loop_device(x_dev, u_dev, ticks, nullptr, rec);
  }
  void write_files() {
    const cgmres_hip_handle h = controller.native_handle();
    std::vector<double> xs(size_t(ticks) * Model::dim_x + 1), us(size_t(ticks) * Model::dim_u + 1);
    cgmres_detail::check(cgmres_hip_memcpy_d2h(h, xs.data(), x_log, sizeof(double) * Model::dim_x * ticks), "memcpy_d2h");
    cgmres_detail::check(cgmres_hip_memcpy_d2h(h, us.data(), u_log, sizeof(double) * Model::dim_u * ticks), "memcpy_d2h");
    FILE *fx = fopen((prefix + "_x.txt").c_str(), "w"), *fu = fopen((prefix + "_u.txt").c_str(), "w");
    if (!fx || !fu) {
      perror("fopen");
      exit(1);
    }
    for (int i = 0; i < ticks; ++i) {
      fprintf(fx, "%f", t[i]);
      fprintf(fu, "%f", t[i]);
      for (int c = 0; c < Model::dim_x; ++c) fprintf(fx, "\t%f", xs[size_t(i) * Model::dim_x + c]);
      for (int c = 0; c < Model::dim_u; ++c) fprintf(fu, "\t%f", us[size_t(i) * Model::dim_u + c]);
      fprintf(fx, "\n");
      fprintf(fu, "\n");
    }
    fclose(fx);
    fclose(fu);
  }
};

template <class Model>
static int run_single_device(const char* prefix, int ticks, const double* x0, const double* u0, const double* p) {
  DeviceLoop<Model> loop(prefix, ticks, x0, u0, p);
  const double t0 = now_s();
  loop.enqueue();
  loop.controller.synchronize();
  const double t_all = now_s() - t0;  // (control and plant together: they share the kernels)
  loop.write_files();
  printf("Elapsed time = %f\n", t_all);
  return 0;
}

static int run_multiple(const char* prefix, int ticks) {  // multiple_controller/main.cpp:89-143
  if (g_device_loop) {  // two independent controllers: their two loops are enqueued back to back and overlap
    DeviceLoop<examples::MsdModel<50, 5>> l1(std::string(prefix) + "1", ticks, kMsdX0, kMsdU0, kMsdP);
    DeviceLoop<examples::PendulumModel<25, 5>> l2(std::string(prefix) + "2", ticks, kPendX0, kPendU0, kPendP);
    const double t0 = now_s();
    l1.enqueue(), l2.enqueue();
    l1.controller.synchronize(), l2.controller.synchronize();
    const double t_all = now_s() - t0;
    l1.write_files(), l2.write_files();
    printf("Elapsed time = %f\n", t_all);
    return 0;
  }
  using M1 = examples::MsdModel<50, 5>;
  using M2 = examples::PendulumModel<25, 5>;
  Loop<M1, examples::MsdPlant> l1(std::string(prefix) + "1", kMsdX0, kMsdU0, kMsdP);
  Loop<M2, examples::PendulumPlant> l2(std::string(prefix) + "2", kPendX0, kPendU0, kPendP);
  double t_all = 0;
  for (int i = 0; i < ticks; ++i) {
    const double t0 = now_s();
    l1.control();
    l2.control();
    t_all += now_s() - t0;
    l1.plant_and_log(i);
    l2.plant_and_log(i);
  }
  printf("Elapsed time = %f\n", t_all);
  return 0;
}

static double splitmix_u01(uint64_t* state) {
  uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return double(z >> 11) * (1.0 / 9007199254740992.0);
}

static int run_batch(int B, int ticks) {
  using M = examples::PendulumModel<50, 10>;
  CgmresBatch<M> ctrl(B);
  std::vector<double> x(size_t(B) * 4), u(size_t(B) * 3), p(size_t(B) * 2), f(4);
  uint64_t seed = 12345;
  for (int b = 0; b < B; ++b) {  // SURVEY.md §8(d) perturbation recipe
    double r[5];
    for (double& v : r) v = splitmix_u01(&seed);
    x[4 * b + 0] = kPi + 0.2 * (r[0] - 0.5), x[4 * b + 1] = kPi + 0.2 * (r[1] - 0.5);
    x[4 * b + 2] = 0.2 * (r[2] - 0.5), x[4 * b + 3] = 0.2 * (r[3] - 0.5);
    p[2 * b + 0] = (kPi / 4.0) * (0.5 + r[4]), p[2 * b + 1] = 0.0;
    for (int j = 0; j < 3; ++j) u[3 * b + j] = kPendU0[j];
  }
  ctrl.set_ptau_repeat(p.data());
  ctrl.init_u0(u.data());
  ctrl.init_u0_newton(u.data(), x.data(), p.data(), 10);
  const double t0 = now_s();
  for (int i = 0; i < ticks; ++i) {
    ctrl.control(u.data(), x.data());
    for (int b = 0; b < B; ++b) {
      examples::PendulumPlant::rhs(f.data(), &x[4 * b], &u[3 * b]);
      mul(f.data(), f.data(), M::dt, 4);
      add(&x[4 * b], &x[4 * b], f.data(), 4);
    }
  }
  const double secs = now_s() - t0;
  printf("batch %d x %d ticks through host pointers: %.3f s, %.0f control steps/s; u[0] = %.12f %.12f %.12f\n", B, ticks,
         secs, double(B) * ticks / secs, u[0], u[1], u[2]);
  return 0;
}

static void seeded_pendulum_batch(int B, std::vector<double>* x, std::vector<double>* u, std::vector<double>* p) {
  x->resize(size_t(B) * 4), u->resize(size_t(B) * 3), p->resize(size_t(B) * 2);
  uint64_t seed = 12345;
  for (int b = 0; b < B; ++b) {  // SURVEY.md §8(d) perturbation recipe
    double r[5];
    for (double& v : r) v = splitmix_u01(&seed);
    (*x)[4 * b + 0] = kPi + 0.2 * (r[0] - 0.5), (*x)[4 * b + 1] = kPi + 0.2 * (r[1] - 0.5);
    (*x)[4 * b + 2] = 0.2 * (r[2] - 0.5), (*x)[4 * b + 3] = 0.2 * (r[3] - 0.5);
    (*p)[2 * b + 0] = (kPi / 4.0) * (0.5 + r[4]), (*p)[2 * b + 1] = 0.0;
    for (int j = 0; j < 3; ++j) (*u)[3 * b + j] = kPendU0[j];
  }
}

// The caller of multiple_controller/main.cpp:89-110 with B controllers on several devices: set-up, then `ticks` of the
// closed loop resident on the GPUs, then ONE gather.  The same job on a single unsharded batch must give the same bits
// (controllers are independent and both sides take the mapping the library picks for the shard size).
static int run_sharded(int B, const char* devlist, int ticks) {
  using M = examples::PendulumModel<50, 10>;
  std::vector<int32_t> devices;
  for (const char* q = devlist; *q;) {
    devices.push_back(int32_t(strtol(q, const_cast<char**>(&q), 10)));
    if (*q == ',') ++q;
  }
  std::vector<double> x0, u0, p;
  seeded_pendulum_batch(B, &x0, &u0, &p);
  std::vector<double> xs(x0), us(u0), xr(x0), ur(u0);
  CgmresBatchSharded<M> sharded(B, devices);
  sharded.set_ptau_repeat(p.data());
  sharded.init_u0(us.data());
  sharded.init_u0_newton(us.data(), xs.data(), p.data(), 10);
  sharded.upload_state(xs.data());
  const double t0 = now_s();
  sharded.closed_loop_device(ticks);
  sharded.synchronize();
  const double secs = now_s() - t0;
  sharded.download_state(xs.data(), us.data());
  for (int r = 0; r < sharded.shards(); ++r) {
    int32_t lo, hi;
    sharded.bounds(r, &lo, &hi);
    printf("shard %d: device %d, controllers [%d, %d)\n", r, devices[r], lo, hi);
  }
  // reference run: one handle, shard by shard sizes do not matter for the bits of an instance
  double worst = 0.0;
  for (int r = 0; r < sharded.shards(); ++r) {
    int32_t lo, hi;
    sharded.bounds(r, &lo, &hi);
    CgmresBatch<M> one(hi - lo, devices[0]);
    one.set_ptau_repeat(&p[2 * lo]);
    one.init_u0(&ur[3 * lo]);
    one.init_u0_newton(&ur[3 * lo], &xr[4 * lo], &p[2 * lo], 10);
    double *xd, *ud;
    cgmres_detail::check(cgmres_hip_malloc(one.native_handle(), reinterpret_cast<void**>(&xd), sizeof(double) * 4 * (hi - lo)), "malloc");
    cgmres_detail::check(cgmres_hip_malloc(one.native_handle(), reinterpret_cast<void**>(&ud), sizeof(double) * 3 * (hi - lo)), "malloc");
    cgmres_detail::check(cgmres_hip_memcpy_h2d(one.native_handle(), xd, &xr[4 * lo], sizeof(double) * 4 * (hi - lo)), "h2d");
    one.closed_loop_device(xd, ud, ticks);
    one.synchronize();
    cgmres_detail::check(cgmres_hip_memcpy_d2h(one.native_handle(), &xr[4 * lo], xd, sizeof(double) * 4 * (hi - lo)), "d2h");
    cgmres_detail::check(cgmres_hip_memcpy_d2h(one.native_handle(), &ur[3 * lo], ud, sizeof(double) * 3 * (hi - lo)), "d2h");
    cgmres_hip_free(one.native_handle(), xd), cgmres_hip_free(one.native_handle(), ud);
  }
  for (size_t i = 0; i < xs.size(); ++i) worst = fmax(worst, fabs(xs[i] - xr[i]));
  for (size_t i = 0; i < us.size(); ++i) worst = fmax(worst, fabs(us[i] - ur[i]));
  printf("sharded %d controllers x %d ticks on %zu shard(s): %.3f s, %.0f control steps/s; max |sharded - single| = %.3g; "
         "u[0] = %.12f %.12f %.12f\n", B, ticks, devices.size(), secs, double(B) * ticks / secs, worst, us[0], us[1], us[2]);
  return worst == 0.0 ? 0 : 1;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)  // the switch may stand anywhere; the positional arguments close up
    if (!strcmp(argv[i], "--device-loop")) {
      g_device_loop = true;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc, --i;
    } else if (!strcmp(argv[i], "--preview")) {
      g_preview = true;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc, --i;
    } else if (!strcmp(argv[i], "--plant") && i + 1 < argc) {  // euler | rk4, optionally :N substeps
      const char* spec = argv[i + 1];
      const char* colon = strchr(spec, ':');
      const size_t len = colon ? size_t(colon - spec) : strlen(spec);
      g_plant.struct_size = int32_t(sizeof g_plant);
      g_plant.substeps = colon ? atoi(colon + 1) : 1;
      if (len == 3 && !strncmp(spec, "rk4", 3)) {
        g_plant.integrator = CGMRES_HIP_PLANT_RK4;
      } else if (len == 5 && !strncmp(spec, "euler", 5)) {
        g_plant.integrator = CGMRES_HIP_PLANT_EULER;
      } else {
        fprintf(stderr, "--plant %s: euler|rk4[:N] expected\n", spec);
        return 1;
      }
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2, --i;
    }
  if ((g_plant.struct_size || g_preview) && !g_device_loop) {
    fprintf(stderr, "--plant and --preview need --device-loop\n");
    return 1;
  }
  const char* which = argc > 1 ? argv[1] : "pendulum";
  if (!strcmp(which, "batch")) return run_batch(argc > 2 ? atoi(argv[2]) : 4096, argc > 3 ? atoi(argv[3]) : 100);
  if (!strcmp(which, "sharded"))
    return run_sharded(argc > 2 ? atoi(argv[2]) : 4096, argc > 3 ? argv[3] : "0", argc > 4 ? atoi(argv[4]) : 100);
  const int ticks = argc > 2 ? atoi(argv[2]) : -1;
  const char* prefix = argc > 3 ? argv[3] : nullptr;
  if (!strcmp(which, "pendulum"))
    return run_single<examples::PendulumModel<25, 5>, examples::PendulumPlant>(
        prefix ? prefix : "arm_type_inverted_pendulum", ticks < 0 ? 10001 : ticks, kPendX0, kPendU0, kPendP);
  if (!strcmp(which, "msd"))
    return run_single<examples::MsdModel<50, 5>, examples::MsdPlant>(prefix ? prefix : "mass_spring_damper",
                                                                      ticks < 0 ? 20001 : ticks, kMsdX0, kMsdU0, kMsdP);
  if (!strcmp(which, "semiactive"))
    return run_single<examples::SemiactiveModel<50, 5>, examples::SemiactivePlant>(
        prefix ? prefix : "semiactive_damper", ticks < 0 ? 20001 : ticks, kSemiX0, kSemiU0, kSemiX0 /*unused: dim_p = 0*/);
  if (!strcmp(which, "multiple")) return run_multiple(prefix ? prefix : "multiple_controller_", ticks < 0 ? 10001 : ticks);
  fprintf(stderr, "usage: %s pendulum|msd|semiactive|multiple [ticks] [prefix] [--device-loop [--plant euler|rk4:N] [--preview]]  |  batch <B> [ticks]  |  sharded <B> <dev,dev,..> [ticks]\n", argv[0]);
  return 2;
}
