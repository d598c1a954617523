// libcgmres_hip.so — extern "C" entry points of include/cgmres_hip.h.
// Host side of the batched C/GMRES tick: a handle owns the HBM-resident controller state of `batch`
// instances (the private members of the reference's Cgmres/Gmres objects, cgmres.hpp:195-202 /
// gmres.hpp:120-124) behind one of three kernel mappings:
//   variant 2 "wg"      (tick_wg.hip.h)   one workgroup per 16 (or 8) instances, LDS-staged sweeps, DPP row
//                                         reductions — the default whenever the problem fits its LDS budget
//   variant 3 "wg-lean" (tick_wg.hip.h)   the same on half the LDS: two workgroups per CU — the default when a batch
//                                         needs more workgroups than the GPU has CUs
//   variant 1 "lane"    (tick_lane.hip.h) one lane per instance, reference statement order, any size
// There is no CPU implementation of the path in this library.
#include <dlfcn.h>

#include <deque>
#include <mutex>

#include "ctx_common.hip.h"
#include "factory.hip.h"
#include "gmres_plan.hip.h"
#include "record_plan.hip.h"
#include "util_kernels.hip.h"

namespace {

using cgm::fail;

// User models registered at run time (cgmres_hip_register_model): model ids CGMRES_HIP_MODEL_USER_BASE + n.
struct Plugin {
  void* dl;
  std::string path;
  cgm::ModelInfo info;
  cgmres_hip_ctx* (*make)(const cgmres_hip_config*);
  int (*probe)(const double*, const double*, const double*, const double*, double*, void*);
  const char* (*last_error)(void);
  cgm::HorizonFn* horizon;  // optional symbol: null in a plugin built before cgmres_hip_horizon_device existed
  int32_t (*record)(void);  // optional symbol: null in a plugin whose contexts predate the record kernels (status_dev)
  cgm::PlantFn* plant;      // optional symbol: null in a plugin built before cgmres_hip_closed_loop_device_plant existed
  int32_t (*preview)(void);  // optional symbol: null in a plugin whose contexts' closed loops predate LoopSeqs::preview_fill
};
std::deque<Plugin>& plugins() {  // deque: find_plugin hands out pointers that must survive later push_backs
  static std::deque<Plugin> v;
  return v;
}
std::mutex& plugins_mutex() {
  static std::mutex m;
  return m;
}
const Plugin* find_plugin(int id) {
  std::lock_guard<std::mutex> g(plugins_mutex());
  const int n = id - CGMRES_HIP_MODEL_USER_BASE;
  return n >= 0 && n < int(plugins().size()) ? &plugins()[n] : nullptr;
}

// Device operators registered at run time (cgmres_hip_register_operator): ids 0, 1, ...
struct OpPlugin {
  void* dl;
  std::string path;
  int32_t len, n_params;
  int (*solve)(int32_t, int32_t, int32_t, double, const double*, double*, const double*, int32_t*, int32_t*);
  const char* (*last_error)(void);
  void (*plan)(int32_t, int32_t*);  // optional symbol: null in a plugin built before the row form existed (serial form)
};
std::deque<OpPlugin>& op_plugins() {
  static std::deque<OpPlugin> v;
  return v;
}
const OpPlugin* find_op(int id) {
  std::lock_guard<std::mutex> g(plugins_mutex());
  return id >= 0 && id < int(op_plugins().size()) ? &op_plugins()[id] : nullptr;
}

// Opens a plugin of either kind and files its record in `reg`; *index receives its place there (that of the earlier
// record when the path is registered already).  `kind` is "model" or "operator", `prefix` what its symbols start with;
// `syms` names the symbols behind the ABI one and where their addresses go in `pl`, `check` fills the rest of `pl` and
// refuses bad dimensions.
struct Sym {
  const char* name;
  void* slot;  // address of a function-pointer member of the record
  bool required;
};
template <class Rec, class Check>
int open_plugin(std::deque<Rec>& reg, const char* kind, const std::string& prefix, const char* path, int32_t* index, Rec& pl,
                std::initializer_list<Sym> syms, Check check) {
  if (!path || !index) return fail(CGMRES_HIP_EINVAL, "register_%s: null argument", kind);
  {
    std::lock_guard<std::mutex> g(plugins_mutex());
    for (size_t n = 0; n < reg.size(); ++n)
      if (reg[n].path == path) {
        *index = int(n);
        return 0;
      }
  }
  void* dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!dl) return fail(CGMRES_HIP_EINVAL, "register_%s: %s", kind, dlerror());
  pl.dl = dl, pl.path = path;
  auto abi = reinterpret_cast<int32_t (*)(void)>(dlsym(dl, (prefix + "abi").c_str()));
  bool all = abi != nullptr;
  for (const Sym& s : syms) {
    void* f = dlsym(dl, (prefix + s.name).c_str());
    std::memcpy(s.slot, &f, sizeof f);
    all = all && (f || !s.required);
  }
  int rc = 0;
  if (!all)
    rc = fail(CGMRES_HIP_EINVAL, "register_%s: %s is not a cgmres_hip %s plugin", kind, path, kind);
  else if (abi() != CGMRES_HIP_ABI_VERSION)
    rc = fail(CGMRES_HIP_EINVAL, "register_%s: plugin ABI %d, library has %d", kind, abi(), CGMRES_HIP_ABI_VERSION);
  else
    rc = check(pl);
  if (rc) {
    dlclose(dl);
    return rc;
  }
  std::lock_guard<std::mutex> g(plugins_mutex());
  reg.push_back(pl);
  *index = int(reg.size()) - 1;
  return 0;
}

// The built-in models, dispatched in one place: f is called with a tag that names the device model and the two
// factories of its translation units (inst_*.hip); false for an id that is none of them.
template <template <class> class M>
struct Builtin {
  using Dev = M<double>;
  cgmres_hip_ctx* (*make_f64)(const cgmres_hip_config&, int*);
  cgmres_hip_ctx* (*make_f32)(const cgmres_hip_config&, int*);
  cgm::HorizonFn *horizon_f64, *horizon_f32;  // cgmres_hip_horizon_device on a context that factory made
  cgm::PlantFn *plant_f64, *plant_f32;        // one launch of the plant kernel on such a context
};
template <class F>
bool with_builtin(int id, F&& f) {
  switch (id) {
    case CGMRES_HIP_MODEL_PENDULUM:
      f(Builtin<cgm::PendulumDev>{cgm::make_pendulum_f64, cgm::make_pendulum_f32, cgm::horizon_pendulum_f64, cgm::horizon_pendulum_f32,
                                    cgm::plant_pendulum_f64, cgm::plant_pendulum_f32});
      return true;
    case CGMRES_HIP_MODEL_MSD:
      f(Builtin<cgm::MsdDev>{cgm::make_msd_f64, cgm::make_msd_f32, cgm::horizon_msd_f64, cgm::horizon_msd_f32, cgm::plant_msd_f64,
                               cgm::plant_msd_f32});
      return true;
    case CGMRES_HIP_MODEL_SEMIACTIVE:
      f(Builtin<cgm::SemiactiveDev>{cgm::make_semiactive_f64, cgm::make_semiactive_f32, cgm::horizon_semiactive_f64,
                                     cgm::horizon_semiactive_f32, cgm::plant_semiactive_f64, cgm::plant_semiactive_f32});
      return true;
  }
  return false;
}

cgm::ModelInfo model_info(int id, bool* ok) {
  *ok = true;
  if (const Plugin* pl = find_plugin(id)) return pl->info;
  cgm::ModelInfo mi{};
  *ok = with_builtin(id, [&](auto m) { mi = decltype(m)::Dev::info(); });
  return mi;
}

int check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(CGMRES_HIP_ENODEV, "no HIP device visible: this library has no CPU path");
  if (device < 0 || device >= n) return fail(CGMRES_HIP_ENODEV, "device %d out of range (%d visible)", device, n);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(CGMRES_HIP_ENODEV, "device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
  return 0;
}

cgmres_hip_ctx* make_ctx(const cgmres_hip_config& cfg, int* resolved) {
  const bool f32 = cfg.dtype == CGMRES_HIP_F32;
  if (const Plugin* pl = find_plugin(cfg.model_id)) {  // user models: the plugin picks the mapping (user_model.hip.h)
    *resolved = cfg.variant;
    return pl->make(&cfg);
  }
  cgmres_hip_ctx* c = nullptr;
  with_builtin(cfg.model_id, [&](auto m) { c = (f32 ? m.make_f32 : m.make_f64)(cfg, resolved); });
  return c;
}

int enter(cgmres_hip_handle h, bool ok = true, const char* what = nullptr) {
  HIP_TRY(hipSetDevice(h->cfg.device));
  return ok ? 0 : fail(CGMRES_HIP_EINVAL, "%s", what);
}

// what the three closed-loop entry points end in
int closed_loop(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks, const cgm::LoopSeqs& sq) {
  if (int rc = enter(h, u && x, "closed_loop: null pointer")) return rc;
  return h->closed_loop(x, u, n_ticks, sq);
}

// The input sequences of cgmres_hip_closed_loop_device_ex / ..._rec, checked: what both end in before closed_loop()
int loop_seqs(cgmres_hip_handle h, const void* x, const void* u, int32_t n_ticks, const cgmres_hip_loop_inputs* in, cgm::LoopSeqs* out) {
  if (n_ticks < 0) return fail(CGMRES_HIP_EINVAL, "n_ticks < 0");
  cgm::LoopSeqs sq;
  if (in) {
    if (in->struct_size != int32_t(sizeof(cgmres_hip_loop_inputs)))
      return fail(CGMRES_HIP_EINVAL, "closed_loop_device_ex: struct_size %d, this library's cgmres_hip_loop_inputs has %d",
                  in->struct_size, int(sizeof(cgmres_hip_loop_inputs)));
    const int32_t pi[3] = {in->ptau_per_instance, in->dist_per_instance, in->meas_per_instance};
    for (int32_t v : pi)
      if (v != 0 && v != 1) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_ex: a *_per_instance field is %d, not 0 or 1", v);
    // the reference's alias guard (cgmres.hpp:119-124): an input sequence must not share bytes with the loop's outputs
    const size_t es = h->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8, B = size_t(h->cfg.batch);
    auto overlaps = [&](const void* seq, int per_instance, const void* out, size_t out_bytes) {
      if (!seq || !out) return false;
      const uintptr_t a = reinterpret_cast<uintptr_t>(seq), b = reinterpret_cast<uintptr_t>(out);
      const size_t seq_bytes = size_t(n_ticks) * (per_instance ? B : 1) * h->nx * es;
      return a < b + out_bytes && b < a + seq_bytes;
    };
    const struct { const char* name; const void* p; int pi; } seqs[2] = {{"dist_seq_dev", in->dist_seq_dev, in->dist_per_instance},
                                                                        {"meas_seq_dev", in->meas_seq_dev, in->meas_per_instance}};
    for (const auto& s : seqs) {
      if (overlaps(s.p, s.pi, x, B * h->nx * es))
        return fail(CGMRES_HIP_EINVAL, "closed_loop_device_ex: %s overlaps x_dev (cgmres.hpp DEBUG_MODE alias guard)", s.name);
      if (overlaps(s.p, s.pi, u, B * h->nu * es))
        return fail(CGMRES_HIP_EINVAL, "closed_loop_device_ex: %s overlaps u_dev (cgmres.hpp DEBUG_MODE alias guard)", s.name);
    }
    sq.ptau = h->np ? in->ptau_seq_dev : nullptr, sq.ptau_per_instance = in->ptau_per_instance;
    sq.dist = in->dist_seq_dev, sq.dist_per_instance = in->dist_per_instance;
    sq.meas = in->meas_seq_dev, sq.meas_per_instance = in->meas_per_instance;
  }
  *out = sq;
  return 0;
}

// Record j of a recorded loop (LoopSeqs::rec_take): the rows of the caller's logs, on the context's stream
int take_loop_record(void* rec, cgmres_hip_ctx* c, int j, const void* x, const void* u, const int32_t* n_ax, const int32_t* reason,
                     double t) {
  const cgmres_hip_loop_record* r = static_cast<const cgmres_hip_loop_record*>(rec);
  const size_t es = c->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8, B = size_t(c->cfg.batch), row = size_t(j);
  if (r->t_host) r->t_host[j] = t;
  auto at = [&](auto* p, size_t bytes) {  // row j of a log, or null
    return p ? static_cast<decltype(p)>(static_cast<void*>(static_cast<char*>(static_cast<void*>(p)) + row * bytes)) : nullptr;
  };
  return cgm::record_take(c, x, u, n_ax, reason,
                          cgm::RecordOut{at(r->x_log_dev, B * c->nx * es), at(r->u_log_dev, B * c->nu * es), at(r->n_ax_log_dev, B * 4),
                                         at(r->reason_log_dev, B * 4), r->centre_dev, at(r->moments_log_dev, size_t(c->nx + c->nu) * 32),
                                         at(r->counts_log_dev, size_t(c->cfg.k_max + 7) * 4)});
}

// The record kernels touch members of cgmres_hip_ctx that a context built before them does not have: such a plugin is told
// to rebuild, as for cgmres_hip_horizon_device.
int plugin_records(cgmres_hip_handle h, const char* who) {
  const Plugin* pl = find_plugin(h->cfg.model_id);
  if (pl && !pl->record)
    return fail(CGMRES_HIP_EINVAL, "%s: the plugin %s was built before this entry point existed: rebuild it", who, pl->path.c_str());
  return 0;
}

// The plant parameters of a model: their number and nominal values (0 for a user model); false for an unknown id
bool plant_theta_of(int id, int* n_theta, const double** nominal) {
  *n_theta = 0, *nominal = nullptr;
  if (find_plugin(id)) return true;
  return with_builtin(id, [&](auto m) {
    using Dev = typename decltype(m)::Dev;
    *n_theta = Dev::NTHETA, *nominal = Dev::theta_nominal;
  });
}

// A cgmres_hip_loop_plant, checked; on success the plant fields of *sq are set (plant_step: the model's launch function)
int plant_check(cgmres_hip_handle h, const char* who, const cgmres_hip_loop_plant* pl, cgm::LoopSeqs* sq) {
  if (pl->struct_size != int32_t(sizeof(cgmres_hip_loop_plant)))
    return fail(CGMRES_HIP_EINVAL, "%s: struct_size %d, this library's cgmres_hip_loop_plant has %d", who, pl->struct_size,
                int(sizeof(cgmres_hip_loop_plant)));
  if (pl->reserved[0] != 0 || pl->reserved[1] != 0)
    return fail(CGMRES_HIP_EINVAL, "%s: cgmres_hip_loop_plant.reserved must be 0 (got %d, %d)", who, pl->reserved[0], pl->reserved[1]);
  if (pl->integrator != CGMRES_HIP_PLANT_EULER && pl->integrator != CGMRES_HIP_PLANT_RK4)
    return fail(CGMRES_HIP_EINVAL, "%s: unknown integrator %d (CGMRES_HIP_PLANT_EULER = 0, CGMRES_HIP_PLANT_RK4 = 1)", who, pl->integrator);
  if (pl->substeps < 1 || pl->substeps > 4096) return fail(CGMRES_HIP_EINVAL, "%s: substeps %d outside 1 .. 4096", who, pl->substeps);
  if (pl->theta_per_instance != 0 && pl->theta_per_instance != 1)
    return fail(CGMRES_HIP_EINVAL, "%s: theta_per_instance is %d, not 0 or 1", who, pl->theta_per_instance);
  int n_theta = 0;
  const double* nominal = nullptr;
  plant_theta_of(h->cfg.model_id, &n_theta, &nominal);
  if (pl->theta_dev && n_theta == 0)
    return fail(CGMRES_HIP_EINVAL, "%s: theta_dev given, but model %d has no plant parameters (n_theta = 0)", who, h->cfg.model_id);
  cgm::PlantFn* fn = nullptr;
  if (const Plugin* p = find_plugin(h->cfg.model_id)) {
    if (!p->plant)
      return fail(CGMRES_HIP_EINVAL, "%s: the plugin %s was built before this entry point existed: rebuild it", who, p->path.c_str());
    fn = p->plant;
  } else {
    with_builtin(h->cfg.model_id, [&](auto m) { fn = h->cfg.dtype == CGMRES_HIP_F32 ? m.plant_f32 : m.plant_f64; });
  }
  if (!fn) return fail(CGMRES_HIP_EINVAL, "%s: unknown model_id %d", who, h->cfg.model_id);
  sq->plant_step = fn, sq->plant_integrator = pl->integrator, sq->plant_substeps = pl->substeps;
  sq->plant_theta = pl->theta_dev, sq->plant_theta_inst = pl->theta_dev && pl->theta_per_instance ? n_theta : 0;
  return 0;
}
// bytes of the theta array of a checked plant
size_t plant_theta_bytes(cgmres_hip_handle h, const cgmres_hip_loop_plant* pl) {
  int n_theta = 0;
  const double* nominal = nullptr;
  plant_theta_of(h->cfg.model_id, &n_theta, &nominal);
  return size_t(pl->theta_per_instance ? h->cfg.batch : 1) * n_theta * (h->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8);
}
// a plugin reports its failures through its own copy of the error string
int plant_rc(cgmres_hip_handle h, int rc) {
  if (rc)
    if (const Plugin* p = find_plugin(h->cfg.model_id)) cgm::g_err = p->last_error();
  return rc;
}

// A cgmres_hip_loop_preview, checked; on success *out describes the signal.  A plugin built before LoopSeqs carried a preview
// reads only the struct's old prefix and would run without it: told to rebuild.
int preview_check(cgmres_hip_handle h, const char* who, const cgmres_hip_loop_preview* pv, cgm::PreviewSig* out) {
  if (pv->struct_size != int32_t(sizeof(cgmres_hip_loop_preview)))
    return fail(CGMRES_HIP_EINVAL, "%s: struct_size %d, this library's cgmres_hip_loop_preview has %d", who, pv->struct_size,
                int(sizeof(cgmres_hip_loop_preview)));
  if (pv->reserved[0] != 0 || pv->reserved[1] != 0)
    return fail(CGMRES_HIP_EINVAL, "%s: cgmres_hip_loop_preview.reserved must be 0 (got %d, %d)", who, pv->reserved[0], pv->reserved[1]);
  if (pv->interp != CGMRES_HIP_PREVIEW_HOLD && pv->interp != CGMRES_HIP_PREVIEW_LINEAR)
    return fail(CGMRES_HIP_EINVAL, "%s: unknown interp %d (CGMRES_HIP_PREVIEW_HOLD = 0, CGMRES_HIP_PREVIEW_LINEAR = 1)", who, pv->interp);
  if (pv->sig_per_instance != 0 && pv->sig_per_instance != 1)
    return fail(CGMRES_HIP_EINVAL, "%s: sig_per_instance is %d, not 0 or 1", who, pv->sig_per_instance);
  if (pv->n_samples < 1) return fail(CGMRES_HIP_EINVAL, "%s: n_samples %d < 1", who, pv->n_samples);
  if (!std::isfinite(pv->ts) || !(pv->ts > 0)) return fail(CGMRES_HIP_EINVAL, "%s: ts must be finite and > 0 (got %g)", who, pv->ts);
  if (!std::isfinite(pv->t0)) return fail(CGMRES_HIP_EINVAL, "%s: t0 must be finite (got %g)", who, pv->t0);
  if (h->np > 0 && !pv->sig_dev) return fail(CGMRES_HIP_EINVAL, "%s: null sig_dev on a model with dim_p = %d", who, h->np);
  const Plugin* pl = find_plugin(h->cfg.model_id);
  if (pl && !pl->preview)
    return fail(CGMRES_HIP_EINVAL, "%s: the plugin %s was built before this entry point existed: rebuild it", who, pl->path.c_str());
  out->sig = pv->sig_dev, out->per_instance = pv->sig_per_instance, out->n_samples = pv->n_samples, out->interp = pv->interp;
  out->t0 = pv->t0, out->ts = pv->ts;
  return 0;
}
size_t preview_sig_bytes(cgmres_hip_handle h, const cgmres_hip_loop_preview* pv) {
  return size_t(pv->sig_per_instance ? h->cfg.batch : 1) * size_t(pv->n_samples) * h->np * (h->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8);
}

__global__ void sincos_selftest_kernel(const double* a, double* s, double* c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cgm::sincos_f64(a[i], &s[i], &c[i]);
}

}  // namespace

#define NEED(h) \
  if (!(h)) return fail(CGMRES_HIP_EINVAL, "%s: null handle", __func__)
// Where a call on a handle, past NEED and whatever the entry point refuses before it touches a device, enters the
// library: the handle's device (the contexts select none themselves), then, where given, the condition on the arguments
// that is refused with the text `what`.
#define ENTER(h, ...) \
  if (int rc_ = enter(h, ##__VA_ARGS__)) return rc_

extern "C" {

const char* cgmres_hip_last_error(void) { return cgm::g_err.c_str(); }

int cgmres_hip_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int cgmres_hip_model_info(int32_t model_id, int32_t dims[5], double tuning[6]) {
  bool ok;
  const cgm::ModelInfo mi = model_info(model_id, &ok);
  if (!ok) return fail(CGMRES_HIP_EINVAL, "unknown model_id %d", model_id);
  if (dims) dims[0] = mi.dim_x, dims[1] = mi.dim_u, dims[2] = mi.dim_p, dims[3] = mi.dv, dims[4] = mi.k_max;
  if (tuning)
    tuning[0] = mi.dt, tuning[1] = mi.h, tuning[2] = mi.zeta, tuning[3] = mi.Tf, tuning[4] = mi.alpha, tuning[5] = mi.tol;
  return 0;
}

int cgmres_hip_default_config(int32_t model_id, cgmres_hip_config* cfg) {
  bool ok;
  const cgm::ModelInfo mi = model_info(model_id, &ok);
  if (!ok) return fail(CGMRES_HIP_EINVAL, "unknown model_id %d", model_id);
  if (!cfg) return fail(CGMRES_HIP_EINVAL, "null cfg");
  std::memset(cfg, 0, sizeof *cfg);
  cfg->abi_version = CGMRES_HIP_ABI_VERSION;
  cfg->model_id = model_id, cfg->dtype = CGMRES_HIP_F64, cfg->batch = 1, cfg->dv = mi.dv, cfg->k_max = mi.k_max;
  cfg->tol = mi.tol, cfg->dt = mi.dt, cfg->h = mi.h, cfg->zeta = mi.zeta, cfg->Tf = mi.Tf, cfg->alpha = mi.alpha;
  return 0;
}

int cgmres_hip_model_probe(int32_t model_id, int32_t device, const double* x, const double* u, const double* p,
                           const double* lmd, double* out) {
  bool ok;
  const cgm::ModelInfo mi = model_info(model_id, &ok);
  if (!ok) return fail(CGMRES_HIP_EINVAL, "unknown model_id %d", model_id);
  if (!x || !u || !lmd || !out || (mi.dim_p && !p)) return fail(CGMRES_HIP_EINVAL, "model_probe: null pointer");
  if (int rc = check_device(device)) return rc;
  HIP_TRY(hipSetDevice(device));
  const int n_in = mi.dim_x + mi.dim_u + mi.dim_p + mi.dim_x, n_out = 3 * mi.dim_x + mi.dim_u;
  double* d = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), (n_in + n_out + 1) * sizeof(double)));
  double *dx = d, *du = dx + mi.dim_x, *dp = du + mi.dim_u, *dl = dp + mi.dim_p, *dout = dl + mi.dim_x;
  // every step is checked: the facade's model fingerprint (include/cgmres.hpp) trusts `out` to pick a device model
  hipError_t e = hipMemcpy(dx, x, mi.dim_x * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(du, u, mi.dim_u * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && mi.dim_p) e = hipMemcpy(dp, p, mi.dim_p * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dl, lmd, mi.dim_x * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xff, n_out * 8);  // (NaN pattern: a kernel that did not run cannot pass for a match)
  const char* what = "copy in";
  if (e == hipSuccess) {
    what = "kernel";
    if (const Plugin* pl = find_plugin(model_id)) {
      if (pl->probe(dx, du, dp, dl, dout, nullptr) != 0) e = hipErrorLaunchFailure;
    } else {
      with_builtin(model_id, [&](auto m) { cgm::probe_kernel<typename decltype(m)::Dev><<<1, 1>>>(dx, du, dp, dl, dout); });
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();  // (execution errors of the probe kernel surface here)
  }
  if (e == hipSuccess) {
    what = "copy out";
    e = hipMemcpy(out, dout, n_out * 8, hipMemcpyDeviceToHost);
  }
  (void)hipFree(d);
  if (e != hipSuccess) return fail(CGMRES_HIP_ERUNTIME, "model_probe (%s): %s", what, hipGetErrorString(e));
  return 0;
}

int cgmres_hip_selftest_sincos(int32_t device, const double* a, int32_t n, double* s, double* c) {
  if (!a || !s || !c || n < 0) return fail(CGMRES_HIP_EINVAL, "selftest_sincos: bad argument");
  if (int rc = check_device(device)) return rc;
  HIP_TRY(hipSetDevice(device));
  double* d = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), size_t(3) * (n ? n : 1) * sizeof(double)));
  hipError_t e = hipMemcpy(d, a, size_t(n) * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && n > 0) {
    sincos_selftest_kernel<<<(n + 255) / 256, 256>>>(d, d + n, d + 2 * size_t(n), n);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(s, d + n, size_t(n) * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(c, d + 2 * size_t(n), size_t(n) * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(CGMRES_HIP_ERUNTIME, "selftest_sincos: %s", hipGetErrorString(e));
  return 0;
}

int cgmres_hip_register_model(const char* plugin_path, int32_t* model_id) {
  Plugin pl{};
  void (*info)(int32_t*, double*) = nullptr;
  int32_t n = 0;
  const int rc = open_plugin(
      plugins(), "model", "cgmres_hip_plugin_", plugin_path, model_id ? &n : nullptr, pl,
      {{"info", &info, true}, {"make", &pl.make, true}, {"probe", &pl.probe, true}, {"last_error", &pl.last_error, true},
       {"horizon", &pl.horizon, false}, {"record", &pl.record, false}, {"plant", &pl.plant, false},
       {"preview", &pl.preview, false}},
      [&](Plugin& q) {
        int32_t dims[5];
        double tun[6];
        info(dims, tun);
        q.info = {dims[0], dims[1], dims[2], dims[3], dims[4], tun[0], tun[1], tun[2], tun[3], tun[4], tun[5]};
        if (dims[0] < 1 || dims[1] < 1 || dims[2] < 0)
          return fail(CGMRES_HIP_EINVAL, "register_model: bad dimensions %d/%d/%d", dims[0], dims[1], dims[2]);
        return 0;
      });
  if (!rc) *model_id = CGMRES_HIP_MODEL_USER_BASE + n;
  return rc;
}

int cgmres_hip_register_operator(const char* plugin_path, int32_t* op_id) {
  OpPlugin pl{};
  void (*info)(int32_t*) = nullptr;
  // (plan: an optional symbol, see OpPlugin)
  return open_plugin(op_plugins(), "operator", "cgmres_hip_opplugin_", plugin_path, op_id, pl,
                     {{"info", &info, true}, {"solve", &pl.solve, true}, {"last_error", &pl.last_error, true}, {"plan", &pl.plan, false}},
                     [&](OpPlugin& q) {
                       int32_t dims[2];
                       info(dims);
                       q.len = dims[0], q.n_params = dims[1];
                       if (q.len < 1 || q.n_params < 0)
                         return fail(CGMRES_HIP_EINVAL, "register_operator: bad dimensions %d/%d", dims[0], dims[1]);
                       return 0;
                     });
}

int cgmres_hip_operator_info(int32_t op_id, int32_t dims[2]) {
  const OpPlugin* pl = find_op(op_id);
  if (!pl || !dims) return fail(CGMRES_HIP_EINVAL, "operator_info: unknown operator %d", op_id);
  dims[0] = pl->len, dims[1] = pl->n_params;
  return 0;
}

int cgmres_hip_operator_plan(int32_t op_id, int32_t k_max, int32_t out[2]) {
  const OpPlugin* pl = find_op(op_id);
  if (!pl || !out) return fail(CGMRES_HIP_EINVAL, "operator_plan: unknown operator %d", op_id);
  if (!cgm::gmres_sizes_ok(pl->len, k_max))
    return fail(CGMRES_HIP_EINVAL, "operator_plan: k_max %d is no solve of a len %d operator", k_max, pl->len);
  if (pl->plan) {
    pl->plan(k_max, out);  // the function the plugin's own solve launches by
  } else {
    const cgm::GmresPlan p = cgm::gmres_plan(pl->len, k_max, false);
    out[0] = p.form, out[1] = p.mapping;
  }
  return 0;
}

int cgmres_hip_gmres_user(int32_t op_id, int32_t device, int32_t batch, int32_t k_max, double tol, const double* params,
                          double* x, const double* b, int32_t* n_ax, int32_t* reason) {
  const OpPlugin* pl = find_op(op_id);
  if (!pl) return fail(CGMRES_HIP_EINVAL, "gmres_user: unknown operator %d", op_id);
  if (int rc = check_device(device)) return rc;
  const int rc = pl->solve(device, batch, k_max, tol, params, x, b, n_ax, reason);
  if (rc) cgm::g_err = pl->last_error();  // (the plugin has its own copy of the error string)
  return rc;
}

int cgmres_hip_create(const cgmres_hip_config* cfg, cgmres_hip_handle* out) {
  if (!cfg || !out) return fail(CGMRES_HIP_EINVAL, "create: null argument");
  *out = nullptr;
  if (cfg->abi_version != CGMRES_HIP_ABI_VERSION)
    return fail(CGMRES_HIP_EINVAL, "ABI version %d, library has %d", cfg->abi_version, CGMRES_HIP_ABI_VERSION);
  bool ok;
  const cgm::ModelInfo mi = model_info(cfg->model_id, &ok);
  if (!ok) return fail(CGMRES_HIP_EINVAL, "unknown model_id %d", cfg->model_id);
  if (cfg->dtype != CGMRES_HIP_F64 && cfg->dtype != CGMRES_HIP_F32) return fail(CGMRES_HIP_EINVAL, "bad dtype %d", cfg->dtype);
  if (cfg->batch < 1 || cfg->dv < 1 || cfg->k_max < 1)
    return fail(CGMRES_HIP_EINVAL, "batch/dv/k_max must be >= 1 (got %d/%d/%d)", cfg->batch, cfg->dv, cfg->k_max);
  // the reference indexes with uint16_t/int16_t (gmres.hpp:29, matrix.hpp:10): same limits here
  const long len = long(mi.dim_u) * cfg->dv;
  if (len >= 32768 || len * (cfg->k_max + 1) >= 65536)
    return fail(CGMRES_HIP_EINVAL, "dim_u*dv = %ld with k_max = %d exceeds the reference's 16-bit index range", len, cfg->k_max);
  if (!(cfg->h > 0) || !(cfg->dt > 0) || !(cfg->tol >= 0)) return fail(CGMRES_HIP_EINVAL, "h, dt must be > 0 and tol >= 0");
  // a NaN / Inf tuning constant would only show as NaN controls many ticks later (1 - zeta*h, 1/h, dtau(t) scale every residual)
  for (double v : {cfg->dt, cfg->h, cfg->zeta, cfg->Tf, cfg->alpha})
    if (!std::isfinite(v))
      return fail(CGMRES_HIP_EINVAL, "dt, h, zeta, Tf, alpha must be finite (got %g, %g, %g, %g, %g)", cfg->dt, cfg->h, cfg->zeta,
                  cfg->Tf, cfg->alpha);
  if (cfg->variant < 0 || cfg->variant > 4) return fail(CGMRES_HIP_EINVAL, "unknown variant %d", cfg->variant);
  if (cfg->flags & ~(CGMRES_HIP_FLAG_SERIAL_COSTATE | CGMRES_HIP_FLAG_IPW8 | CGMRES_HIP_FLAG_NO_BINNING | CGMRES_HIP_FLAG_TWO_PASS_COSTATE |
                     CGMRES_HIP_FLAG_NO_WAVE | CGMRES_HIP_FLAG_WAVE_FRESH_TRIG | CGMRES_HIP_FLAG_WAVE_SERIAL_SWEEPS |
                     CGMRES_HIP_FLAG_SERIAL_STATE_SWEEP))
    return fail(CGMRES_HIP_EINVAL, "unknown flags 0x%x", cfg->flags);
  if (cfg->reserved != 0) return fail(CGMRES_HIP_EINVAL, "cgmres_hip_config.reserved must be 0 (got %d)", cfg->reserved);
  if (int rc = check_device(cfg->device)) return rc;
  int resolved = 0;
  cgmres_hip_ctx* c = make_ctx(*cfg, &resolved);
  if (!c) return fail(CGMRES_HIP_EINVAL, "variant %d does not support model %d with dv = %d, k_max = %d", resolved,
                      cfg->model_id, cfg->dv, cfg->k_max);
  c->cfg = *cfg;  // init() replaces cfg.variant (the request, 0 = library's choice) by the resolved mapping
  if (int rc = c->init()) {
    if (const Plugin* pl = find_plugin(cfg->model_id)) cgm::g_err = pl->last_error();  // the plugin has its own copy
    delete c;
    return rc;
  }
  *out = c;
  return 0;
}

int cgmres_hip_destroy(cgmres_hip_handle h) {
  NEED(h);
  delete h;
  return 0;
}
int cgmres_hip_get_config(cgmres_hip_handle h, cgmres_hip_config* cfg) {
  NEED(h);
  if (!cfg) return fail(CGMRES_HIP_EINVAL, "null cfg");
  *cfg = h->cfg;
  return 0;
}
const char* cgmres_hip_variant_name(cgmres_hip_handle h) { return h ? h->variant_name() : nullptr; }
int cgmres_hip_set_ptau(cgmres_hip_handle h, const void* p, int per_instance) {
  NEED(h);
  ENTER(h, h->np == 0 || p, "set_ptau: null pointer");
  return h->set_ptau(p, per_instance, false);
}
int cgmres_hip_set_ptau_repeat(cgmres_hip_handle h, const void* p, int per_instance) {
  NEED(h);
  ENTER(h, h->np == 0 || p, "set_ptau: null pointer");
  return h->set_ptau(p, per_instance, true);
}
int cgmres_hip_init_u0(cgmres_hip_handle h, const void* u0, int per_instance) {
  NEED(h);
  ENTER(h, u0, "init_u0: null pointer");
  return h->init_u0(u0, per_instance);
}
int cgmres_hip_init_u0_newton(cgmres_hip_handle h, void* u0, const void* x0, const void* p0, int32_t n_loop) {
  NEED(h);
  ENTER(h, u0 && x0 && (h->np == 0 || p0), "init_u0_newton: null pointer");
  if (n_loop < 0) return fail(CGMRES_HIP_EINVAL, "init_u0_newton: n_loop < 0");
  return h->init_u0_newton(u0, x0, p0, n_loop);
}
// The reference's DEBUG_MODE builds exit(-1) when an output argument aliases an input (cgmres.hpp:119-124,
// matrix.hpp:76-81); at the ABI the same calls are refused.
int cgmres_hip_control(cgmres_hip_handle h, void* u, const void* x) {
  NEED(h);
  if (u && u == x) return fail(CGMRES_HIP_EINVAL, "control: u and x are the same buffer (cgmres.hpp DEBUG_MODE alias guard)");
  ENTER(h, u && x, "control: null pointer");
  return h->control_host(u, x);
}
int cgmres_hip_control_device(cgmres_hip_handle h, void* u, const void* x) {
  NEED(h);
  if (u && u == x) return fail(CGMRES_HIP_EINVAL, "control_device: u and x are the same buffer (cgmres.hpp DEBUG_MODE alias guard)");
  ENTER(h, u && x, "control: null pointer");
  return h->control_device(u, x, nullptr);
}
int cgmres_hip_closed_loop_device(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks) {
  NEED(h);
  if (n_ticks < 0) return fail(CGMRES_HIP_EINVAL, "n_ticks < 0");
  return closed_loop(h, x, u, n_ticks, cgm::LoopSeqs{});
}
int cgmres_hip_closed_loop_device_ptau(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks, const void* ptau_seq,
                                       int per_instance) {
  NEED(h);
  if (n_ticks < 0) return fail(CGMRES_HIP_EINVAL, "n_ticks < 0");
  if (h->np && !ptau_seq) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_ptau: null ptau sequence");
  cgm::LoopSeqs sq;
  sq.ptau = h->np ? ptau_seq : nullptr, sq.ptau_per_instance = per_instance;
  return closed_loop(h, x, u, n_ticks, sq);
}
int cgmres_hip_closed_loop_device_ex(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks, const cgmres_hip_loop_inputs* in) {
  NEED(h);
  cgm::LoopSeqs sq;
  if (int rc = loop_seqs(h, x, u, n_ticks, in, &sq)) return rc;
  return closed_loop(h, x, u, n_ticks, sq);
}
int cgmres_hip_record_plan(int32_t n_ticks, int32_t stride, int32_t* n_rec, int32_t* launch_ticks, int32_t cap, int32_t* n_launches) {
  if (n_ticks < 0) return fail(CGMRES_HIP_EINVAL, "record_plan: n_ticks < 0");
  if (stride < 1) return fail(CGMRES_HIP_EINVAL, "record_plan: stride %d < 1", stride);
  if (!cgm::record_plan(n_ticks, stride, CGMRES_HIP_TICKS_PER_LAUNCH, n_rec, launch_ticks, cap, n_launches))
    return fail(CGMRES_HIP_EINVAL, "record_plan: %d ticks at stride %d take more than cap = %d launches", n_ticks, stride, cap);
  return 0;
}
int cgmres_hip_ensemble_device(cgmres_hip_handle h, const void* x, const void* u, const cgmres_hip_ensemble_out* out) {
  NEED(h);
  if (!x) return fail(CGMRES_HIP_EINVAL, "ensemble_device: null x_dev");
  if (!u) return fail(CGMRES_HIP_EINVAL, "ensemble_device: null u_dev");
  if (!out) return fail(CGMRES_HIP_EINVAL, "ensemble_device: null out");
  if (out->struct_size != int32_t(sizeof(cgmres_hip_ensemble_out)))
    return fail(CGMRES_HIP_EINVAL, "ensemble_device: struct_size %d, this library's cgmres_hip_ensemble_out has %d", out->struct_size,
                int(sizeof(cgmres_hip_ensemble_out)));
  if (out->reserved != 0) return fail(CGMRES_HIP_EINVAL, "ensemble_device: cgmres_hip_ensemble_out.reserved must be 0 (got %d)", out->reserved);
  if (!out->moments_dev && !out->counts_dev)
    return fail(CGMRES_HIP_EINVAL, "ensemble_device: no output wanted (moments_dev and counts_dev are both null)");
  if (int rc = plugin_records(h, "ensemble_device")) return rc;
  ENTER(h);
  const int32_t *n_ax = nullptr, *reason = nullptr;
  if (int rc = h->status_dev(&n_ax, &reason)) return rc;
  return cgm::record_take(h, x, u, n_ax, reason, cgm::RecordOut{nullptr, nullptr, nullptr, nullptr, out->centre_dev, out->moments_dev, out->counts_dev});
}
int cgmres_hip_closed_loop_device_rec(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks, const cgmres_hip_loop_inputs* in,
                                      const cgmres_hip_loop_record* rec) {
  return cgmres_hip_closed_loop_device_preview(h, x, u, n_ticks, in, rec, nullptr, nullptr);
}
int cgmres_hip_closed_loop_device_plant(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks, const cgmres_hip_loop_inputs* in,
                                        const cgmres_hip_loop_record* rec, const cgmres_hip_loop_plant* plant) {
  return cgmres_hip_closed_loop_device_preview(h, x, u, n_ticks, in, rec, plant, nullptr);
}
int cgmres_hip_closed_loop_device_preview(cgmres_hip_handle h, void* x, void* u, int32_t n_ticks, const cgmres_hip_loop_inputs* in,
                                          const cgmres_hip_loop_record* rec, const cgmres_hip_loop_plant* plant,
                                          const cgmres_hip_loop_preview* preview) {
  NEED(h);
  cgm::LoopSeqs sq;
  if (int rc = loop_seqs(h, x, u, n_ticks, in, &sq)) return rc;
  struct Range { const char* name; const void* p; size_t bytes; };
  auto overlap = [](const Range& a, const Range& b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a.p), pb = reinterpret_cast<uintptr_t>(b.p);
    return pa < pb + b.bytes && pb < pa + a.bytes;
  };
  const size_t es = h->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8, B = size_t(h->cfg.batch), seq_rows = size_t(n_ticks);
  const size_t nc = size_t(h->nx + h->nu);
  Range theta{"theta_dev", nullptr, 0};
  if (plant) {
    if (int rc = plant_check(h, "closed_loop_device_plant", plant, &sq)) return rc;
    theta = {"theta_dev", plant->theta_dev, plant_theta_bytes(h, plant)};
    // the alias guard, extended: theta shares no byte with x_dev, u_dev or an input sequence (the logs: below)
    const Range io[5] = {{"x_dev", x, B * h->nx * es},
                         {"u_dev", u, B * h->nu * es},
                         {"ptau_seq_dev", sq.ptau, seq_rows * (sq.ptau_per_instance ? B : 1) * h->np * (h->cfg.dv + 1) * es},
                         {"dist_seq_dev", sq.dist, seq_rows * (sq.dist_per_instance ? B : 1) * h->nx * es},
                         {"meas_seq_dev", sq.meas, seq_rows * (sq.meas_per_instance ? B : 1) * h->nx * es}};
    for (const Range& o : io)
      if (overlap(theta, o))
        return fail(CGMRES_HIP_EINVAL, "closed_loop_device_plant: theta_dev overlaps %s (cgmres.hpp DEBUG_MODE alias guard)", o.name);
  }
  Range sig{"sig_dev", nullptr, 0};
  if (preview) {
    if (int rc = preview_check(h, "closed_loop_device_preview", preview, &sq.preview)) return rc;
    if (in && in->ptau_seq_dev)
      return fail(CGMRES_HIP_EINVAL, "closed_loop_device_preview: ptau_seq_dev and a preview are both given: the preview forms every tick's ptau");
    sig = {"sig_dev", preview->sig_dev, preview_sig_bytes(h, preview)};
    // the alias guard, extended: the signal shares no byte with x_dev, u_dev, an input sequence or theta (the logs: below)
    const Range io[5] = {{"x_dev", x, B * h->nx * es},
                         {"u_dev", u, B * h->nu * es},
                         {"dist_seq_dev", sq.dist, seq_rows * (sq.dist_per_instance ? B : 1) * h->nx * es},
                         {"meas_seq_dev", sq.meas, seq_rows * (sq.meas_per_instance ? B : 1) * h->nx * es},
                         theta};
    for (const Range& o : io)
      if (overlap(sig, o))
        return fail(CGMRES_HIP_EINVAL, "closed_loop_device_preview: sig_dev overlaps %s (cgmres.hpp DEBUG_MODE alias guard)", o.name);
    if (h->np > 0) sq.preview_fill = cgm::preview_fill;  // (dim_p = 0: ignored, as a ptau sequence is)
  }
  auto run = [&] { return plant ? plant_rc(h, closed_loop(h, x, u, n_ticks, sq)) : closed_loop(h, x, u, n_ticks, sq); };
  if (!rec) return run();
  if (rec->struct_size != int32_t(sizeof(cgmres_hip_loop_record)))
    return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: struct_size %d, this library's cgmres_hip_loop_record has %d",
                rec->struct_size, int(sizeof(cgmres_hip_loop_record)));
  if (rec->reserved[0] != 0 || rec->reserved[1] != 0)
    return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: cgmres_hip_loop_record.reserved must be 0 (got %d, %d)", rec->reserved[0],
                rec->reserved[1]);
  if (rec->stride < 1) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: stride %d < 1", rec->stride);
  if (!x) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: null x_dev");
  if (!u) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: null u_dev");
  if (!rec->x_log_dev && !rec->u_log_dev && !rec->n_ax_log_dev && !rec->reason_log_dev && !rec->t_host && !rec->moments_log_dev &&
      !rec->counts_log_dev)
    return run();
  // the alias guard of ..._ex, extended: a log shares no byte with x_dev, u_dev, another log, an input sequence or theta
  const size_t n_rec = size_t(n_ticks / rec->stride);
  const Range logs[6] = {{"x_log_dev", rec->x_log_dev, n_rec * B * h->nx * es},       {"u_log_dev", rec->u_log_dev, n_rec * B * h->nu * es},
                         {"n_ax_log_dev", rec->n_ax_log_dev, n_rec * B * 4},          {"reason_log_dev", rec->reason_log_dev, n_rec * B * 4},
                         {"moments_log_dev", rec->moments_log_dev, n_rec * nc * 32}, {"counts_log_dev", rec->counts_log_dev, n_rec * size_t(h->cfg.k_max + 7) * 4}};
  const Range others[8] = {{"x_dev", x, B * h->nx * es},
                           {"u_dev", u, B * h->nu * es},
                           {"ptau_seq_dev", sq.ptau, seq_rows * (sq.ptau_per_instance ? B : 1) * h->np * (h->cfg.dv + 1) * es},
                           {"dist_seq_dev", sq.dist, seq_rows * (sq.dist_per_instance ? B : 1) * h->nx * es},
                           {"meas_seq_dev", sq.meas, seq_rows * (sq.meas_per_instance ? B : 1) * h->nx * es},
                           {"centre_dev", rec->centre_dev, nc * 8},
                           theta,
                           sig};
  for (int i = 0; i < 6; ++i) {
    for (const Range& o : others)
      if (overlap(logs[i], o)) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: %s overlaps %s (cgmres.hpp DEBUG_MODE alias guard)", logs[i].name, o.name);
    for (int k = i + 1; k < 6; ++k)
      if (overlap(logs[i], logs[k])) return fail(CGMRES_HIP_EINVAL, "closed_loop_device_rec: %s overlaps %s (cgmres.hpp DEBUG_MODE alias guard)", logs[i].name, logs[k].name);
  }
  if (int rc = plugin_records(h, "closed_loop_device_rec")) return rc;
  sq.rec_stride = rec->stride, sq.rec_take = take_loop_record, sq.rec = const_cast<cgmres_hip_loop_record*>(rec);
  return run();
}
int cgmres_hip_plant_info(int32_t model_id, int32_t* n_theta, double* nominal, int32_t cap) {
  int n = 0;
  const double* nom = nullptr;
  if (!plant_theta_of(model_id, &n, &nom)) return fail(CGMRES_HIP_EINVAL, "unknown model_id %d", model_id);
  if (n_theta) *n_theta = n;
  if (nominal) {
    if (cap < n) return fail(CGMRES_HIP_EINVAL, "plant_info: model %d has %d plant parameters, cap = %d", model_id, n, cap);
    for (int i = 0; i < n; ++i) nominal[i] = nom[i];
  }
  return 0;
}
int cgmres_hip_plant_step_device(cgmres_hip_handle h, void* x, const void* u, const cgmres_hip_loop_plant* plant) {
  NEED(h);
  if (!plant) return fail(CGMRES_HIP_EINVAL, "plant_step_device: null plant");
  if (!x) return fail(CGMRES_HIP_EINVAL, "plant_step_device: null x_dev");
  if (!u) return fail(CGMRES_HIP_EINVAL, "plant_step_device: null u_dev");
  cgm::LoopSeqs sq;
  if (int rc = plant_check(h, "plant_step_device", plant, &sq)) return rc;
  const size_t es = h->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8, B = size_t(h->cfg.batch), tb = plant_theta_bytes(h, plant);
  auto overlaps = [&](const void* o, size_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(plant->theta_dev), b = reinterpret_cast<uintptr_t>(o);
    return plant->theta_dev && tb && a < b + bytes && b < a + tb;
  };
  if (overlaps(x, B * h->nx * es)) return fail(CGMRES_HIP_EINVAL, "plant_step_device: theta_dev overlaps x_dev (cgmres.hpp DEBUG_MODE alias guard)");
  if (overlaps(u, B * h->nu * es)) return fail(CGMRES_HIP_EINVAL, "plant_step_device: theta_dev overlaps u_dev (cgmres.hpp DEBUG_MODE alias guard)");
  ENTER(h);
  cgm::PlantCall c;
  c.x = x, c.u = u, c.theta = sq.plant_theta, c.theta_inst = sq.plant_theta_inst;
  c.integrator = sq.plant_integrator, c.substeps = sq.plant_substeps;
  return plant_rc(h, sq.plant_step(h, c));
}
int cgmres_hip_preview_device(cgmres_hip_handle h, const cgmres_hip_loop_preview* preview, int32_t n_ticks, void* rows) {
  NEED(h);
  if (!preview) return fail(CGMRES_HIP_EINVAL, "preview_device: null preview");
  if (!rows) return fail(CGMRES_HIP_EINVAL, "preview_device: null rows_dev");
  if (n_ticks < 0) return fail(CGMRES_HIP_EINVAL, "preview_device: n_ticks < 0");
  cgm::PreviewSig s;
  if (int rc = preview_check(h, "preview_device", preview, &s)) return rc;
  const size_t es = h->cfg.dtype == CGMRES_HIP_F32 ? 4 : 8, sb = preview_sig_bytes(h, preview);
  const size_t rb = size_t(n_ticks) * h->cfg.batch * h->np * (h->cfg.dv + 1) * es;
  const uintptr_t a = reinterpret_cast<uintptr_t>(preview->sig_dev), b = reinterpret_cast<uintptr_t>(rows);
  if (sb && rb && a < b + rb && b < a + sb)
    return fail(CGMRES_HIP_EINVAL, "preview_device: sig_dev overlaps rows_dev (cgmres.hpp DEBUG_MODE alias guard)");
  ENTER(h);
  return cgm::preview_export(h, s, n_ticks, rows);
}
int cgmres_hip_horizon_device(cgmres_hip_handle h, const void* x, const cgmres_hip_horizon_out* out) {
  NEED(h);
  if (!x) return fail(CGMRES_HIP_EINVAL, "horizon_device: null x_dev");
  if (!out) return fail(CGMRES_HIP_EINVAL, "horizon_device: null out");
  if (out->struct_size != int32_t(sizeof(cgmres_hip_horizon_out)))
    return fail(CGMRES_HIP_EINVAL, "horizon_device: struct_size %d, this library's cgmres_hip_horizon_out has %d", out->struct_size,
                int(sizeof(cgmres_hip_horizon_out)));
  if (out->reserved != 0) return fail(CGMRES_HIP_EINVAL, "horizon_device: cgmres_hip_horizon_out.reserved must be 0 (got %d)", out->reserved);
  if (!out->xtau_dev && !out->ltau_dev && !out->F_dev && !out->fnorm_dev)
    return fail(CGMRES_HIP_EINVAL, "horizon_device: no output wanted (xtau_dev, ltau_dev, F_dev and fnorm_dev are all null)");
  ENTER(h);
  if (const Plugin* pl = find_plugin(h->cfg.model_id)) {  // user models: the plugin knows the context's concrete type
    if (!pl->horizon)
      return fail(CGMRES_HIP_EINVAL, "horizon_device: the plugin %s was built before this entry point existed: rebuild it",
                  pl->path.c_str());
    const int rc = pl->horizon(h, x, out);
    if (rc) cgm::g_err = pl->last_error();  // (the plugin has its own copy of the error string)
    return rc;
  }
  int rc = fail(CGMRES_HIP_EINVAL, "horizon_device: unknown model_id %d", h->cfg.model_id);
  with_builtin(h->cfg.model_id, [&](auto m) { rc = (h->cfg.dtype == CGMRES_HIP_F32 ? m.horizon_f32 : m.horizon_f64)(h, x, out); });
  return rc;
}
int cgmres_hip_shard_bounds(int32_t n, int32_t world, int32_t rank, int32_t* lo, int32_t* hi) {
  if (n < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi)
    return fail(CGMRES_HIP_EINVAL, "shard_bounds: n = %d, world = %d, rank = %d", n, world, rank);
  const int32_t base = n / world, extra = n % world;
  *lo = rank * base + (rank < extra ? rank : extra);
  *hi = *lo + base + (rank < extra ? 1 : 0);
  return 0;
}
int cgmres_hip_synchronize(cgmres_hip_handle h) {
  NEED(h);
  ENTER(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}
int cgmres_hip_get_time(cgmres_hip_handle h, double* t) {
  NEED(h);
  if (t) *t = h->time();
  return 0;
}
int cgmres_hip_get_state(cgmres_hip_handle h, double* t, void* U, void* dUdt) {
  NEED(h);
  ENTER(h);
  return h->get_state(t, U, dUdt);
}
int cgmres_hip_set_state(cgmres_hip_handle h, double t, const void* U, const void* dUdt) {
  NEED(h);
  ENTER(h);
  return h->set_state(t, U, dUdt);
}
int cgmres_hip_state_rows(cgmres_hip_handle h, void** U, void** dUdt, int32_t* pitch) {
  NEED(h);
  if (!U || !dUdt || !pitch) return fail(CGMRES_HIP_EINVAL, "state_rows: null pointer");
  return h->state_rows(U, dUdt, pitch);
}
int cgmres_hip_get_status(cgmres_hip_handle h, int32_t* n_ax, int32_t* reason) {
  NEED(h);
  ENTER(h);
  return h->get_status(n_ax, reason);
}
int cgmres_hip_get_krylov(cgmres_hip_handle h, void* V, void* H, void* rho, void* g) {
  NEED(h);
  ENTER(h);
  return h->get_krylov(V, H, rho, g);
}
int cgmres_hip_F_func(cgmres_hip_handle h, void* ret, const void* U, const void* x, double t) {
  NEED(h);
  if (!ret || !U || !x) return fail(CGMRES_HIP_EINVAL, "F_func: null pointer");
  if (ret == U || ret == x) return fail(CGMRES_HIP_EINVAL, "F_func: ret aliases an input (cgmres.hpp:119-124)");
  ENTER(h);
  return h->hook_F(ret, U, x, t);
}
int cgmres_hip_prepare(cgmres_hip_handle h, void* b, const void* x) {
  NEED(h);
  if (!x) return fail(CGMRES_HIP_EINVAL, "prepare: null pointer");
  ENTER(h);
  return h->hook_prepare(b, x);
}
int cgmres_hip_Ax_func(cgmres_hip_handle h, void* out, const void* v) {
  NEED(h);
  if (!out || !v) return fail(CGMRES_HIP_EINVAL, "Ax_func: null pointer");
  if (out == v) return fail(CGMRES_HIP_EINVAL, "Ax_func: Ax aliases v (cgmres.hpp:119-124)");
  ENTER(h);
  return h->hook_Ax(out, v);
}
int cgmres_hip_gmres(cgmres_hip_handle h, void* x, const void* b) {
  NEED(h);
  if (!x || !b) return fail(CGMRES_HIP_EINVAL, "gmres: null pointer");
  if (x == b) return fail(CGMRES_HIP_EINVAL, "gmres: x aliases b (matrix.hpp:76-81)");
  ENTER(h);
  return h->hook_gmres(x, b);
}
int cgmres_hip_timer_start(cgmres_hip_handle h) {
  NEED(h);
  ENTER(h);
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  return 0;
}
int cgmres_hip_timer_stop(cgmres_hip_handle h, float* ms) {
  NEED(h);
  ENTER(h);
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev1));
  float v = 0;
  HIP_TRY(hipEventElapsedTime(&v, h->ev0, h->ev1));
  if (ms) *ms = v;
  return 0;
}
int cgmres_hip_malloc(cgmres_hip_handle h, void** p, uint64_t bytes) {
  NEED(h);
  if (!p) return fail(CGMRES_HIP_EINVAL, "malloc: null pointer");
  ENTER(h);
  HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
  return 0;
}
int cgmres_hip_free(cgmres_hip_handle h, void* p) {
  NEED(h);
  ENTER(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipFree(p));
  return 0;
}
int cgmres_hip_memcpy_h2d(cgmres_hip_handle h, void* dst, const void* src, uint64_t bytes) {
  NEED(h);
  ENTER(h);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}
int cgmres_hip_memcpy_d2h(cgmres_hip_handle h, void* dst, const void* src, uint64_t bytes) {
  NEED(h);
  ENTER(h);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

#ifdef CGM_STAMPS
/* diagnostic build only (tools/phase_stamps.py): copies and clears the 64 stamp words of the pendulum/f64 wg context */
int cgmres_hip_debug_stamps(long long* out) {
  long long* p = cgm::debug_stamps_ptr();
  if (!p || !out) return fail(CGMRES_HIP_EINVAL, "no stamp buffer");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, p, 64 * sizeof(long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(p, 0, 64 * sizeof(long long)));
  return 0;
}
#endif

#ifdef CGM_AMAX
/* diagnostic build only (tools/rot_increments.py): copies and clears the 16 words of cgm_amax_record (wg_stamps.hip.h) */
int cgmres_hip_debug_amax(unsigned long long* out) {
  unsigned long long* p = cgm::debug_amax_ptr();
  if (!p || !out) return fail(CGMRES_HIP_EINVAL, "no increment buffer");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(p, 0, 16 * sizeof(unsigned long long)));
  return 0;
}
#endif

}  // extern "C"
