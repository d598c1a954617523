/* cgmres_hip.h — C ABI of libcgmres_hip.so: batched C/GMRES control ticks on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of blockahead/CGMRES_cpp: the per-tick FDGMRES solve
 *     Cgmres<Model>::control()      reference include/cgmres.hpp:78-110
 *       F_func / Ax_func            reference include/cgmres.hpp:113-175
 *       Gmres::gmres()              reference include/gmres.hpp:28-112
 * batched over `batch` independent controller instances that advance in lock-step (one shared t).
 * The reference has no FFI; its boundary is the C++ class surface, which include/cgmres.hpp (façade)
 * re-creates on top of the entry points below.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative CGMRES_HIP_E* code otherwise; the message of the
 *     last failure on the calling thread is cgmres_hip_last_error().  No exceptions cross the ABI.
 *   - `void*` vectors hold `double` (dtype F64) or `float` (dtype F32) scalars.
 *   - all vectors are INSTANCE-MAJOR, instance b first, then the reference's own layout:
 *       x[b][dim_x], u[b][dim_u], U[b][dim_u*stage + j] (cgmres.hpp:13,57),
 *       ptau[b][dim_p*stage + j], stage = 0..dv (cgmres.hpp:17,37-38).
 *     Host entry points take host pointers; *_device entry points take device pointers with the same
 *     layout (HBM resident: nothing crosses PCIe in them).
 *   - one handle = one GPU + one HIP stream; a handle is not re-entrant, distinct handles are independent
 *     (same threading contract as distinct Cgmres objects).
 *   - there is NO CPU fallback: without a usable gfx950 device cgmres_hip_create fails.
 */
#ifndef CGMRES_HIP_H_
#define CGMRES_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cgmres_hip_config gained `flags`; plugin contract (the model plugin picks the mapping, closed loop with a reference
 *    sequence); exit reason CGMRES_HIP_EXIT_NONFINITE.  A plugin or binding built against version 1 is rejected.
 * 3: plugin contract (closed loop with a process-disturbance and a measurement-noise sequence:
 *    cgmres_hip_closed_loop_device_ex).  A plugin or binding built against version 2 is rejected. */
#define CGMRES_HIP_ABI_VERSION 3

/* problem definitions compiled into the library (reference <example>/model.hpp) */
enum {
  CGMRES_HIP_MODEL_PENDULUM = 0,   /* arm_type_inverted_pendulum/model.hpp == multiple_controller/model2.hpp */
  CGMRES_HIP_MODEL_MSD = 1,        /* mass_spring_damper/model.hpp        == multiple_controller/model1.hpp */
  CGMRES_HIP_MODEL_SEMIACTIVE = 2, /* semiactive_damper/model.hpp */
  CGMRES_HIP_MODEL_COUNT = 3,
  CGMRES_HIP_MODEL_USER_BASE = 1000 /* ids of user models registered with cgmres_hip_register_model */
};
enum { CGMRES_HIP_F64 = 0, CGMRES_HIP_F32 = 1 };

/* error codes */
enum {
  CGMRES_HIP_OK = 0,
  CGMRES_HIP_EINVAL = -1,   /* bad argument / unsupported configuration */
  CGMRES_HIP_ENODEV = -2,   /* no usable gfx950 device */
  CGMRES_HIP_ERUNTIME = -3, /* HIP runtime error */
  CGMRES_HIP_ENOMEM = -4
};

/* per-instance exit reason of the last solve (the reference only prints "Breakdown", gmres.hpp:64) */
enum {
  CGMRES_HIP_EXIT_NATURAL = 0,        /* all k_max Arnoldi iterations ran      gmres.hpp:46 */
  CGMRES_HIP_EXIT_CONVERGED = 1,      /* |rho_e[k+1]| < tol                     gmres.hpp:93-95 */
  CGMRES_HIP_EXIT_SMALL_RESIDUAL = 2, /* ||r0|| < tol, dUdt untouched           gmres.hpp:39-41 */
  CGMRES_HIP_EXIT_BREAKDOWN = 3,      /* |h(k+1,k)| < DBL_EPSILON, dUdt untouched  gmres.hpp:63-65 */
  /* ||r0|| or h(k+1,k) is NaN/Inf: the reference has no test for it — every comparison with a NaN is false, the solve
   * runs on and NaNs propagate into dUdt, U and u.  Here the solve of that instance stops at the first
   * non-finite norm, its dUdt is set to NaN (what the reference ends up with), and the status says why. */
  CGMRES_HIP_EXIT_NONFINITE = 4
};

/* cgmres_hip_config.flags: choices inside a mapping that are normally the library's (measurement / A-B use) */
enum {
  CGMRES_HIP_FLAG_SERIAL_COSTATE = 1, /* wg mapping: keep the one-lane-per-instance costate sweep (no chunk-parallel scan) */
  CGMRES_HIP_FLAG_IPW8 = 2,           /* wg mapping: 8 instead of 16 instances per workgroup where that fits */
  CGMRES_HIP_FLAG_NO_BINNING = 4,     /* closed loop: keep instances in caller order inside the workgroups (no k-binning) */
  CGMRES_HIP_FLAG_TWO_PASS_COSTATE = 8, /* wg mapping: the two-pass chunk-parallel costate sweep also where the LDS-scratch form fits */
  CGMRES_HIP_FLAG_NO_WAVE = 16,        /* library's choice of mapping: never the wave mapping (small batches stay on wg) */
  CGMRES_HIP_FLAG_WAVE_FRESH_TRIG = 32, /* wave mapping and the row-parallel wg kernel of the pendulum: every Newton iteration
                                          evaluates sin/cos afresh (the path taken when an angle moves by more than the
                                          rotation range between iterations) */
  CGMRES_HIP_FLAG_WAVE_SERIAL_SWEEPS = 64, /* wave mapping: every mat-vec takes the serial state sweep (the fall-back of a Newton
                                          iteration that does not settle) */
  CGMRES_HIP_FLAG_SERIAL_STATE_SWEEP = 128 /* wg mapping, fp64: keep the serial state sweep in the Arnoldi loop instead of the
                                          row-parallel sweeps (tick_wg.hip.h: NWT), which the library takes where they apply
                                          (full LDS plan, k_max <= 12: pendulum 33 <= dv <= 53, semi-active damper dv <= 53) */
};

/* cgmres_hip_closed_loop_device advances up to this many consecutive ticks per kernel launch (the controller
 * state stays on chip between them); a tool that divides kernel time by ticks needs the number. */
#define CGMRES_HIP_TICKS_PER_LAUNCH 10

/* Run-time counterpart of the `static constexpr` block of a reference Model (e.g.
 * arm_type_inverted_pendulum/model.hpp:7-35), which Cgmres re-exports (cgmres.hpp:179-188). */
typedef struct cgmres_hip_config {
  int32_t abi_version; /* CGMRES_HIP_ABI_VERSION */
  int32_t model_id;    /* CGMRES_HIP_MODEL_* */
  int32_t dtype;       /* CGMRES_HIP_F64 / _F32 */
  int32_t batch;       /* number of controller instances B >= 1 */
  int32_t dv;          /* Model::dv    horizon stages */
  int32_t k_max;       /* Model::k_max GMRES iterations */
  int32_t device;      /* HIP device ordinal */
  int32_t variant;     /* kernel mapping: 0 = library's choice, 1 = "lane", 2 = "wg" (one workgroup per CU: everything
                          of 16 instances in LDS), 3 = "wg-lean" (half the LDS, two workgroups per CU),
                          4 = "wave" (one wavefront per controller, horizon recurrences as wave scans: the latency
                          mapping for batches smaller than the GPU; user models take it only when asked for
                          explicitly, within dim_x <= 4, dim_u <= 6, dv <= 63, k_max <= 10); get_config returns the
                          resolved value */
  int32_t flags;       /* CGMRES_HIP_FLAG_* (0 = library defaults) */
  int32_t reserved;    /* 0 */
  double tol;          /* Model::tol */
  double dt;           /* Model::dt   sampling period */
  double h;            /* Model::h    forward-difference step */
  double zeta;         /* Model::zeta */
  double Tf;           /* Model::Tf */
  double alpha;        /* Model::alpha */
  void* stream;        /* hipStream_t to launch on; NULL = the library creates its own */
} cgmres_hip_config;

typedef struct cgmres_hip_ctx* cgmres_hip_handle;

/* ---- registry -------------------------------------------------------------------------------- */
/* dims[0..4] = dim_x, dim_u, dim_p, shipped dv, shipped k_max; tuning[0..5] = dt, h, zeta, Tf, alpha, tol */
int cgmres_hip_model_info(int32_t model_id, int32_t dims[5], double tuning[6]);
/* Fills every field of *cfg from the registry (shipped dv / k_max / tuning), batch = 1, device = 0. */
int cgmres_hip_default_config(int32_t model_id, cgmres_hip_config* cfg);
/* Evaluates the DEVICE model functions at one probe point (fp64) so a host binding can fingerprint a
 * user Model class against the registry: out = [dxdt(dim_x) | dPhidx(dim_x) | dHdx(dim_x) | dHdu(dim_u)]. */
int cgmres_hip_model_probe(int32_t model_id, int32_t device, const double* x, const double* u, const double* p,
                           const double* lmd, double* out);
/* Registers a USER model: `plugin_path` is a shared object generated from a reference-style Model header
 * (static constexpr dim_x/.../tol and static dxdt/dPhidx/dHdx/dHdu/ddHduu, <example>/model.hpp:7-76) by
 * cgmres_cpp_amd/plugin.py (hipcc, gfx950).  *model_id receives an id >= CGMRES_HIP_MODEL_USER_BASE that every
 * other entry point accepts; such models run in fp64, on the "wg" mapping when their sizes fit its LDS plan
 * (the affine costate split is generated from the user's own dHdx / dHdu, csrc/user_model.hip.h) and on the "lane"
 * mapping otherwise.  An explicit variant = 4 runs them on the "wave" mapping (serial state sweep inside the wave,
 * costate recurrence as a scan of dim_x x dim_x affine maps) where the wg mapping serves the sizes and dim_x <= 4,
 * dim_u <= 6, dv <= 63, k_max <= 10; outside those limits it fails with CGMRES_HIP_EINVAL.  Registering the same path twice returns the same id.  This is what a `Cgmres<Model>` facade binds for a Model that is not in the registry. */
int cgmres_hip_register_model(const char* plugin_path, int32_t* model_id);
/* ---- stand-alone Gmres with a caller-supplied operator: class Gmres, reference include/gmres.hpp:8-129 ------------ */
/* Registers a device OPERATOR: `plugin_path` is a shared object generated by cgmres_cpp_amd/plugin.py
 * (build_operator) from a header with `struct Op { static constexpr int len, n_params; ... }` — the device build of a
 * subclass's `Ax_func` (gmres.hpp:26) — whose product comes in one of two forms (or both; detected at compile time):
 *   static double Ax_row(int i, const double* x, const double* params);   the ROW form: element i of A x.  The rows of
 *       a product run on all 64 lanes of the wavefront that owns the system.  Write this one whenever a row can be
 *       computed on its own (stencils, sparse and dense rows, anything without a recurrence across rows).
 *   static void Ax(double* Ax, const double* x, const double* params);    the SERIAL form: the whole vector, like
 *       Ax_func.  One lane runs it while 63 wait; for operators that cannot be split by rows.
 * With both defined the device uses Ax_row (Ax then serves the host subclass).  *op_id receives an id for cgmres_hip_gmres_user; the same path twice returns the same id. */
int cgmres_hip_register_operator(const char* plugin_path, int32_t* op_id);
/* dims[0] = len, dims[1] = n_params of a registered operator */
int cgmres_hip_operator_info(int32_t op_id, int32_t dims[2]);
/* out[0] = 0 serial Ax / 1 Ax_row; out[1] = 0 one lane per system / 1 one wavefront per system, for this k_max.
 * Pure host arithmetic: needs no GPU.  It is the function cgmres_hip_gmres_user launches by.  A plugin built before the
 * row form existed reports the serial form. */
int cgmres_hip_operator_plan(int32_t op_id, int32_t k_max, int32_t out[2]);
/* Gmres::gmres(x, b) (gmres.hpp:28-112) for `batch` independent systems A(params_i) x_i = b_i, all with the same
 * k_max and tol, on the GPU: x [batch][len] in/out (the warm start, :33), b [batch][len], params [batch][n_params]
 * (NULL when n_params = 0); n_ax / reason [batch] as in cgmres_hip_get_status (NULL skips).  Host pointers; blocks. */
int cgmres_hip_gmres_user(int32_t op_id, int32_t device, int32_t batch, int32_t k_max, double tol, const double* params,
                          double* x, const double* b, int32_t* n_ax, int32_t* reason);
/* Diagnostic: the device sin/cos the horizon sweeps use (fp64), evaluated at n host-supplied arguments. */
int cgmres_hip_selftest_sincos(int32_t device, const double* a, int32_t n, double* s, double* c);
const char* cgmres_hip_last_error(void);
int cgmres_hip_device_count(void);

/* ---- lifetime: Cgmres() / ~Cgmres(), cgmres.hpp:11-30 ------------------------------------------- */
/* State after create: t = 0, U = 0, dUdt = 0 (the reference leaves dUdt uninitialised, cgmres.hpp:14). */
int cgmres_hip_create(const cgmres_hip_config* cfg, cgmres_hip_handle* out);
int cgmres_hip_destroy(cgmres_hip_handle h);
int cgmres_hip_get_config(cgmres_hip_handle h, cgmres_hip_config* cfg);
/* Name of the mapping / kernel family the handle resolved to: "lane", "wave", "wg", "wg-lean", "wg+row-newton", "wg+row-scan",
 * "wg+parallel-costate", "wg+two-pass-costate", "wg-lean+two-pass-costate" (static
 * string; NULL on an invalid handle).  No counterpart in the reference: for logs and for tests that must know which
 * instantiation they exercised. */
const char* cgmres_hip_variant_name(cgmres_hip_handle h);

/* ---- setup: cgmres.hpp:36-76 --------------------------------------------------------------------- */
/* per_instance = 0: one vector broadcast to every instance; 1: [batch][...] */
int cgmres_hip_set_ptau(cgmres_hip_handle h, const void* ptau, int per_instance);         /* cgmres.hpp:36-39 */
int cgmres_hip_set_ptau_repeat(cgmres_hip_handle h, const void* p, int per_instance);     /* cgmres.hpp:41-49 */
int cgmres_hip_init_u0(cgmres_hip_handle h, const void* u0, int per_instance);            /* cgmres.hpp:51-59 */
/* Batched Newton on dH/du = 0 with the 3x3 / 6x6 partial-pivot solve (matrix.hpp:166-224), on the device.
 * u0 [batch][dim_u] in/out, x0 [batch][dim_x], p0 [batch][dim_p] (ignored when dim_p = 0).  cgmres.hpp:61-76 */
int cgmres_hip_init_u0_newton(cgmres_hip_handle h, void* u0, const void* x0, const void* p0, int32_t n_loop);

/* ---- the hot path: Cgmres::control, cgmres.hpp:78-110 -------------------------------------------- */
/* One tick for every instance: u [batch][dim_u] out, x [batch][dim_x] in.  Host pointers; blocks. */
int cgmres_hip_control(cgmres_hip_handle h, void* u, const void* x);
/* Same, device pointers, asynchronous on the handle's stream. */
int cgmres_hip_control_device(cgmres_hip_handle h, void* u_dev, const void* x_dev);
/* n_ticks of the example main loop (<example>/main.cpp:63-73) without leaving the GPU: control, then the
 * simulator's forward-Euler plant step x += dxdt(x,u)*dt.  x_dev in/out, u_dev = last tick's u.
 * Asynchronous on the handle's stream. */
int cgmres_hip_closed_loop_device(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks);
/* The same loop with a TIME-VARYING reference: before tick k (k = 0 .. n_ticks-1) the parameter horizon of every
 * instance is replaced by ptau_seq[k], i.e. what a caller of the reference does by calling set_ptau (cgmres.hpp:36-39)
 * before every control().  ptau_seq_dev is a device pointer: [n_ticks][batch][dim_p*(dv+1)] when per_instance = 1,
 * [n_ticks][dim_p*(dv+1)] (one horizon broadcast to all instances) when per_instance = 0.  The ticks stay fused
 * (CGMRES_HIP_TICKS_PER_LAUNCH per launch); after the call the handle keeps the last tick's ptau, as set_ptau would.
 * With dim_p = 0 the sequence is ignored.  Asynchronous on the handle's stream. */
int cgmres_hip_closed_loop_device_ptau(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks,
                                       const void* ptau_seq_dev, int per_instance);
/* The same loop (<example>/main.cpp:63-73) with a plant that is NOT the controller's nominal model run on the
 * controller's own state: a process disturbance d and a measurement noise v, both optional, per tick and per instance.
 * x_k is the TRUE plant state; x_dev holds x_0 on entry.  For tick k = 0 .. n_ticks-1 of one call
 *     y_k     = x_k + v_k                      (v absent: y_k = x_k)
 *     u_k     = control(y_k)                   (cgmres.hpp:78-110 unchanged: x_dxh etc. are built from y_k)
 *     x_{k+1} = (x_k + f(x_k, u_k)*dt) + d_k   (d absent: the expression of cgmres_hip_closed_loop_device; f = the
 *                                               model's dxdt at the TRUE state, with p of stage 0)
 * On return x_dev = x_n (true state) and u_dev = u_{n-1}; time, status, Krylov arrays, F_dxh_h / x_dxh are as after the
 * same ticks of cgmres_hip_closed_loop_device, the handle's ptau is the last tick's as after ..._ptau.
 * dist_seq_dev / meas_seq_dev are device arrays of the handle's dtype, [n_ticks][batch][dim_x] when the matching
 * *_per_instance is 1, [n_ticks][dim_x] (one vector broadcast to every instance) when it is 0, indexed by the caller's
 * instance index.  The library draws no random numbers: a Monte-Carlo study brings its own.  The ticks stay fused.
 * in == NULL or all three pointers NULL: exactly cgmres_hip_closed_loop_device; only ptau_seq_dev set: exactly
 * ..._ptau (with dim_p = 0 the ptau sequence is ignored).  n_ticks == 0 does nothing.  CGMRES_HIP_EINVAL: struct_size
 * other than sizeof(cgmres_hip_loop_inputs), a *_per_instance outside {0, 1}, n_ticks < 0, a dist / meas array whose
 * byte range overlaps x_dev or u_dev (the alias guard of cgmres_hip_control).  Asynchronous on the handle's stream. */
typedef struct cgmres_hip_loop_inputs {
  int32_t struct_size;        /* sizeof(cgmres_hip_loop_inputs); anything else: CGMRES_HIP_EINVAL */
  int32_t ptau_per_instance;  /* 0 / 1, as in cgmres_hip_closed_loop_device_ptau */
  int32_t dist_per_instance;  /* 0 / 1 */
  int32_t meas_per_instance;  /* 0 / 1 */
  const void* ptau_seq_dev;   /* NULL: the handle's ptau on every tick */
  const void* dist_seq_dev;   /* d: NULL = none */
  const void* meas_seq_dev;   /* v: NULL = none */
} cgmres_hip_loop_inputs;
int cgmres_hip_closed_loop_device_ex(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks,
                                     const cgmres_hip_loop_inputs* in);
/* ---- the predicted horizon and the optimality error: what F_func builds, cgmres.hpp:113-162 ----------------------- */
/* Evaluates F_func(ret, U, x, t) of the reference with the handle's CURRENT U, ptau and t (after a closed loop with a ptau
 * sequence: the last tick's ptau) at the caller's x_dev [batch][dim_x], and keeps what a tick throws away: the predicted
 * state trajectory xtau, the costate trajectory ltau, the optimality residual F and its norm, the health figure of
 * C/GMRES.  Scalars in the handle's dtype, device pointers, instance-major like every other vector.  A NULL output pointer
 * means that output is not wanted.  Stream-ordered on the handle's stream and asynchronous: no host copy, no synchronise,
 * so it follows a cgmres_hip_closed_loop_device on the stream.  It changes nothing a later tick reads (t, U, dUdt, x_dxh,
 * F_dxh_h, the Krylov arrays, the status).  Every mapping, both dtypes, every size cgmres_hip_create accepts.
 * CGMRES_HIP_EINVAL, each with its own text: x_dev NULL, out NULL, a struct_size other than
 * sizeof(cgmres_hip_horizon_out), a non-zero reserved, all four outputs NULL; a user model whose plugin was built before
 * this entry point existed (rebuild the plugin: everything else of it keeps working). */
typedef struct cgmres_hip_horizon_out {
  int32_t struct_size;   /* sizeof(cgmres_hip_horizon_out); anything else: CGMRES_HIP_EINVAL */
  int32_t reserved;      /* 0; anything else: CGMRES_HIP_EINVAL */
  void* xtau_dev;        /* [batch][dv+1][dim_x]  cgmres.hpp:132-140 */
  void* ltau_dev;        /* [batch][dv+1][dim_x]  cgmres.hpp:145-153 */
  void* F_dev;           /* [batch][dim_u*dv]     cgmres.hpp:156-161 */
  void* fnorm_dev;       /* [batch]               sqrt(sum_e F[e]^2), e ascending, accumulated in the handle's scalar type */
} cgmres_hip_horizon_out;
int cgmres_hip_horizon_device(cgmres_hip_handle h, const void* x_dev, const cgmres_hip_horizon_out* out);
/* ---- the ensemble of a batch and the record of a closed loop: the lines <example>/main.cpp:75-82 writes ------------- */
/* The statistics of ONE row of the batch: x_dev [batch][dim_x], u_dev [batch][dim_u] (the caller's, handle dtype) and the
 * status arrays the handle currently holds (what cgmres_hip_get_status would return).  Instance b COUNTS when all
 * dim_x + dim_u values of its row are finite.  Component c runs over x, then u; with z = double(value) - centre[c] over
 * the counting instances
 *     moments[c] = { s1 = sum z, s2 = sum z*z, min, max }    (min / max of the values themselves; no counting instance:
 *                                                              s1 = s2 = 0, min = +inf, max = -inf)
 * in double for fp32 handles too.  The caller forms mean = centre + s1/n and var = s2/n - (s1/n)^2: with the set point as
 * centre nothing cancels, which is why there is a centre.
 *     counts[0 .. k_max]             histogram of n_ax over ALL instances
 *     counts[k_max+1 .. k_max+5]     instances per CGMRES_HIP_EXIT_* code 0 .. 4, over ALL instances
 *     counts[k_max+6]                the counting instances (n above)
 * The sums use no floating-point atomics and a fixed order: two runs from the same state give the same bits.  Stream-
 * ordered on the handle's stream and asynchronous, changing nothing a later tick reads (the contract of
 * cgmres_hip_horizon_device).  Every mapping, both dtypes, built-in and user models (the kernel is the library's, independent
 * of the model: a plugin holds none of it).  CGMRES_HIP_EINVAL, each with its own text: x_dev or u_dev NULL, out NULL, a
 * struct_size other than sizeof(cgmres_hip_ensemble_out), a non-zero reserved, both outputs NULL, counts for
 * k_max + 7 > 8192; a user model whose plugin was built before this entry point existed (rebuild the plugin: everything
 * else of it keeps working). */
typedef struct cgmres_hip_ensemble_out {
  int32_t struct_size;      /* sizeof(cgmres_hip_ensemble_out); anything else: CGMRES_HIP_EINVAL */
  int32_t reserved;         /* 0; anything else: CGMRES_HIP_EINVAL */
  const double* centre_dev; /* [dim_x+dim_u] doubles, or NULL = zeros */
  double* moments_dev;      /* [dim_x+dim_u][4] = {s1, s2, min, max}, always double; NULL: not wanted */
  int32_t* counts_dev;      /* [k_max+7]; NULL: not wanted */
} cgmres_hip_ensemble_out;
int cgmres_hip_ensemble_device(cgmres_hip_handle h, const void* x_dev, const void* u_dev, const cgmres_hip_ensemble_out* out);
/* Instances one workgroup of the record kernel covers per grid step (a batch above it has several partials to combine:
 * what a test of the ensemble wants to know). */
#define CGMRES_HIP_RECORD_BLOCK 256
/* cgmres_hip_closed_loop_device_ex that RECORDS every stride-th tick: tick k (0-based within the call) is recorded iff
 * (k+1) % stride == 0, n_rec = n_ticks / stride records in all; ticks behind the last recorded one still run.  The phase
 * restarts with every call: a caller who chains calls uses multiples of the stride.  Record j (tick k = (j+1)*stride - 1)
 * is the reference's own output line (<example>/main.cpp:75-82), the state AFTER the plant step and the input that
 * produced it:
 *     x_log[j] = x_{k+1}   (under disturbance / noise inputs the TRUE state, disturbance included)
 *     u_log[j] = u_k
 *     n_ax_log[j], reason_log[j] = what cgmres_hip_get_status would return after tick k
 *     t_host[j] = the handle's time when tick k's control() ran, i.e. before t += dt (cgmres.hpp:107): main.cpp's first
 *                 column.  HOST memory, filled before the call returns.
 *     moments_log[j], counts_log[j] = cgmres_hip_ensemble_device of that row, with centre_dev
 * Every output pointer may be NULL.  rec == NULL, or all seven outputs NULL: exactly cgmres_hip_closed_loop_device_ex(h,
 * x_dev, u_dev, n_ticks, in), launch for launch.  The record is taken BETWEEN kernel launches, by a kernel of its own on
 * the same stream: the launches are cut so that every recorded tick is the last tick of one (cgmres_hip_record_plan), and
 * the loop is, launch for launch and bit for bit, the loop of a caller who calls ..._ex once per stride window and
 * downloads x, u and the status in between.  A stride that is a multiple of CGMRES_HIP_TICKS_PER_LAUNCH adds no launch
 * but the records'; below that the caller trades fusion for resolution.  n_ticks == 0 does nothing.  CGMRES_HIP_EINVAL,
 * each with its own text: everything ..._ex refuses; a struct_size other than sizeof(cgmres_hip_loop_record), a non-zero
 * reserved, stride < 1, x_dev or u_dev NULL, a device log whose byte range overlaps x_dev, u_dev, another log of the same
 * call or a sequence of `in`; a user model whose plugin was built before this entry point existed (rebuild the plugin).
 * Asynchronous on the handle's stream. */
typedef struct cgmres_hip_loop_record {
  int32_t struct_size;      /* sizeof(cgmres_hip_loop_record); anything else: CGMRES_HIP_EINVAL */
  int32_t stride;           /* >= 1 */
  int32_t reserved[2];      /* 0 */
  void* x_log_dev;          /* [n_rec][batch][dim_x], handle dtype */
  void* u_log_dev;          /* [n_rec][batch][dim_u] */
  int32_t* n_ax_log_dev;    /* [n_rec][batch] */
  int32_t* reason_log_dev;  /* [n_rec][batch] */
  double* t_host;           /* HOST memory [n_rec] */
  const double* centre_dev; /* as in cgmres_hip_ensemble_out */
  double* moments_log_dev;  /* [n_rec][dim_x+dim_u][4] */
  int32_t* counts_log_dev;  /* [n_rec][k_max+7] */
} cgmres_hip_loop_record;
int cgmres_hip_closed_loop_device_rec(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks,
                                      const cgmres_hip_loop_inputs* in, const cgmres_hip_loop_record* rec);
/* The launch cut of ..._rec on the mappings that fuse ticks: *n_rec = n_ticks / stride, *n_launches launches, their tick
 * counts in launch_ticks[0 .. *n_launches) (cap = its capacity; launch_ticks NULL: only the two numbers are wanted).  Each
 * stride window is cut exactly as a fresh call of `stride` ticks is cut (CGMRES_HIP_TICKS_PER_LAUNCH, ..., then the
 * remainder), the tail behind the last record as a fresh call of the remaining ticks.  n_rec / n_launches may be NULL.
 * CGMRES_HIP_EINVAL: n_ticks < 0, stride < 1, cap too small.  Pure host arithmetic: needs no GPU. */
int cgmres_hip_record_plan(int32_t n_ticks, int32_t stride, int32_t* n_rec, int32_t* launch_ticks, int32_t cap,
                           int32_t* n_launches);
/* ---- a closed loop against a plant of its own: parameters, RK4, substeps ----------------------------------------------- */
/* The plant of the loops above is the controller's own model with its compile-time constants, stepped by one forward-Euler
 * step of dt.  Here the plant is
 *     Phi(x, u; theta, p) = `substeps` steps of length dt/substeps of forward Euler or classical RK4 on the model's state
 *                           equation, u, p and theta held over the tick (zero-order hold), computed in the handle's dtype
 * theta: the constants the state equation reads, as run-time values (cgmres_hip_plant_info gives their number and the
 * nominal values, in this order):
 *     pendulum     7   As, Bs, A52, C22, A32a, A32, A32b      (arm_type_inverted_pendulum/model.hpp:80-98)
 *     MSD          6   m1, m2, d1, d2, k1, k2                 (mass_spring_damper/model.hpp; the (k1*k2) form of dxdt kept)
 *     semi-active  2   a, b                                   (semiactive_damper/model.hpp:85-86)
 * theta_dev is a device array of the handle's dtype, [batch][n_theta] (theta_per_instance = 1) or one row [n_theta]
 * broadcast to every instance (0); NULL = nominal (the model's own dxdt runs).  A user model has n_theta = 0: its plant is
 * its own dxdt(x, u, p), with p = stage 0 of the horizon the controller was given for that tick (row k of ptau_seq_dev
 * where a sequence is given, the handle's ptau otherwise).  The plant is a kernel of its own between the tick launches:
 * the loop runs ONE tick per launch, which is what this entry point costs against the fused loop. */
enum { CGMRES_HIP_PLANT_EULER = 0, CGMRES_HIP_PLANT_RK4 = 1 };
typedef struct cgmres_hip_loop_plant {
  int32_t struct_size;        /* sizeof(cgmres_hip_loop_plant); anything else: CGMRES_HIP_EINVAL */
  int32_t integrator;         /* CGMRES_HIP_PLANT_* */
  int32_t substeps;           /* 1 .. 4096 */
  int32_t theta_per_instance; /* 0 / 1 */
  const void* theta_dev;      /* handle's dtype; NULL = nominal */
  int32_t reserved[2];        /* 0 */
} cgmres_hip_loop_plant;
/* *n_theta = the number of plant parameters of a model (0 for a user model), nominal[0 .. n_theta) their nominal values
 * (nominal NULL: only the number is wanted; cap = its capacity).  CGMRES_HIP_EINVAL: an unknown model, cap < n_theta.
 * Pure host arithmetic: needs no GPU. */
int cgmres_hip_plant_info(int32_t model_id, int32_t* n_theta, double* nominal, int32_t cap);
/* One plant step on the stream: x_dev <- Phi(x_dev, u_dev), x_dev [batch][dim_x] in/out, u_dev [batch][dim_u]; no d, no v.
 * Changes no controller state; p (user models) is stage 0 of the handle's ptau.  CGMRES_HIP_EINVAL: what
 * ..._closed_loop_device_plant refuses of a plant, a NULL plant, x_dev or u_dev.  Asynchronous on the handle's stream. */
int cgmres_hip_plant_step_device(cgmres_hip_handle h, void* x_dev, const void* u_dev, const cgmres_hip_loop_plant* plant);
/* cgmres_hip_closed_loop_device_rec against this plant; `in` and `rec` as there.  For tick k = 0 .. n_ticks-1
 *     y_k     = x_k + v_k
 *     u_k     = control(y_k)              with ptau_k
 *     x_{k+1} = Phi(x_k, u_k) + d_k
 * x_dev always holds the TRUE state (y lives in a buffer of the handle); a record sees the true x_{k+1}.  After the call
 * the handle's time, U, dUdt, status and last ptau are as after ..._rec.  plant == NULL: exactly ..._rec.
 * CGMRES_HIP_EINVAL, each with its own text: everything ..._rec refuses; a struct_size other than
 * sizeof(cgmres_hip_loop_plant), a non-zero reserved, an unknown integrator, substeps outside 1 .. 4096, a
 * theta_per_instance outside {0, 1}, theta_dev on a model with n_theta == 0, theta_dev overlapping x_dev, u_dev, a log or
 * a sequence; a user model whose plugin was built before this entry point existed (rebuild the plugin).
 * Asynchronous on the handle's stream. */
int cgmres_hip_closed_loop_device_plant(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks,
                                        const cgmres_hip_loop_inputs* in, const cgmres_hip_loop_record* rec,
                                        const cgmres_hip_loop_plant* plant);
/* ---- a closed loop that previews a sampled reference signal ------------------------------------------------------------- */
/* The parameter horizon of a controller is ptau = [ p(t), p(t + dtau), ..., p(t + dv*dtau) ] (cgmres.hpp:37) with
 * dtau = get_dtau(t) (cgmres.hpp:32-34).  ptau_seq_dev takes it ready-made for every tick, [n_ticks][batch][dim_p*(dv+1)];
 * here the caller hands over the SIGNAL p, sampled on a uniform grid, and the loop forms every tick's ptau on the device
 * from the handle's own t and dtau, while the ticks stay fused.  sig_dev is a device array of the handle's dtype,
 * [batch][n_samples][dim_p] (sig_per_instance = 1; instance-major, so a shard is a contiguous slice) or one signal
 * [n_samples][dim_p] for every instance (0); sample j is p at time t0 + j*ts.  For the tick at the handle's time t_k, stage
 * i = 0 .. dv and component c, in double for fp32 handles too:
 *     tau = double(t_k) + i * double(dtau_k)                            dtau_k = get_dtau(t_k) in the handle's dtype
 *     s   = clamp((tau - t0) / ts, 0, n_samples - 1)
 *     CGMRES_HIP_PREVIEW_HOLD:    j = min(floor(s), n_samples-1);           p = sig[j][c]
 *     CGMRES_HIP_PREVIEW_LINEAR:  j = min(floor(s), max(n_samples-2, 0));   p = sig[j][c] + (s - j)*(sig[j+1][c] - sig[j][c])
 *                                                                           (n_samples == 1: p = sig[0][c])
 *     ptau_k[i*dim_p + c] = p, rounded to the handle's dtype
 * Before t0 the first sample holds, past the end the last.  The rows are written by a kernel of its own in front of every
 * launch, into a ring of CGMRES_HIP_TICKS_PER_LAUNCH rows the handle owns (allocated on first use, freed with the handle),
 * on the handle's stream. */
enum { CGMRES_HIP_PREVIEW_HOLD = 0, CGMRES_HIP_PREVIEW_LINEAR = 1 };
typedef struct cgmres_hip_loop_preview {
  int32_t struct_size;      /* sizeof(cgmres_hip_loop_preview); anything else: CGMRES_HIP_EINVAL */
  int32_t interp;           /* CGMRES_HIP_PREVIEW_* */
  int32_t sig_per_instance; /* 0 / 1 */
  int32_t n_samples;        /* >= 1 */
  double t0;                /* the time of sample 0; finite */
  double ts;                /* the sample period; finite, > 0 */
  const void* sig_dev;      /* handle's dtype; may be NULL when dim_p = 0 */
  int32_t reserved[2];      /* 0 */
} cgmres_hip_loop_preview;
/* cgmres_hip_closed_loop_device_plant with such a preview; `in`, `rec` and `plant` as there, each may be NULL.  Tick k runs
 * with the ptau_k above; a record's cut decides the launch sizes as without a preview, a plant of its own runs one tick per
 * launch and a user model's plant reads stage 0 of that tick's row.  After the call the handle keeps the last tick's row as
 * its ptau, exactly as after a ptau_seq_dev loop, and the loop is, bit for bit, the ptau_seq_dev loop over the rows
 * cgmres_hip_preview_device exports.  With dim_p = 0 the preview is ignored, as a ptau sequence is.  preview == NULL:
 * exactly ..._plant.  CGMRES_HIP_EINVAL, each with its own text: everything ..._plant refuses; a struct_size other than
 * sizeof(cgmres_hip_loop_preview), a non-zero reserved, interp or sig_per_instance outside its values, n_samples < 1, ts
 * not finite or <= 0, t0 not finite, sig_dev NULL on a model with dim_p > 0, in->ptau_seq_dev together with a preview,
 * sig_dev overlapping x_dev, u_dev, a log, a sequence or theta_dev; a user model whose plugin was built before this entry
 * point existed (rebuild the plugin).  Asynchronous on the handle's stream. */
int cgmres_hip_closed_loop_device_preview(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks,
                                          const cgmres_hip_loop_inputs* in, const cgmres_hip_loop_record* rec,
                                          const cgmres_hip_loop_plant* plant, const cgmres_hip_loop_preview* preview);
/* The rows that loop WOULD use for its next n_ticks ticks from the handle's current time: rows_dev
 * [n_ticks][batch][dim_p*(dv+1)], handle's dtype.  What a caller plots.  Stream-ordered on the handle's stream and
 * asynchronous; changes no state (not the time, not the handle's ptau).  dim_p = 0 or n_ticks = 0 writes nothing.
 * CGMRES_HIP_EINVAL: what ..._preview refuses of a preview, a NULL preview, rows_dev NULL, n_ticks < 0. */
int cgmres_hip_preview_device(cgmres_hip_handle h, const cgmres_hip_loop_preview* preview, int32_t n_ticks, void* rows_dev);
int cgmres_hip_synchronize(cgmres_hip_handle h);

/* ---- state: the private members of Cgmres (cgmres.hpp:195-202) and Gmres (gmres.hpp:120-124) ------ */
int cgmres_hip_get_time(cgmres_hip_handle h, double* t);
int cgmres_hip_get_state(cgmres_hip_handle h, double* t, void* U, void* dUdt); /* [batch][dim_u*dv]; NULL skips */
int cgmres_hip_set_state(cgmres_hip_handle h, double t, const void* U, const void* dUdt);
/* Device addresses of U and dUdt as the kernels keep them: [batch][*pitch] scalars, *pitch >= dim_u*dv; the words behind
 * dim_u*dv of a row are pads that no kernel reads or writes and get_state / set_state skip.  Valid while the handle
 * lives; synchronise before touching them.  Mappings that keep their state in another form return NULL addresses. */
int cgmres_hip_state_rows(cgmres_hip_handle h, void** U_dev, void** dUdt_dev, int32_t* pitch);
/* n_ax[b] = Arnoldi mat-vecs executed inside the k loop of the last solve, reason[b] = CGMRES_HIP_EXIT_* */
int cgmres_hip_get_status(cgmres_hip_handle h, int32_t* n_ax, int32_t* reason);
/* H [batch][(k_max+1)*(k_max+1)] column-major ld k_max+1 (gmres.hpp:12,54), rho [batch][k_max+1],
 * g [batch][3*k_max] (gmres.hpp:14), V [batch][(k_max+1)*len] column-major (gmres.hpp:11); NULL skips */
int cgmres_hip_get_krylov(cgmres_hip_handle h, void* V, void* H, void* rho, void* g);

/* ---- white-box hooks used by the parity tests (private methods of the reference) ------------------ */
/* F_func(ret, U, x, t), cgmres.hpp:113-162, with the handle's ptau.  All [batch][...], host pointers. */
int cgmres_hip_F_func(cgmres_hip_handle h, void* ret, const void* U, const void* x, double t);
/* The statements of control() before the solve (cgmres.hpp:83-96): leaves x_dxh, F_dxh_h in the handle and
 * returns the GMRES right-hand side b [batch][len]. */
int cgmres_hip_prepare(cgmres_hip_handle h, void* b, const void* x);
/* Ax_func(out, v), cgmres.hpp:164-175; needs cgmres_hip_prepare first. */
int cgmres_hip_Ax_func(cgmres_hip_handle h, void* out, const void* v);
/* Gmres::gmres(x, b), gmres.hpp:28-112; needs cgmres_hip_prepare first. x [batch][len] in/out. */
int cgmres_hip_gmres(cgmres_hip_handle h, void* x, const void* b);

/* ---- sharding a batch over the GPUs of one node ------------------------------------- */
/* Contiguous, balanced slice [*lo, *hi) of `n` controller instances for shard `rank` of `world` (the first n % world
 * shards get one more) — the rule cgmres_cpp_amd/sharding.py and include/cgmres_batch.hpp (CgmresBatchSharded) share.
 * The reference's multiple_controller/main.cpp:89-110 owns its controllers one by one; this is the bookkeeping of
 * owning `n` of them on `world` devices.  Pure host arithmetic: needs no GPU. */
int cgmres_hip_shard_bounds(int32_t n, int32_t world, int32_t rank, int32_t* lo, int32_t* hi);

/* ---- measurement ---------------------------------------------------------------------------------- */
/* HIP events on the handle's stream around whatever is enqueued between the two calls. */
int cgmres_hip_timer_start(cgmres_hip_handle h);
int cgmres_hip_timer_stop(cgmres_hip_handle h, float* elapsed_ms); /* synchronises the stream */
/* Device allocator for callers without a HIP runtime of their own (tests, bench via ctypes). */
int cgmres_hip_malloc(cgmres_hip_handle h, void** dev_ptr, uint64_t bytes);
int cgmres_hip_free(cgmres_hip_handle h, void* dev_ptr);
int cgmres_hip_memcpy_h2d(cgmres_hip_handle h, void* dev_dst, const void* host_src, uint64_t bytes);
int cgmres_hip_memcpy_d2h(cgmres_hip_handle h, void* host_dst, const void* dev_src, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* CGMRES_HIP_H_ */
