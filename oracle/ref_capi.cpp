// ORACLE — TEST INFRASTRUCTURE ONLY. extern "C" entry points of oracle/_ref/libref.so:
// dispatches orc_create / orc_create_tuned to the fp64 / fp32 builds of oracle/ref_harness.cpp.
#define ORC_DEFINE_CAPI
#include "orc_base.hpp"

OrcBase* ref_make_f64(int model, int dv, int km, double tol, const double* tun);
OrcBase* ref_make_f32(int model, int dv, int km, double tol, const double* tun);

OrcBase* orc_factory(int model, int dv, int kmax, double tol, int dtype, const double* tun) {
  return dtype == 1 ? ref_make_f32(model, dv, kmax, tol, tun) : ref_make_f64(model, dv, kmax, tol, tun);
}
