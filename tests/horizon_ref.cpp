// TEST INFRASTRUCTURE: an independent statement of what cgmres_hip_horizon_device returns.  The oracle's C ABI exposes F
// but not the two trajectories it builds on the way, so this file restates the two recurrences of
// oracle/cgmres_oracle.hpp::F (:104-124 = cgmres.hpp:132-161) over a Model class with the reference's static signatures
// and hands out xtau, ltau and F.  tests/test_horizon_ref.py pins its F bit for bit to the oracle's.
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<repo> tests/horizon_ref.cpp -o libhorizon_ref.so
// serves oracle::Pendulum / MassSpringDamper / SemiactiveDamper (model 0 / 1 / 2) in double and float; with
//   -DMODEL_HEADER='"tests/user_models/vdp_model.hpp"' -DMODEL_CLASS=VdpModel
// it serves that user model in double (model and f32 are ignored).  All arrays cross the boundary as double.
#include <cmath>
#include <vector>

#ifdef MODEL_HEADER
#include MODEL_HEADER
#else
#include "oracle/models.hpp"
#endif

template <class Model, class T>
static int horizon(int dv, double Tf, double alpha, double t_in, const double* x_in, const double* U_in, const double* p_in,
                   double* xtau, double* ltau, double* F) {
  constexpr int nx = Model::dim_x, nu = Model::dim_u, np = Model::dim_p;
  std::vector<T> X(nx * (dv + 1)), Lm(nx * (dv + 1)), U(nu * dv), P(np * (dv + 1) + 1, T(0)), ret(nu * dv);
  for (int i = 0; i < nu * dv; ++i) U[i] = T(U_in[i]);
  for (int i = 0; i < np * (dv + 1); ++i) P[i] = T(p_in[i]);
  const T t = T(t_in);
  const T dtau = T(Tf) * (1 - std::exp(-T(alpha) * t)) / T(dv);  // cgmres.hpp:32-34
  for (int i = 0; i < nx; ++i) X[i] = T(x_in[i]);               // :132
  for (int s = 0; s < dv; ++s) {                                // :133-140
    T* nxt = &X[nx * (s + 1)];
    Model::dxdt(nxt, &X[nx * s], &U[nu * s], &P[np * s]);
    for (int i = 0; i < nx; ++i) nxt[i] = nxt[i] * dtau;
    for (int i = 0; i < nx; ++i) nxt[i] = nxt[i] + X[nx * s + i];
  }
  Model::dPhidx(&Lm[nx * dv], &X[nx * dv], &P[np * dv]);  // :145
  for (int s = dv - 1; s >= 0; --s) {                     // :146-153
    T* cur = &Lm[nx * s];
    Model::dHdx(cur, &X[nx * s], &U[nu * s], &P[np * s], &Lm[nx * (s + 1)]);
    for (int i = 0; i < nx; ++i) cur[i] = cur[i] * dtau;
    for (int i = 0; i < nx; ++i) cur[i] = cur[i] + Lm[nx * (s + 1) + i];
  }
  for (int s = 0; s < dv; ++s)  // :156-161
    Model::dHdu(&ret[nu * s], &X[nx * s], &U[nu * s], &P[np * s], &Lm[nx * (s + 1)]);
  for (int i = 0; i < nx * (dv + 1); ++i) xtau[i] = double(X[i]), ltau[i] = double(Lm[i]);
  for (int i = 0; i < nu * dv; ++i) F[i] = double(ret[i]);
  return 0;
}

// x [dim_x], U [dim_u*dv], ptau [dim_p*(dv+1)] -> xtau, ltau [(dv+1)*dim_x], F [dim_u*dv]; -1 for an unknown model
extern "C" int horizon_ref(int model, int f32, int dv, double Tf, double alpha, double t, const double* x, const double* U,
                           const double* ptau, double* xtau, double* ltau, double* F) {
#ifdef MODEL_HEADER
  return horizon<MODEL_CLASS, double>(dv, Tf, alpha, t, x, U, ptau, xtau, ltau, F);
#else
#define HORIZON_OF(M) \
  return f32 ? horizon<oracle::M<float>, float>(dv, Tf, alpha, t, x, U, ptau, xtau, ltau, F) \
             : horizon<oracle::M<double>, double>(dv, Tf, alpha, t, x, U, ptau, xtau, ltau, F)
  if (model == 0) HORIZON_OF(Pendulum);
  if (model == 1) HORIZON_OF(MassSpringDamper);
  if (model == 2) HORIZON_OF(SemiactiveDamper);
  return -1;
#endif
}
