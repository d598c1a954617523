// Host check that the row-form operators of gmres_row_ops.hpp ARE the serial operators of gmres_ops.hpp: for every twin
// and the scenario vectors of tests/test_user_gmres.py (b and the warm start x0 of instances 0..11), Ax_row(i, x, p)
// equals element i of Ax(., x, p) bit for bit.  Prints one line per twin and returns the number of mismatches.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "gmres_ops.hpp"
#include "gmres_row_ops.hpp"

template <class Serial, class Row>
int twins(const char* name, bool spd) {
  static_assert(Serial::len == Row::len && Serial::n_params == Row::n_params, "twins of different shapes");
  constexpr int L = Serial::len;
  static double x[L], ax[L];
  int bad = 0;
  for (int i = 0; i < 12; ++i)
    for (int which = 0; which < 2; ++which) {
      const double p[2] = {spd ? 0.3 + 0.11 * i : 0.4 + 0.07 * i, spd ? 0.0 : 0.35 - 0.02 * i};
      for (int e = 0; e < L; ++e) x[e] = which ? 0.01 * (e - i) : std::sin(0.3 * e + 0.5 * i) + 0.1 * e;
      Serial::Ax(ax, x, p);
      for (int e = 0; e < L; ++e) {
        const double r = Row::Ax_row(e, x, p);
        bad += std::memcmp(&r, &ax[e], sizeof r) != 0;
      }
    }
  printf("%s len %d mismatches %d\n", name, L, bad);
  return bad;
}

template <int N>
struct SerialOfRowN {  // the serial member of a both-forms struct, as an operator of its own
  static constexpr int len = N, n_params = 2;
  static void Ax(double* Ax, const double* x, const double* p) { ConvDiffRowOpN<N>::Ax(Ax, x, p); }
};

int main() {
  int bad = 0;
  bad += twins<SpdTridiagOp, SpdTridiagRowOp>("spd", true);
  bad += twins<ConvDiffOp, ConvDiffRowOp>("convdiff", false);
  bad += twins<ConvDiffOp150, ConvDiffRowOp150>("convdiff150", false);
  bad += twins<ConvDiffOp300, ConvDiffRowOp300>("convdiff300", false);
  bad += twins<ConvDiffOpN<1>, ConvDiffRowOp1>("convdiff1", false);
  bad += twins<ConvDiffOpN<64>, ConvDiffRowOp64>("convdiff64", false);
  bad += twins<ConvDiffOpN<65>, ConvDiffRowOp65>("convdiff65", false);
  bad += twins<ConvDiffOpN<840>, ConvDiffRowOp840>("convdiff840", false);
  bad += twins<SerialOfRowN<300>, ConvDiffRowOp300>("convdiff300 (its own Ax)", false);
  return bad ? 1 : 0;
}
