// test_path_correlator.cc -- the host arithmetic on the time correlator of a 1-D path (include/mlmcpi/correlator.hh): the effective
// mass on the exact lattice correlator of the harmonic oscillator, its NaN on a triple that is not convex, and the closed form at
// lag 0 against the action's analytic <x^2>.  No device is touched.  Prints one line per check; exit status 1 on a failure.
#include <cstdio>

#include "mlmcpi/action.hh"
#include "mlmcpi/correlator.hh"

using namespace mlmcpi;

static int failures = 0;

static void expect(bool ok, const char *what, double got, double want) {
  std::printf("%s %s: got %.17g want %.17g\n", ok ? "ok  " : "FAIL", what, got, want);
  if (!ok) ++failures;
}

int main() {
  // (M, a^2 mu2): T_final = 4, mu2 from the pair
  const unsigned Ms[2] = {16, 128};
  const double a2mu2[2] = {1.0 / 16.0, 1e-3};
  for (int c = 0; c < 2; ++c) {
    const unsigned M = Ms[c];
    const double T_final = 4.0, a = T_final / M, mu2 = a2mu2[c] / (a * a), m0 = 1.3;
    const double w = path_ho_lattice_omega(M, T_final, mu2);
    expect(std::fabs(std::cosh(w) - (1.0 + 0.5 * a2mu2[c])) <= 1e-15, "cosh(omega~) = 1 + a^2 mu2 / 2", std::cosh(w), 1.0 + 0.5 * a2mu2[c]);
    std::vector<double> C(M / 2 + 1);
    for (unsigned tau = 0; tau <= M / 2; ++tau) C[tau] = path_correlator_ho_exact(M, T_final, m0, mu2, tau);
    double worst = 0.0;
    for (unsigned tau = 1; tau < M / 2; ++tau) worst = std::max(worst, std::fabs(effective_mass(C, tau) - w));
    expect(worst <= 1e-12, "effective mass of the exact correlator at every interior lag, worst deviation", worst, 0.0);
    auto lat = std::make_shared<Lattice1D>(M, T_final);
    HarmonicOscillatorAction act(lat, RenormalisationNone, m0, mu2);
    const double x2 = act.Xsquared_analytical();
    expect(std::fabs(C[0] - x2) <= 1e-13 * x2, "closed form at lag 0 = the action's analytic <x^2>", C[0], x2);
  }
  const double nan1 = effective_mass({1.0, 1.0, 0.9}, 1), nan2 = effective_mass({0.5, 1.0, 0.7}, 1);
  expect(std::isnan(nan1) && std::isnan(nan2), "NaN on a triple that is not convex", nan1, NAN);
  expect(effective_mass({1.0, 1.0, 1.0}, 1) == 0.0, "zero mass on a flat triple", effective_mass({1.0, 1.0, 1.0}, 1), 0.0);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
