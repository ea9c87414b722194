// test_gff_correlator.cc -- the host arithmetic on the GFF slice correlators (include/mlmcpi/correlator.hh, GffCorrelator of
// include/mlmcpi/qoi.hh): the mode sum against the closed cosh form and the dispersion relation (printed for
// tests/test_gff_correlator_host.py, which compares them with its own long-double values), the effective mass of the exact law, and
// the chain-spread error and the jackknife of E_q on constructed inputs.  No device is touched.  Prints one line per check; exit
// status 1 on a failure.
#include <cstdio>

#include "mlmcpi/qoi.hh"

using namespace mlmcpi;

static int failures = 0;

static void expect(bool ok, const char *what, double got, double want) {
  std::printf("%s %s: got %.17g want %.17g\n", ok ? "ok  " : "FAIL", what, got, want);
  if (!ok) ++failures;
}

int main() {
  const unsigned shapes[2][2] = {{16, 16}, {64, 32}};
  const double masses[2] = {1.0, 8.0};
  for (const auto &sh : shapes)
    for (double mass : masses) {
      const unsigned Mt = sh[0], Mx = sh[1];
      // A mode sum of terms of the size of C(0) carries an absolute error of a few ulp of C(0): 1e-13 C(0) here.  At q = 0 (E Mt / 2
      // <= 4 on these shapes) that is 1e-13 of C(tau) itself; at q > 0 the law falls by up to e^(-E Mt / 2) = 1e-8 across the lags
      // and the deviation is taken relative to C(0; q).
      double worst = 0.0, worst_abs = 0.0, worst_mass = 0.0;
      for (unsigned q = 0; q < 4; ++q) {
        const double E = gff_dispersion_exact(Mt, Mx, mass, q);
        std::printf("dispersion %u %u %.17g %u %.17g\n", Mt, Mx, mass, q, E);
        std::vector<double> C(Mt / 2 + 1);
        for (unsigned tau = 0; tau <= Mt / 2; ++tau) {
          C[tau] = gff_correlator_exact(Mt, Mx, mass, q, tau);
          std::printf("exact %u %u %.17g %u %u %.17g\n", Mt, Mx, mass, q, tau, C[tau]);
          const double closed = std::cosh(E * (0.5 * Mt - tau)) / (2.0 * std::sinh(E) * std::sinh(0.5 * E * Mt));
          if (q == 0) worst = std::max(worst, std::fabs(C[tau] / closed - 1.0));
          worst_abs = std::max(worst_abs, std::fabs(C[tau] - closed) / C[0]);
        }
        // effective_mass is acosh(r), r = (C(tau - 1) + C(tau + 1)) / (2 C(tau)) = cosh E_q for the exact law: three values of relative
        // error 1e-13 C(0) / C(tau + 1) at the most move r by 3 r times that, and acosh by that over sinh E_q
        for (unsigned tau = 1; tau < Mt / 2; ++tau) {
          const double tol = 3e-13 * (C[0] / C[tau + 1]) * std::cosh(E) / std::sinh(E), got = effective_mass(C, tau);
          worst_mass = std::isnan(got) ? INFINITY : std::max(worst_mass, std::fabs(got - E) / tol);
        }
      }
      expect(worst <= 1e-13, "q = 0: the mode sum is the closed cosh form, worst relative deviation", worst, 0.0);
      expect(worst_abs <= 1e-13, "q < 4: the mode sum is the closed cosh form, worst deviation relative to C(0; q)", worst_abs, 0.0);
      expect(worst_mass <= 1.0, "the effective mass of the exact law is E_q at every lag, worst deviation over its tolerance", worst_mass, 0.0);
    }
  // q = 0, tau summed with the correlator weights: sum_tau w C_t(tau; 0) = 1 / mu^2, the zero mode alone
  {
    const unsigned M = 16;
    const double mass = 4.0, mu2 = (mass / M) * (mass / M);
    double s = 0.0;
    for (unsigned tau = 0; tau <= M / 2; ++tau) s += correlator_weight(tau, M) * gff_correlator_exact(M, M, mass, 0, tau);
    expect(std::fabs(s * mu2 - 1.0) <= 1e-13, "sum_tau w C_t(tau; 0) = 1 / mu^2", s, 1.0 / mu2);
  }
  // index of C_d(tau; q) in a vector of n_out entries
  expect(GffCorrelator::index(8, 6, 3, 0, 2, 4) == 14 && GffCorrelator::index(8, 6, 3, 1, 0, 0) == 15 && GffCorrelator::index(8, 6, 3, 1, 2, 3) == 26,
         "index: C_t first, momentum-major, lag fastest", GffCorrelator::index(8, 6, 3, 1, 2, 3), 26);
  // four chains on (4, 4), P = 1, whose C_t(tau; 0) is a_b cosh(E (2 - tau)) with a_b = 1, 2, 3, 4 and E = 0.7 (C_x: zeros but C_x(1) = 1)
  const double E = 0.7;
  std::vector<std::vector<double>> m;
  for (unsigned b = 0; b < 4; ++b) {
    std::vector<double> row(6, 0.0);
    for (unsigned tau = 0; tau <= 2; ++tau) row[tau] = (b + 1.0) * std::cosh(E * (2.0 - tau));
    row[4] = 1.0;
    m.push_back(row);
  }
  const GffCorrelator::Energy en = GffCorrelator::energy_jackknife(m, 4, 4, 1, 0, 0, 1);
  expect(en.has_error && std::fabs(en.value - E) <= 1e-14 && en.error <= 1e-14, "jackknife: chains that differ by a factor agree on E", en.value, E);
  // chains that differ in shape: printed for the Python side, which redoes the jackknife
  std::vector<std::vector<double>> n = m;
  for (unsigned b = 0; b < 4; ++b) n[b][1] *= 1.0 - 0.05 * b;
  const GffCorrelator::Energy en2 = GffCorrelator::energy_jackknife(n, 4, 4, 1, 0, 0, 1);
  std::printf("jackknife %.17g %.17g %d\n", en2.value, en2.error, (int)en2.has_error);
  const GffCorrelator::Energy one = GffCorrelator::energy_jackknife({m[0]}, 4, 4, 1, 0, 0, 1);
  expect(!one.has_error && one.error == 0.0, "one chain: no jackknife error", one.error, 0.0);
  const GffCorrelator::Energy nan = GffCorrelator::energy_jackknife(m, 4, 4, 1, 1, 0, 1);
  expect(std::isnan(nan.value), "NaN where the triple is not convex", nan.value, NAN);
  // sums of 2 samples of chains with means 0.5 .. 0.8 -+ 0.1: sum C = 2 mean, sum C^2 = 2 mean^2 + 0.02
  std::vector<double> a;
  for (double mean : {0.5, 0.6, 0.7, 0.8}) {
    a.push_back(2.0 * mean);
    a.push_back(2.0 * mean * mean + 0.02);
  }
  const GffCorrelator::Estimate e = GffCorrelator::estimate(a, 4, 1, 2);
  const double spread = std::sqrt((0.15 * 0.15 + 0.05 * 0.05) * 2.0 / 12.0);
  expect(e.chain_spread && std::fabs(e.mean[0] - 0.65) <= 1e-15 && std::fabs(e.error[0] - spread) <= 1e-15,
         "four chains: the error is the spread of the per-chain means", e.error[0], spread);
  const GffCorrelator::Estimate e1 = GffCorrelator::estimate({a[0], a[1]}, 1, 1, 2);
  expect(!e1.chain_spread && std::fabs(e1.error[0] - 0.1) <= 1e-14, "one chain: the naive error of its samples", e1.error[0], 0.1);
  const std::vector<std::vector<double>> cm = GffCorrelator::chain_means_of(a, 4, 1, 2);
  expect(cm.size() == 4 && std::fabs(cm[3][0] - 0.8) <= 1e-16, "per-chain means are the sums over the number of samples", cm[3][0], 0.8);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
