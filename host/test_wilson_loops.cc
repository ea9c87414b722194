// test_wilson_loops.cc -- the host arithmetic on Wilson loops (include/mlmcpi/correlator.hh, WilsonLoops of include/mlmcpi/qoi.hh): the
// exact series of the periodic lattice (printed for tests/test_wilson_loops_host.py, which compares it with its own long-double series),
// its limits, the Creutz ratio of a pure area law, and the chain-spread error and the jackknife on constructed inputs.  No device is
// touched.  Prints one line per check; exit status 1 on a failure.
#include <cstdio>

#include "mlmcpi/qoi.hh"

using namespace mlmcpi;

static int failures = 0;

static void expect(bool ok, const char *what, double got, double want) {
  std::printf("%s %s: got %.17g want %.17g\n", ok ? "ok  " : "FAIL", what, got, want);
  if (!ok) ++failures;
}

int main() {
  const double betas[3] = {0.5, 2.0, 10.0};
  const unsigned Ms[2] = {4, 64};
  for (double beta : betas)
    for (unsigned M : Ms) {
      for (unsigned r = 1; r <= 4; ++r)
        for (unsigned s = 1; s <= 4; ++s) std::printf("exact %.17g %u %u %u %u %.17g\n", beta, M, M, r, s, wilson_loop_exact(beta, M, M, r, s));
      const double full = wilson_loop_exact(beta, M, M, M, M);
      expect(std::fabs(full - 1.0) <= 1e-14, "the loop around the whole lattice is 1", full, 1.0);
    }
  for (double beta : betas) {
    const double sigma = string_tension_exact(beta), w = wilson_loop_exact(beta, 64, 64, 2, 3), area = std::exp(-6.0 * sigma);
    expect(std::fabs(w - area) <= 1e-13 * area, "64 x 64: W(2, 3) is the area law of the infinite lattice", w, area);
    // a pure area law W = exp(-sigma r s): every Creutz ratio is sigma
    const unsigned R = 5, S = 4;
    std::vector<double> W(R * S);
    for (unsigned r = 1; r <= R; ++r)
      for (unsigned s = 1; s <= S; ++s) W[(r - 1) * S + s - 1] = std::exp(-sigma * r * s);
    double worst = 0.0;
    for (unsigned r = 1; r <= R; ++r)
      for (unsigned s = 1; s <= S; ++s) worst = std::max(worst, std::fabs(creutz_ratio(W, R, S, r, s) - sigma));
    expect(worst <= 1e-13 * (1.0 + sigma), "Creutz ratio of a pure area law at every (r, s), worst deviation from sigma", worst, 0.0);
  }
  expect(std::isnan(creutz_ratio({0.5, -0.1}, 1, 2, 1, 2)), "NaN where the ratio is not positive", creutz_ratio({0.5, -0.1}, 1, 2, 1, 2), NAN);
  // chi(1, 1) = -log W(1, 1)
  expect(creutz_ratio({0.25}, 1, 1, 1, 1) == -std::log(0.25), "chi(1, 1) = -log W(1, 1)", creutz_ratio({0.25}, 1, 1, 1, 1), -std::log(0.25));
  // four chains whose W(1, 1) means are 0.5, 0.6, 0.7, 0.8 (printed for the Python side, which redoes the jackknife)
  const std::vector<std::vector<double>> m = {{0.5}, {0.6}, {0.7}, {0.8}};
  const WilsonLoops::Ratio c = WilsonLoops::creutz_jackknife(m, 1, 1, 1, 1);
  std::printf("jackknife %.17g %.17g %d\n", c.value, c.error, (int)c.has_error);
  expect(std::fabs(c.value + std::log(0.65)) <= 1e-15, "jackknife: the value is that of the mean over chains", c.value, -std::log(0.65));
  const WilsonLoops::Ratio one = WilsonLoops::creutz_jackknife({{0.5}}, 1, 1, 1, 1);
  expect(!one.has_error && one.error == 0.0, "one chain: no jackknife error", one.error, 0.0);
  // sums of 2 samples of those chains: W = mean -+ 0.1, so sum W = 2 mean, sum W^2 = 2 mean^2 + 0.02
  std::vector<double> a;
  for (const auto &row : m) {
    a.push_back(2.0 * row[0]);
    a.push_back(2.0 * row[0] * row[0] + 0.02);
  }
  const WilsonLoops::Estimate e = WilsonLoops::wilson_loops_estimate(a, 4, 1, 2);
  const double spread = std::sqrt((0.15 * 0.15 + 0.05 * 0.05) * 2.0 / 12.0);
  expect(e.chain_spread && std::fabs(e.mean[0] - 0.65) <= 1e-15 && std::fabs(e.error[0] - spread) <= 1e-15,
         "four chains: the error is the spread of the per-chain means", e.error[0], spread);
  const WilsonLoops::Estimate e1 = WilsonLoops::wilson_loops_estimate({a[0], a[1]}, 1, 1, 2);
  expect(!e1.chain_spread && std::fabs(e1.error[0] - 0.1) <= 1e-14, "one chain: the naive error of its samples", e1.error[0], 0.1);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
