// test_flow_scale.cc -- the reference scale of the gradient flow, flow_scale of include/mlmcpi/correlator.hh: the linear
// interpolation of the flow time at which t <E> / n = c, its NaN where c is not bracketed, and its jackknife error over chains
// through chain_estimate.hh.  No device, no library.  Prints one line per check; exit status 1 on a failure
// (tests/test_sigma_flow_driver.py runs it and redoes the numbers in numpy).
#include <cmath>
#include <cstdio>

#include "mlmcpi/chain_estimate.hh"
#include "mlmcpi/correlator.hh"

using namespace mlmcpi;

static int failures = 0;

static void expect(bool ok, const char *what, double got, double want) {
  std::printf("%s %s: got %.17g want %.17g\n", ok ? "ok  " : "FAIL", what, got, want);
  if (!ok) ++failures;
}

int main() {
  const std::vector<double> t = {0.0, 0.5, 1.0, 2.0}, y = {0.0, 0.02, 0.05, 0.07};
  expect(std::fabs(flow_scale(t, y, 0.035) - 0.75) < 1e-15, "between two times", flow_scale(t, y, 0.035), 0.75);
  expect(flow_scale(t, y, 0.05) == 1.0, "at a listed time", flow_scale(t, y, 0.05), 1.0);
  expect(flow_scale(t, y, 0.0) == 0.0, "at the first time", flow_scale(t, y, 0.0), 0.0);
  expect(std::fabs(flow_scale(t, y, 0.06) - 1.5) < 1e-15, "in the last interval", flow_scale(t, y, 0.06), 1.5);
  expect(std::isnan(flow_scale(t, y, 0.1)), "above every value: NaN", flow_scale(t, y, 0.1), NAN);
  expect(std::isnan(flow_scale(t, y, -0.01)), "below every value: NaN", flow_scale(t, y, -0.01), NAN);
  expect(std::isnan(flow_scale({1.0}, {0.05}, 0.05)), "one time: NaN", flow_scale({1.0}, {0.05}, 0.05), NAN);
  expect(std::isnan(flow_scale({}, {}, 0.05)), "no times: NaN", flow_scale({}, {}, 0.05), NAN);
  const std::vector<double> down = {0.09, 0.05, 0.01};
  expect(std::fabs(flow_scale({0.0, 1.0, 2.0}, down, 0.03) - 1.5) < 1e-15, "a falling curve", flow_scale({0.0, 1.0, 2.0}, down, 0.03), 1.5);
  // the first bracketing pair wins
  const std::vector<double> bump = {0.0, 0.04, 0.02, 0.06};
  expect(std::fabs(flow_scale({0.0, 1.0, 2.0, 3.0}, bump, 0.03) - 0.75) < 1e-15, "the first crossing", flow_scale({0.0, 1.0, 2.0, 3.0}, bump, 0.03), 0.75);

  // jackknife over three chains whose curves are y scaled by 0.9, 1.0, 1.1: printed for the numpy restatement
  std::vector<std::vector<double>> m;
  for (double f : {0.9, 1.0, 1.1}) {
    std::vector<double> c;
    for (double v : y) c.push_back(f * v);
    m.push_back(c);
  }
  const ChainScalar s = chain_jackknife(m, [&](const std::vector<double> &v) { return flow_scale(t, v, 0.035); });
  std::printf("jackknife flow_scale %.17g %.17g %d\n", s.value, s.error, (int)s.has_error);
  expect(s.has_error && std::fabs(s.value - 0.75) < 1e-15 && s.error > 0.0, "jackknife over chains", s.value, 0.75);
  std::printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
