// test_chain_estimate.cc -- the host arithmetic every measurement beside the QoI shares (include/mlmcpi/chain_estimate.hh): the
// per-chain means, the chain-spread and the naive error, and the jackknife over chains with each of the four functions the classes
// of include/mlmcpi/qoi.hh hand it (printed for tests/test_chain_estimate_host.py, which redoes them in numpy).  No device is
// touched.  Prints one line per check; exit status 1 on a failure.
//   test_chain_estimate statics   prints, as hexadecimal floats, what the static entry points of WilsonLoops and GffCorrelator
//                                 give on a fixed pseudo-random input; tests/golden/chain_estimate_statics.txt is that text from
//                                 the classes as they were before they shared chain_estimate.hh, and it must not change
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mlmcpi/qoi.hh"

using namespace mlmcpi;

static int failures = 0;

static void expect(bool ok, const char *what, double got, double want) {
  std::printf("%s %s: got %.17g want %.17g\n", ok ? "ok  " : "FAIL", what, got, want);
  if (!ok) ++failures;
}

static void print_jackknife(const char *name, const ChainScalar &s) {
  std::printf("jackknife %s %.17g %.17g %d\n", name, s.value, s.error, (int)s.has_error);
}

// 5 chains, 7 entries, 3 samples from a 64-bit linear congruential generator (Knuth's MMIX constants), each entry scattered by
// 10 % about a convex profile so that no effective mass is NaN
static void print_statics() {
  const unsigned B = 5, n_out = 7, n_calls = 3;
  const double base[7] = {1.0, 0.6, 0.5, 1.0, 0.55, 0.35, 0.3};
  uint64_t state = 2481317;
  std::vector<double> a(2 * B * n_out, 0.0);
  for (unsigned b = 0; b < B; ++b)
    for (unsigned k = 0; k < n_out; ++k)
      for (unsigned i = 0; i < n_calls; ++i) {
        state = state * 6364136223846793005ULL + 1442695040888963407ULL;
        const double x = base[k] * (0.9 + 0.2 * ((double)(state >> 11) * 0x1p-53));
        a[2 * (b * n_out + k)] += x;
        a[2 * (b * n_out + k) + 1] += x * x;
      }
  for (unsigned chains : {B, 1u}) {
    const WilsonLoops::Estimate w = WilsonLoops::wilson_loops_estimate(a, chains, n_out, n_calls);
    const GffCorrelator::Estimate g = GffCorrelator::estimate(a, chains, n_out, n_calls);
    for (unsigned k = 0; k < n_out; ++k)
      std::printf("estimate %u %u %a %a %a %a %d %d\n", chains, k, w.mean[k], w.error[k], g.mean[k], g.error[k], (int)w.chain_spread, (int)g.chain_spread);
    const std::vector<std::vector<double>> m = GffCorrelator::chain_means_of(a, chains, n_out, n_calls);
    for (unsigned b = 0; b < chains; ++b)
      for (unsigned k = 0; k < n_out; ++k) std::printf("chain_mean %u %u %u %a\n", chains, b, k, m[b][k]);
    const unsigned loops[4][2] = {{7, 1}, {1, 7}, {2, 3}, {3, 2}};
    for (const auto &l : loops)
      for (unsigned r = 1; r <= l[0]; ++r)
        for (unsigned s = 1; s <= l[1]; ++s) {
          const WilsonLoops::Ratio c = WilsonLoops::creutz_jackknife(m, l[0], l[1], r, s);
          std::printf("creutz %u %u %u %u %u %a %a %d\n", chains, l[0], l[1], r, s, c.value, c.error, (int)c.has_error);
        }
    // Mt = 4, Mx = 6, P = 1: C_t(0 .. 2; 0) then C_x(0 .. 3; 0)
    const unsigned slices[3][2] = {{0, 1}, {1, 1}, {1, 2}};
    for (const auto &s : slices) {
      const GffCorrelator::Energy en = GffCorrelator::energy_jackknife(m, 4, 6, 1, (int)s[0], 0, s[1]);
      std::printf("energy %u %u %u %a %a %d\n", chains, s[0], s[1], en.value, en.error, (int)en.has_error);
    }
  }
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "statics")) {
    print_statics();
    return 0;
  }
  // sums of 2 samples of chains with means 0.5 .. 0.8 -+ 0.1: sum = 2 mean, sum of squares = 2 mean^2 + 0.02
  std::vector<double> a;
  for (double mean : {0.5, 0.6, 0.7, 0.8}) {
    a.push_back(2.0 * mean);
    a.push_back(2.0 * mean * mean + 0.02);
  }
  const ChainEstimate e = chain_estimate(a, 4, 1, 2);
  const double spread = std::sqrt((0.15 * 0.15 + 0.05 * 0.05) * 2.0 / 12.0);
  expect(e.chain_spread && std::fabs(e.mean[0] - 0.65) <= 1e-15 && std::fabs(e.error[0] - spread) <= 1e-15,
         "four chains: the error is the spread of the per-chain means", e.error[0], spread);
  const ChainEstimate e1 = chain_estimate({a[0], a[1]}, 1, 1, 2);
  expect(!e1.chain_spread && std::fabs(e1.mean[0] - 0.5) <= 1e-16 && std::fabs(e1.error[0] - 0.1) <= 1e-14,
         "one chain: the naive error of its samples", e1.error[0], 0.1);
  const ChainEstimate e0 = chain_estimate({0.5, 0.25}, 1, 1, 1);
  expect(!e0.chain_spread && e0.mean[0] == 0.5 && e0.error[0] == 0.0, "one chain, one sample: no variance, error 0", e0.error[0], 0.0);
  const std::vector<std::vector<double>> cm = chain_means_of(a, 4, 1, 2);
  expect(cm.size() == 4 && cm[0].size() == 1 && std::fabs(cm[3][0] - 0.8) <= 1e-16, "per-chain means are the sums over the number of samples",
         cm[3][0], 0.8);
  // two entries a chain: entry 1 of chain b is 10 (b + 1) + 1, 3 samples each the mean itself
  std::vector<double> a2;
  for (unsigned b = 0; b < 4; ++b)
    for (double mean : {0.5 + 0.1 * b, 10.0 * (b + 1) + 1.0}) {
      a2.push_back(3.0 * mean);
      a2.push_back(3.0 * mean * mean);
    }
  const ChainEstimate e2 = chain_estimate(a2, 4, 2, 3);
  std::printf("estimate %.17g %.17g %.17g %.17g %d\n", e2.mean[0], e2.error[0], e2.mean[1], e2.error[1], (int)e2.chain_spread);
  expect(chain_means_of(a2, 4, 2, 3)[2][1] == 31.0, "per-chain means: entry k of chain b", chain_means_of(a2, 4, 2, 3)[2][1], 31.0);

  // four chains of six entries: C_t(0 .. 2) and C_x(0 .. 2) of a 4 x 4 lattice, the loops W(1 .. 2, 1 .. 3), a path correlator of 6 lags
  const std::vector<std::vector<double>> m = {{1.00, 0.60, 0.45, 1.10, 0.62, 0.50},
                                              {1.05, 0.58, 0.40, 1.00, 0.66, 0.48},
                                              {0.95, 0.64, 0.50, 1.20, 0.70, 0.52},
                                              {1.10, 0.55, 0.42, 0.90, 0.58, 0.44}};
  // SigmaCorrelator::xi(1): xi_2 of the x part of the vector
  const auto xi_x = [](const std::vector<double> &C) { return xi_second_moment(std::vector<double>(C.begin() + 3, C.end()), 4); };
  print_jackknife("xi", chain_jackknife(m, xi_x));
  // PathCorrelator::effective_mass(2)
  print_jackknife("mass", chain_jackknife(m, [](const std::vector<double> &C) { return effective_mass(C, 2); }));
  // WilsonLoops::creutz(2, 2) with R = 2, S = 3, and through the class
  const auto chi22 = [](const std::vector<double> &W) { return creutz_ratio(W, 2, 3, 2, 2); };
  const ChainScalar c = chain_jackknife(m, chi22);
  print_jackknife("creutz", c);
  const WilsonLoops::Ratio cw = WilsonLoops::creutz_jackknife(m, 2, 3, 2, 2);
  expect(cw.value == c.value && cw.error == c.error && cw.has_error, "WilsonLoops::creutz_jackknife is chain_jackknife of creutz_ratio", cw.error, c.error);
  // GffCorrelator::energy(1, 0, 1) with P = 1: the effective mass of the slice 3 .. 5, and through the class
  const ChainScalar en = chain_jackknife(m, [](const std::vector<double> &C) { return effective_mass(C, 1); }, 3, 3);
  print_jackknife("energy", en);
  const GffCorrelator::Energy eg = GffCorrelator::energy_jackknife(m, 4, 4, 1, 1, 0, 1);
  expect(eg.value == en.value && eg.error == en.error && eg.has_error, "GffCorrelator::energy_jackknife is chain_jackknife on the slice of (d, q)",
         eg.error, en.error);
  // the functor sees the slice alone, in order
  const ChainScalar seen = chain_jackknife(m, [](const std::vector<double> &C) { return C.size() == 2 ? 10.0 * C[0] + C[1] : -1.0; }, 4, 2);
  const double want_seen = 10.0 * ((0.62 + 0.66 + 0.70 + 0.58) / 4) + (0.50 + 0.48 + 0.52 + 0.44) / 4;
  expect(std::fabs(seen.value - want_seen) <= 1e-14, "the functor sees entries first .. first + count - 1 as a vector of count entries", seen.value, want_seen);

  const ChainScalar one = chain_jackknife({m[0]}, xi_x);
  expect(!one.has_error && one.error == 0.0 && one.value == xi_x(m[0]), "one chain: the value of that chain, no jackknife error", one.error, 0.0);
  // C_x = (0, 1, 0) is not convex
  std::vector<std::vector<double>> flat = m;
  for (auto &row : flat) row[3] = row[5] = 0.0, row[4] = 1.0;
  const ChainScalar nan = chain_jackknife(flat, [](const std::vector<double> &C) { return effective_mass(C, 1); }, 3, 3);
  expect(std::isnan(nan.value), "NaN where the function of the mean is NaN", nan.value, NAN);
  // chains b = 1 .. 4 that are b times chain 0: the effective mass does not see the factor
  std::vector<std::vector<double>> scaled;
  for (unsigned b = 0; b < 4; ++b) {
    scaled.push_back(m[0]);
    for (double &v : scaled[b]) v *= b + 1.0;
  }
  const ChainScalar sc = chain_jackknife(scaled, [](const std::vector<double> &C) { return effective_mass(C, 2); });
  const double mass0 = effective_mass(m[0], 2);
  expect(sc.has_error && std::fabs(sc.value - mass0) <= 1e-14 && sc.error <= 1e-14, "chains that differ by a factor agree on a scale-free function",
         sc.value, mass0);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
