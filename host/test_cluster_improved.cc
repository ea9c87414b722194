// test_cluster_improved.cc -- ClusterImprovedSums (include/mlmcpi/cluster_improved.hh) alone: no device is touched and no library
// is linked.  tests/test_cluster_improved_host.py reads the output.
//   test_cluster_improved                 prints, as hexadecimal floats, what the class gives on fixed pseudo-random draws for 1, 2
//                                         and 5 chains with structure, with correlator, with both and F formed from C, and with
//                                         both and F given; tests/golden/cluster_improved_sums.txt is that text from the class as
//                                         it was inside sampler.hh, and it must not change
//   test_cluster_improved fatal WHAT WHY  WHAT = correlator | structure_factor | xi, WHY = without | nodraws: the call that must
//                                         end the program with the class's message
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mlmcpi/cluster_improved.hh"

using namespace mlmcpi;

static const unsigned Mt = 8, Mx = 6, n_out = (Mt / 2 + 1) + (Mx / 2 + 1), n_updates = 2, n_draws = 3;

static void record(ClusterImprovedSums &s, const std::vector<double> &imp, const std::vector<double> *F, const std::vector<double> *C) {
  s.record(Mt, Mx, imp, F, C);
}
static ClusterImprovedSums::Estimate xi(const ClusterImprovedSums &s, int d) { return s.xi(d, d == 0 ? Mt : Mx); }

/** one draw of B chains from a 64-bit linear congruential generator (Knuth's MMIX constants): every entry is n_updates times a
 *  profile value scattered by 10 %; the profiles are convex and chi is well above F, so that no xi is NaN */
struct Draws {
  uint64_t state = 2481317;
  double next(double base) {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return n_updates * base * (0.9 + 0.2 * ((double)(state >> 11) * 0x1p-53));
  }
  void draw(unsigned B, std::vector<double> &imp, std::vector<double> &F, std::vector<double> &C) {
    const double c_base[n_out] = {1.0, 0.6, 0.4, 0.3, 0.28, 1.0, 0.55, 0.35, 0.3}, f_base[2] = {1.1, 0.9};
    imp.assign(B, 0.0);
    F.assign(2 * B, 0.0);
    C.assign((size_t)B * n_out, 0.0);
    for (unsigned b = 0; b < B; ++b) {
      imp[b] = next(3.9);
      for (unsigned d = 0; d < 2; ++d) F[2 * b + d] = next(f_base[d]);
      for (unsigned k = 0; k < n_out; ++k) C[(size_t)b * n_out + k] = next(c_base[k]);
    }
  }
};

struct Config {
  const char *name;
  bool structure, correlator, give_F;
};
static const Config configs[4] = {{"structure", true, false, true}, {"correlator", false, true, false}, {"both", true, true, false},
                                  {"both_given_F", true, true, true}};

static void fill(ClusterImprovedSums &s, const Config &c, unsigned B) {
  Draws draws;
  std::vector<double> imp, F, C;
  for (unsigned k = 0; k < n_draws; ++k) {
    draws.draw(B, imp, F, C);
    record(s, imp, c.give_F ? &F : nullptr, c.correlator ? &C : nullptr);
  }
}

static void print_all() {
  for (unsigned B : {1u, 2u, 5u})
    for (const Config &c : configs) {
      ClusterImprovedSums s("TestSampler", B, n_updates, c.structure, c.correlator, n_out);
      fill(s, c, B);
      std::printf("improved %u %s %a %a %u\n", B, c.name, s.mean(), s.error(), (unsigned)s.draws());
      for (int d = 0; c.structure && d < 2; ++d) {
        const ClusterImprovedSums::Estimate f = s.structure_factor(d), x = xi(s, d);
        std::printf("structure %u %s %d %a %a %d\n", B, c.name, d, f.value, f.error, (int)f.has_error);
        std::printf("xi %u %s %d %a %a %d\n", B, c.name, d, x.value, x.error, (int)x.has_error);
      }
      if (c.correlator) {
        const ClusterImprovedSums::CorrelatorEstimate e = s.correlator();
        for (unsigned k = 0; k < n_out; ++k) std::printf("correlator %u %s %u %a %a %d\n", B, c.name, k, e.mean[k], e.error[k], (int)e.chain_spread);
      }
      s.reset();
      std::printf("reset %u %s %a %a %u\n", B, c.name, s.mean(), s.error(), (unsigned)s.draws());
    }
}

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "fatal")) {
    const bool without = !std::strcmp(argv[3], "without");
    // without: the other option alone, with draws; nodraws: every option, draws recorded and then forgotten
    const bool correlator_call = !std::strcmp(argv[2], "correlator");
    const Config c = without ? (correlator_call ? configs[0] : configs[1]) : configs[2];
    ClusterImprovedSums s("TestSampler", 2, n_updates, c.structure, c.correlator, n_out);
    fill(s, c, 2);
    if (!without) s.reset();
    if (correlator_call) s.correlator();
    else if (!std::strcmp(argv[2], "structure_factor")) s.structure_factor(1);
    else xi(s, 0);
    std::printf("the call returned\n");
    return 0;
  }
  print_all();
  return 0;
}
