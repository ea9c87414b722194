// cluster_improved.hh -- ClusterImprovedSums: host arithmetic on the cluster-improved estimators that the cluster samplers of the
// sigma model download draw by draw (cluster_sampler.hh).  Plain sums on std::vector; no device code, no ABI header
// (host/test_cluster_improved.cc runs the class alone).
#ifndef MLMCPI_CLUSTER_IMPROVED_HH
#define MLMCPI_CLUSTER_IMPROVED_HH
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "chain_estimate.hh"
#include "correlator.hh"

namespace mlmcpi {

/** What the cluster samplers of the sigma model keep of their improved estimators (WolffClusterSampler, SwendsenWangSampler):
 *  since the last reset(), the mean over draws of the per-draw improved chi_m (the mean over the draw's updates and the chains)
 *  with its standard error over the draws and, PER CHAIN, the sums over the updates of the improved chi_m, F_t, F_x (structure)
 *  and of the improved C_t and C_x, every lag (correlator).  structure_factor(d) and correlator() are means over the chains with
 *  their spread as the error, as SigmaCorrelator::means_and_errors; xi(d) is xi_2 from the chain-averaged (chi, F) with a
 *  jackknife over the chains, the arithmetic of SigmaCorrelator::xi (NaN where chi / F < 1).
 *  The sums stay here and not in chain_estimate.hh: the mean over chains divides every chain's sum by the chain count before it
 *  adds (chain_estimate adds, then divides), and xi jackknifes the pair of sums, not a vector of per-chain means; other bits. */
class ClusterImprovedSums {
public:
  typedef ChainScalar Estimate;  // has_error: the spread and the jackknife over chains need batch >= 2
  struct CorrelatorEstimate {
    std::vector<double> mean, error;  // [n_out], C_t first: the layout of SigmaCorrelator::Estimate
    bool chain_spread;                // true: error = spread of the per-chain means (batch >= 2); false: no error (one chain)
  };
  ClusterImprovedSums(const char *owner_, unsigned int B_, unsigned int n_updates_, bool structure, bool correlator, unsigned int n_out_)
      : owner(owner_), B(B_), n_updates(n_updates_), with_structure(structure), with_correlator(correlator), n_out(n_out_),
        chain_C(correlator ? (size_t)B_ * n_out_ : 0, 0.0), chain_chi(B_, 0.0),
        chain_F{std::vector<double>(B_, 0.0), std::vector<double>(B_, 0.0)} {}
  void reset() {
    improved_sum = improved_sum2 = 0.0;
    draws_counted = 0;
    std::fill(chain_chi.begin(), chain_chi.end(), 0.0);
    for (std::vector<double> &f : chain_F) std::fill(f.begin(), f.end(), 0.0);
    std::fill(chain_C.begin(), chain_C.end(), 0.0);
  }
  /** one draw on an Mt x Mx level: imp [B], the draw's improved chi_m per chain summed over its updates; F [B][2] (may be NULL) and
   *  C [B][n_out] (may be NULL) likewise.  With structure and no F, F_d of the draw is structure_factor() of the draw's improved
   *  C_d, chain by chain. */
  void record(unsigned int Mt, unsigned int Mx, const std::vector<double> &imp, const std::vector<double> *F, const std::vector<double> *C) {
    double v = 0.0;
    for (double x : imp) v += x;
    if (with_correlator && C)
      for (size_t k = 0; k < C->size(); ++k) chain_C[k] += (*C)[k];
    if (with_structure && F) {
      for (unsigned int b = 0; b < B; ++b) {
        chain_chi[b] += imp[b];
        chain_F[0][b] += (*F)[2 * b];
        chain_F[1][b] += (*F)[2 * b + 1];
      }
    } else if (with_structure && C) {
      const unsigned int nt = Mt / 2 + 1;
      for (unsigned int b = 0; b < B; ++b) {
        const std::vector<double>::const_iterator c = C->begin() + (size_t)b * n_out;
        chain_chi[b] += imp[b];
        chain_F[0][b] += mlmcpi::structure_factor(std::vector<double>(c, c + nt), Mt);
        chain_F[1][b] += mlmcpi::structure_factor(std::vector<double>(c + nt, c + n_out), Mx);
      }
    }
    v /= (double)B * n_updates;                          // this draw's value: the mean over its updates and the chains
    improved_sum += v;
    improved_sum2 += v * v;
    ++draws_counted;
  }
  uint64_t draws() const { return draws_counted; }
  CorrelatorEstimate correlator() const {
    if (!with_correlator) fail("improved_correlator", "constructed without ClusterParameters::correlator.");
    if (!draws_counted) fail("improved_correlator", "no draws since reset_improved().");
    CorrelatorEstimate e{std::vector<double>(n_out, 0.0), std::vector<double>(n_out, 0.0), B >= 2};
    for (unsigned int k = 0; k < n_out; ++k) {
      const Estimate s = chain_mean_and_spread(&chain_C[k], n_out);
      e.mean[k] = s.value;
      e.error[k] = s.error;
    }
    return e;
  }
  Estimate structure_factor(int d) const {
    need_structure("improved_structure_factor");
    return chain_mean_and_spread(chain_F[d].data(), 1);
  }
  /** M: the extent of direction d */
  Estimate xi(int d, unsigned int M) const {
    need_structure("improved_xi");
    double chi = 0.0, F = 0.0;
    for (unsigned int b = 0; b < B; ++b) {
      chi += chain_chi[b];
      F += chain_F[d][b];
    }
    Estimate r{xi_from_chi_and_F(chi / B, F / B, M), 0.0, B >= 2};
    if (B >= 2) {
      std::vector<double> x(B);
      double xm = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) {
        x[b] = xi_from_chi_and_F((chi - chain_chi[b]) / (B - 1.0), (F - chain_F[d][b]) / (B - 1.0), M);
        xm += x[b] / B;
      }
      for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
      r.error = std::sqrt((B - 1.0) / B * s2);
    }
    return r;
  }
  double mean() const { return draws_counted ? improved_sum / draws_counted : 0.0; }
  double error() const {
    if (draws_counted < 2) return 0.0;
    const double n = (double)draws_counted, m = improved_sum / n, var = std::max(0.0, (improved_sum2 - n * m * m) / (n - 1.0));
    return std::sqrt(var / n);
  }

private:
  /** of the per-chain sums sums[b * stride], b < B, each over draws() * n_updates updates: the mean over the chains of the
   *  per-chain means and, batch >= 2, their spread over sqrt(batch) */
  Estimate chain_mean_and_spread(const double *sums, size_t stride) const {
    const double n = (double)draws_counted * n_updates;
    double m = 0.0, s2 = 0.0;
    for (unsigned int b = 0; b < B; ++b) m += sums[b * stride] / n / B;
    for (unsigned int b = 0; b < B; ++b) s2 += (sums[b * stride] / n - m) * (sums[b * stride] / n - m);
    return Estimate{m, B >= 2 ? std::sqrt(s2 / ((double)B * (B - 1.0))) : 0.0, B >= 2};
  }
  /** the error convention of samplestate.hh's fatal(), which this header cannot include: message on cerr, then exit */
  [[noreturn]] void fail(const char *what, const char *why) const {
    std::cerr << "ERROR: " << owner << "::" << what << ": " << why << std::endl;
    std::exit(EXIT_FAILURE);
  }
  void need_structure(const char *what) const {
    if (!with_structure) fail(what, "constructed without ClusterParameters::structure.");
    if (!draws_counted) fail(what, "no draws since reset_improved().");
  }
  const std::string owner;
  const unsigned int B, n_updates;
  const bool with_structure, with_correlator;
  const unsigned int n_out;
  std::vector<double> chain_C;                // per chain and lag: sums over the updates of the improved C
  std::vector<double> chain_chi, chain_F[2];  // per chain: sums over the updates of improved chi_m, F_t, F_x
  double improved_sum = 0.0, improved_sum2 = 0.0;
  uint64_t draws_counted = 0;
};

}  // namespace mlmcpi
#endif
