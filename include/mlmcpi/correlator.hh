// correlator.hh -- host arithmetic on a mean time-slice correlator C(tau), tau = 0 .. M/2, of a periodic direction of even
// extent M (mlmcpi_sigma_level_correlator; the class that measures it is SigmaCorrelator, qoi.hh).  No device code.
#ifndef MLMCPI_CORRELATOR_HH
#define MLMCPI_CORRELATOR_HH
#include <cmath>
#include <vector>

namespace mlmcpi {

/** weight of lag tau in a sum over all M lags folded onto 0 .. M/2: 1 at tau = 0 and tau = M/2, 2 in between */
inline double correlator_weight(unsigned int tau, unsigned int M) { return tau == 0 || 2 * tau == M ? 1.0 : 2.0; }

/** chi = sum_tau w(tau) C(tau) (= |sum sigma|^2 / N configuration by configuration) */
inline double correlator_susceptibility(const std::vector<double> &C, unsigned int M) {
  double s = 0.0;
  for (unsigned int tau = 0; tau <= M / 2; ++tau) s += correlator_weight(tau, M) * C[tau];
  return s;
}

/** F = sum_tau w(tau) C(tau) cos(2 pi tau / M): the structure factor at the lowest non-zero momentum k = 2 pi / M */
inline double structure_factor(const std::vector<double> &C, unsigned int M) {
  const double k = 2.0 * std::acos(-1.0) / M;
  double s = 0.0;
  for (unsigned int tau = 0; tau <= M / 2; ++tau) s += correlator_weight(tau, M) * C[tau] * std::cos(k * tau);
  return s;
}

/** xi_2 from the susceptibility and the structure factor, however they were estimated (the cluster-improved pair of
 *  mlmcpi_sigma_level_sw_structure_draw included): sqrt(chi / F - 1) / (2 sin(pi / M)), NaN where chi / F < 1 */
inline double xi_from_chi_and_F(double chi, double F, unsigned int M) {
  const double r = chi / F - 1.0;
  return std::sqrt(r) / (2.0 * std::sin(std::acos(-1.0) / M));
}

/** second-moment correlation length xi_2 = sqrt(chi / F - 1) / (2 sin(pi / M)); for a single-cosh correlator of mass m it is
 *  exactly 1 / (2 sinh(m / 2)).  NaN where chi / F < 1 (noise) */
inline double xi_second_moment(const std::vector<double> &C, unsigned int M) {
  return xi_from_chi_and_F(correlator_susceptibility(C, M), structure_factor(C, M), M);
}

}  // namespace mlmcpi
#endif
