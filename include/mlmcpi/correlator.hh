// correlator.hh -- host arithmetic on a mean time-slice correlator C(tau), tau = 0 .. M/2, of a periodic direction of even
// extent M (mlmcpi_sigma_level_correlator; the class that measures it is SigmaCorrelator, qoi.hh), and on the time correlator of
// a 1-D path, on Wilson loops and on the slice correlators of the Gaussian free field (below): the functions of a mean vector whose
// error over chains chain_estimate.hh forms (chain_jackknife).  No device code.
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

// ---- the time correlator C(tau) = <x(0) x(tau)> of a 1-D path (mlmcpi_path_correlator; the class that measures it is
// PathCorrelator, qoi.hh) ----

/** effective mass at lag tau, 1 <= tau <= C.size() - 2: acosh((C(tau - 1) + C(tau + 1)) / (2 C(tau))), which is m exactly for
 *  C = A cosh(m (M/2 - tau)), wrap-around included; times 1/a it is the gap E_1 - E_0 where one state dominates.  NaN where the
 *  argument is < 1 (a triple that is not convex: noise) */
inline double effective_mass(const std::vector<double> &C, unsigned int tau) {
  const double r = (C[tau - 1] + C[tau + 1]) / (2.0 * C[tau]);
  return r >= 1.0 ? std::acosh(r) : std::nan("");
}

/** omega~ of the lattice harmonic oscillator, cosh(omega~) = 1 + a^2 mu2 / 2, a = T_final / M: the gap in lattice units */
inline double path_ho_lattice_omega(unsigned int M, double T_final, double mu2) {
  const double a = T_final / M;
  return std::acosh(1.0 + 0.5 * a * a * mu2);
}

/** <x_0 x_tau> of the harmonic oscillator S = (a m0 / 2) sum_j ((x_j - x_{j-1})^2 / a^2 + mu2 x_j^2) on the periodic lattice of
 *  M sites: (a / m0) cosh(omega~ (M/2 - tau)) / (2 sinh(omega~) sinh(omega~ M / 2)); at tau = 0 the action's analytic <x^2> */
inline double path_correlator_ho_exact(unsigned int M, double T_final, double m0, double mu2, unsigned int tau) {
  const double a = T_final / M, w = path_ho_lattice_omega(M, T_final, mu2);
  return (a / m0) * std::cosh(w * (0.5 * M - (double)tau)) / (2.0 * std::sinh(w) * std::sinh(0.5 * w * M));
}

// ---- Wilson loops W(r, s) of the quenched Schwinger model (mlmcpi_schwinger_wilson_loops; the class that measures them is
// WilsonLoops, qoi.hh) ----

/** <W(r, s)> on the periodic Mt x Mx lattice, V = Mt Mx, A = r s <= V: sum_n I_n(beta)^(V-A) I_(n+1)(beta)^A / sum_n I_n(beta)^V over
 *  all integers n (the character expansion; the sum over n carries the torus constraint sum theta_p = 0 mod 2 pi).  Evaluated with
 *  rho_n = I_n / I_0 (the scaling of the Bessel functions cancels), n = 0, -1, 1, -2, .. until the terms fall below 1e-17 of the sum */
inline double wilson_loop_exact(double beta, unsigned int Mt, unsigned int Mx, unsigned int r, unsigned int s) {
  const double V = (double)Mt * Mx, A = (double)r * s;
  const double i0 = std::cyl_bessel_i(0.0, beta);
  auto rho = [&](int n) { return std::cyl_bessel_i((double)(n < 0 ? -n : n), beta) / i0; };
  double num = 0.0, den = 0.0;
  for (int m = 0; m < 400; ++m) {
    double tn = 0.0, td = 0.0;
    for (int n : {m, -m - 1}) {  // the pair (I_n, I_(n+1)) is (I_m, I_(m+1)) and, mirrored, (I_(m+1), I_m)
      const double a = rho(n), b = rho(n + 1);
      tn += std::pow(a, V - A) * std::pow(b, A);
      td += std::pow(a, V);
    }
    num += tn;
    den += td;
    if (tn <= 1e-17 * num && td <= 1e-17 * den) break;
  }
  return num / den;
}

/** the string tension of the infinite lattice, sigma = -log(I_1(beta) / I_0(beta)): W -> exp(-sigma r s) */
inline double string_tension_exact(double beta) { return -std::log(std::cyl_bessel_i(1.0, beta) / std::cyl_bessel_i(0.0, beta)); }

/** the Creutz ratio chi(r, s) = -log[W(r,s) W(r-1,s-1) / (W(r-1,s) W(r,s-1))] of W [R][S] (entry [r-1][s-1]), 1 <= r <= R, 1 <= s <= S,
 *  with W(0,.) = W(.,0) = 1: the string tension exactly for a pure area law.  NaN where the argument is not positive (noise) */
inline double creutz_ratio(const std::vector<double> &W, unsigned int R, unsigned int S, unsigned int r, unsigned int s) {
  (void)R;
  auto w = [&](unsigned int a, unsigned int b) { return a == 0 || b == 0 ? 1.0 : W[(size_t)(a - 1) * S + (b - 1)]; };
  const double q = w(r, s) * w(r - 1, s - 1) / (w(r - 1, s) * w(r, s - 1));
  return q > 0.0 ? -std::log(q) : std::nan("");
}

// ---- the momentum-projected slice correlators of the Gaussian free field (mlmcpi_gff_correlator; the class that measures them
// is GffCorrelator, qoi.hh) ----

/** E_q of the GFF action on the unrotated Mt x Mx lattice, mu^2 = (mass / Mt)^2 as the action defines it: the lattice dispersion
 *  relation cosh E_q = 1 + (mu^2 + 2 - 2 cos(2 pi q / Mx)) / 2, the decay rate of C_t(tau; q) */
inline double gff_dispersion_exact(unsigned int Mt, unsigned int Mx, double mass, unsigned int q) {
  const double mu2 = (mass / Mt) * (mass / Mt);
  return std::acosh(1.0 + 0.5 * (mu2 + 2.0 - 2.0 * std::cos(2.0 * M_PI * q / Mx)));
}

/** <C_t(tau; q)> of that action, as the mode sum (1/Mt) sum_k cos(2 pi k tau / Mt) / lambda(k, q), lambda(k, q) = 4 + mu^2 -
 *  2 cos(2 pi k / Mt) - 2 cos(2 pi q / Mx) the eigenvalue of the precision matrix; equal to cosh(E_q (Mt/2 - tau)) / (2 sinh E_q
 *  sinh(E_q Mt / 2)).  C_x(tau; q) is the same with the extents exchanged. */
inline double gff_correlator_exact(unsigned int Mt, unsigned int Mx, double mass, unsigned int q, unsigned int tau) {
  const double mu2 = (mass / Mt) * (mass / Mt), cq = 2.0 * std::cos(2.0 * M_PI * q / Mx);
  double s = 0.0;
  for (unsigned int k = 0; k < Mt; ++k)
    s += std::cos(2.0 * M_PI * (double)(((unsigned long long)k * tau) % Mt) / Mt) / (4.0 + mu2 - 2.0 * std::cos(2.0 * M_PI * k / Mt) - cq);
  return s / Mt;
}

// ---- the gradient flow of the O(3) sigma model (mlmcpi_sigma_level_flowed_charge; the class that measures it is
// SigmaFlowProfile, qoi.hh) ----

/** the reference scale of the flow: the flow time at which t <E(t)> / n, given as tE[k] at the ascending times[k], first reaches
 *  c, by linear interpolation between the neighbouring pair of times that brackets c; NaN when no pair does */
inline double flow_scale(const std::vector<double> &times, const std::vector<double> &tE, double c) {
  for (size_t k = 0; k + 1 < times.size() && k + 1 < tE.size(); ++k) {
    const double lo = tE[k], hi = tE[k + 1];
    if (((lo <= c && c <= hi) || (hi <= c && c <= lo)) && lo != hi)
      return times[k] + (times[k + 1] - times[k]) * (c - lo) / (hi - lo);
  }
  return std::nan("");
}

}  // namespace mlmcpi
#endif
