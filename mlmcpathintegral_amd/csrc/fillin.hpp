// fillin.hpp -- the densities and fill-in distributions of the Schwinger two-level step: -log of the ExpCos density, the
// Bessel-product draw (exact and approximate) and the Gaussian fill-in of a 2 x 2 block.  Included by lattice_twolevel.hip,
// and by test_math.hip for the test hook of bessel_i0 (mlmcpi_test_math).
#pragma once
#include "device_common.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// -log of ExpCosDistribution::evaluate(x, x_p, x_m) (distribution/expcosdistribution.cc:7-21)
__device__ __forceinline__ double expcos_neg_log_pdf(double beta, double x, double x_p, double x_m) {
  double dx = x_p - x_m, z = x - x_m;
  double flip = (dx < 0.0) ? -1.0 : 1.0;
  dx *= flip;
  if (dx > kPi) {
    flip = -flip;
    dx = kTwoPi - dx;
  }
  z *= flip;
  const double sigma = 2. * beta * fabs(cos(0.5 * dx));
  return -sigma * (cos(z - 0.5 * dx) - 1.0) + log(kTwoPi * bessel_i0_scaled(sigma));
}

// ---- fill-in distributions of the Schwinger lattice coarsened in both directions ----------------------------
// distribution/besselproductdistribution.{hh,cc} (beta <= 8), approximatebesselproductdistribution.{hh,cc} (beyond)
struct BesselFill {
  double beta, I0_twobeta, sigma_beta;
  double alphaZ[17];   // besselproductdistribution.hh:55-71 (host-built)
  int approximate;     // beta > 8 (quenchedschwingerconditionedfineaction.hh:62-71)
};

__device__ __forceinline__ double bessel_i0(double z) {  // gsl_sf_bessel_I0
  const double az = fabs(z);
  return exp(az) * bessel_i0_scaled(az);
}

// BesselProductDistribution::Znorm_inv(phi, rescaled = true), besselproductdistribution.cc:15-25
__device__ __forceinline__ double bessel_znorm_inv_rescaled(const BesselFill &P, double phi) {
  double s = 1.0;
  for (int k = 1; k <= 16; ++k) s += P.alphaZ[k] * cos(k * phi);
  return 1.0 / s;
}

// BesselProductDistribution::draw (besselproductdistribution.hh:88-152).  The calls of `site` are numbered
// n = 0, 1, ...: an outer attempt takes one call (two uniforms), the truncated-normal loop one call per two
// normals; n is bounded, so every lane leaves the loop.
__device__ __forceinline__ double bessel_product_draw(const RngKey &k, uint32_t site, const BesselFill &P, double x_p,
                                                      double x_m) {
  double dx = x_m - x_p;
  const double flip = (dx < 0) ? -1. : +1.;
  dx *= flip;
  const double N_p = erf((kPi - 0.5 * dx) / P.sigma_beta);
  const double N_m = erf(0.5 * dx / P.sigma_beta) * pow(P.I0_twobeta, 2. * (dx / kPi - 1.));
  const double C_p = pow(P.I0_twobeta, 2. * (1. - dx * dx / (4. * kPi * kPi)));
  const double C_m = pow(P.I0_twobeta, 2. * (1. - (dx - 2. * kPi) * (dx - 2. * kPi) / (4. * kPi * kPi)));
  const double sigma = P.sigma_beta / sqrt(2.);
  uint32_t n = 0;
  double x = 0.0;
  while (n < 60000u) {
    double xi, xi2;
    rng_uniforms(k, site, P_BESSEL, n++, xi, xi2);
    double a_min, a_max, mu, C;
    if (xi >= N_m / (N_p + N_m)) {
      a_min = -kPi + dx; a_max = +kPi; mu = 0.5 * dx; C = C_p;
    } else {
      a_min = -kPi; a_max = -kPi + dx; mu = 0.5 * (dx - 2. * kPi); C = C_m;
    }
    bool inside = false;
    while (!inside && n < 60000u) {
      double g0, g1;
      rng_normals(k, site, P_BESSEL, n++, g0, g1);
      x = sigma * g0 + mu;
      inside = (x >= a_min) && (x < a_max);
      if (!inside) {
        x = sigma * g1 + mu;
        inside = (x >= a_min) && (x < a_max);
      }
    }
    const double I0 = bessel_i0(2. * P.beta * cos(0.5 * x));
    const double I0_dx = bessel_i0(2. * P.beta * cos(0.5 * (x - dx)));
    const double xs = (x - mu) / P.sigma_beta;
    if (xi2 <= I0 * I0_dx / C * exp(xs * xs)) break;
  }
  return mod_2pi(flip * x + x_p);
}

// approximatebesselproductdistribution.cc:43-54
__device__ __forceinline__ void approx_bessel_params(double beta, double x0, double &N_p, double &s2p_inv,
                                                     double &s2m_inv) {
  if (x0 < 0.125 * kPi) {
    s2p_inv = beta; s2m_inv = 0.0; N_p = 1.0;
  } else {
    s2p_inv = beta * cos(0.25 * x0);
    s2m_inv = beta * sin(0.25 * x0);
    const double rho = pow(s2p_inv / s2m_inv, 1.5) * exp(-4.0 * (s2p_inv - s2m_inv));
    N_p = 1.0 / (1.0 + rho);
  }
}
// approximatebesselproductdistribution.hh:82-107: call 0 = the uniform, call 1 = the normal
__device__ __forceinline__ double approx_bessel_draw(const RngKey &k, uint32_t site, double beta, double x_p,
                                                     double x_m) {
  double x0 = x_p - x_m;
  double flip = (x0 < 0) ? -1. : +1.;
  x0 *= flip;
  if (x0 > kPi) { x0 = kTwoPi - x0; flip = -flip; }
  double N_p, s2p, s2m;
  approx_bessel_params(beta, x0, N_p, s2p, s2m);
  double xi, unused, g0, g1;
  rng_uniforms(k, site, P_BESSEL, 0, xi, unused);
  rng_normals(k, site, P_BESSEL, 1, g0, g1);
  const double sigma = (xi <= N_p) ? 1. / sqrt(s2p) : 1. / sqrt(s2m);
  const double xshift = (xi <= N_p) ? 0.0 : kPi;
  const double x = sigma * g0 + 0.5 * x0 - xshift;
  return mod_2pi(flip * x + x_m);
}
// approximatebesselproductdistribution.cc:7-40
__device__ __forceinline__ double approx_bessel_pdf(double beta, double x, double x_p, double x_m) {
  double x0 = x_p - x_m, z = x - x_m;
  double flip = (x0 < 0) ? -1. : +1.;
  x0 *= flip;
  if (x0 > kPi) { x0 = kTwoPi - x0; flip = -flip; }
  z *= flip;
  double N_p, s2p, s2m;
  approx_bessel_params(beta, x0, N_p, s2p, s2m);
  const double N_m = 1. - N_p;
  double sp = 0.0, sm = 0.0;
  for (int kk = -4; kk <= 4; ++kk) {
    double zs = z - 0.5 * x0 + 2 * kk * kPi;
    sp += sqrt(s2p) * exp(-0.5 * s2p * zs * zs);
    zs += kPi;
    sm += sqrt(s2m) * exp(-0.5 * s2m * zs * zs);
  }
  return sqrt(0.5 / kPi) * (N_p * sp + N_m * sm);
}

// ---- GaussianFillinDistribution (distribution/gaussianfillindistribution.{hh,cc}): the four interior links of a 2 x 2
// block given the four perimeter sums phi_12 .. phi_41, as a two-peak Gaussian mixture in three non-trivial directions
// (eta_1, eta_2, eta_3) plus a uniform common shift omega.  Used by QuenchedSchwingerGaussianConditionedFineAction.
__device__ __forceinline__ double gaussfill_pc(double beta, double Phi) {  // gaussianfillindistribution.hh get_pc
  if (Phi < 0.125 * kPi) return 1.0;
  if (Phi > 0.375 * kPi) return 0.0;
  const double sp = beta * cos(Phi), sm = beta * sin(Phi);
  const double rho = pow(sp / sm, 1.5) * exp(-4.0 * (sp - sm));
  return 1. / (1. + rho);
}

// gaussianfillindistribution.hh draw (add_gaussian_noise = true): calls of `site` with purpose P_GAUSSFILL: 0 -> (xi, omega / 2 pi),
// 1 -> normals of eta_1, eta_2, 2 -> normal of eta_3
__device__ __forceinline__ void gaussfill_draw(const RngKey &k, uint32_t site, double beta, double phi_12, double phi_23,
                                               double phi_34, double phi_41, double (&theta)[4]) {
  const double Phi = 0.25 * (phi_12 + phi_23 + phi_34 + phi_41);
  double Phi_star = Phi;
  bool swap_eta = false, shift_eta = false;
  if (Phi_star < 0) { Phi_star = -Phi_star; swap_eta = true; }
  if (Phi_star > 0.5 * kPi) { Phi_star = kPi - Phi_star; swap_eta = !swap_eta; shift_eta = true; }
  const double p_c = gaussfill_pc(beta, Phi_star);
  double xi, om, n1, n2, n3, unused;
  rng_uniforms(k, site, P_GAUSSFILL, 0, xi, om);
  rng_normals(k, site, P_GAUSSFILL, 1, n1, n2);
  rng_normals(k, site, P_GAUSSFILL, 2, n3, unused);
  double eta_1, eta_2, eta_3, sigma;
  if (xi < p_c) {
    eta_1 = 0.0; eta_2 = 0.0; eta_3 = 0.0;
    sigma = 1. / sqrt(4. * beta * cos(Phi_star));
  } else {
    eta_1 = kPi; eta_2 = 0.0; eta_3 = 0.5 * kPi;
    sigma = 1. / sqrt(4. * beta * sin(Phi_star));
  }
  const double sqrt2 = 1.41421356237309504880;
  eta_1 += sqrt2 * sigma * n1;
  eta_2 += sqrt2 * sigma * n2;
  eta_3 += sigma * n3;
  if (swap_eta) { const double t = eta_1; eta_1 = eta_2; eta_2 = t; }
  if (shift_eta) { eta_1 += kPi; eta_2 += kPi; }
  const double omega = 2. * kPi * om;
  theta[0] = mod_2pi(0.5 * (+eta_1 + eta_2 + eta_3) + omega);
  theta[1] = mod_2pi(0.5 * (+eta_1 - eta_2 - eta_3) + omega + Phi - phi_12);
  theta[2] = mod_2pi(0.5 * (-eta_1 - eta_2 + eta_3) + omega + 2. * Phi - phi_12 - phi_23);
  theta[3] = mod_2pi(0.5 * (-eta_1 + eta_2 - eta_3) + omega + 3. * Phi - phi_12 - phi_23 - phi_34);
}

// gaussianfillindistribution.cc:7-67 (add_gaussian_noise = true).  The peak lattices of construct_peaks (:70-118), in
// units of pi/2: main peaks = {0 (mod 4)}^3 and {2 (mod 4)}^3, secondary peaks = (2 mod 4, 0 mod 4, 1 mod 4) and
// (0 mod 4, 2 mod 4, 3 mod 4), each coordinate within one period of the base cell (n_offsets = 1; 0 for beta > 72, which
// keeps only the base cell's 9 + 4 peaks).
__device__ __forceinline__ double gaussfill_pdf(double beta, double theta_1, double theta_2, double theta_3, double theta_4,
                                                double phi_12, double phi_23, double phi_34, double phi_41) {
  double eta_1 = mod_2pi(0.5 * (theta_1 + theta_2 - theta_3 - theta_4) + 0.5 * (phi_41 - phi_23));
  double eta_2 = mod_2pi(0.5 * (theta_1 - theta_2 - theta_3 + theta_4) + 0.5 * (phi_34 - phi_12));
  const double eta_3 = mod_2pi(0.5 * (theta_1 - theta_2 + theta_3 - theta_4) + 0.25 * (-phi_12 + phi_23 - phi_34 + phi_41));
  double Phi_star = 0.25 * (phi_12 + phi_23 + phi_34 + phi_41);
  bool swap_eta = false;
  if (Phi_star < 0.) { Phi_star = -Phi_star; swap_eta = true; }
  if (Phi_star > 0.5 * kPi) {
    Phi_star = kPi - Phi_star;
    swap_eta = !swap_eta;
    eta_1 = mod_2pi(eta_1 + kPi);
    eta_2 = mod_2pi(eta_2 + kPi);
  }
  if (swap_eta) { const double t = eta_1; eta_1 = eta_2; eta_2 = t; }
  const double p_c = gaussfill_pc(beta, Phi_star);
  const double s2c = 2. * beta * cos(Phi_star), s2s = 2. * beta * sin(Phi_star);
  const bool wide = !(beta > 72.0);  // n_offsets = 1
  const double h = 0.5 * kPi;
  auto gauss = [&](double s2, int px, int py, int pz) {
    const double d1 = eta_1 - h * px, d2 = eta_2 - h * py, d3 = eta_3 - h * pz;
    return exp(-0.5 * s2 * (d1 * d1 + d2 * d2 + 2. * d3 * d3));
  };
  double g_c = 0.0, g_s = 0.0;
  if (wide) {
    for (int a = -4; a <= 4; a += 4)
      for (int b = -4; b <= 4; b += 4)
        for (int c = -4; c <= 4; c += 4) g_c += gauss(s2c, a, b, c);
    for (int a = -6; a <= 6; a += 4)
      for (int b = -6; b <= 6; b += 4)
        for (int c = -6; c <= 6; c += 4) g_c += gauss(s2c, a, b, c);
    for (int a = -6; a <= 6; a += 4)
      for (int b = -4; b <= 4; b += 4)
        for (int c = -3; c <= 5; c += 4) g_s += gauss(s2s, a, b, c);
    for (int a = -4; a <= 4; a += 4)
      for (int b = -6; b <= 6; b += 4)
        for (int c = -5; c <= 3; c += 4) g_s += gauss(s2s, a, b, c);
  } else {
    g_c += gauss(s2c, 0, 0, 0);
    for (int a = -2; a <= 2; a += 4)
      for (int b = -2; b <= 2; b += 4)
        for (int c = -2; c <= 2; c += 4) g_c += gauss(s2c, a, b, c);
    g_s = gauss(s2s, 2, 0, 1) + gauss(s2s, -2, 0, 1) + gauss(s2s, 0, 2, -1) + gauss(s2s, 0, -2, -1);
  }
  return p_c * pow(s2c, 1.5) * g_c + (1. - p_c) * pow(s2s, 1.5) * g_s;
}

}  // namespace mlmcpi
