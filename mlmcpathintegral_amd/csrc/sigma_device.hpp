// sigma_device.hpp -- device functions of the O(3) nonlinear sigma model shared by its kernels (sigma2d.hip) and the
// random-order sweep (random_sweep.hip).  Everything from here to the end of the including file is compiled without fp
// contraction, so that the same expression cannot round differently in two kernels (the canonical form: sigma2d.hip).
#pragma once
#include "internal.hpp"

#pragma clang fp contract(off)

namespace mlmcpi {

struct V3 {
  double x, y, z;
};

__device__ __forceinline__ V3 sigma_of(double2 a) {
  double st, ct, sp, cp;
  sincos(a.x, &st, &ct);
  sincos(a.y, &sp, &cp);
  return V3{st * cp, st * sp, ct};
}

// one association everywhere: (x x + y y) + z z
__device__ __forceinline__ double dot3(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__device__ __forceinline__ double2 angles_of(const V3 &s) {
  return make_double2(atan2(sqrt(s.x * s.x + s.y * s.y), s.z), atan2(s.y, s.x));
}

// x ~ p(x) ∝ exp(s x) on [-1, 1] (distribution/compactexpdistribution.{hh,cc}) by inversion:
//   x = log1p(u expm1(2 s)) / s - 1 = 1 + log1p((1 - u) expm1(-2 s)) / s,
// the second form because it cannot overflow at large s; x = 2 u - 1 at s = 0 (the reference's form is NaN there).
// Absolute error <= 2^-50 + 1.5 2^-52 |y| / ((1 + y) s), y = (1 - u) expm1(-2 s): log1p is ill-conditioned at y -> -1 (small u at
// s >~ 1; measured 3.8e-15 at s = 4, u = 0.003).  That term is the image of a change of u by less than its own spacing.
__device__ __forceinline__ double compact_exp_inverse(double s, double u) {
  if (!(s > 0.0)) return 2.0 * u - 1.0;
  double x = 1.0 + log1p((1.0 - u) * expm1(-2.0 * s)) / s;
  return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);
}

// NonlinearSigmaAction::heatbath_update (nonlinearsigmaaction.cc:24-72) in one frame: sigma' = x D + sqrt(1 - x^2)
// (cos a E + sin a D x E), D = Delta / |Delta|, E the reference's perpendicular (the component of D of smallest modulus
// zeroed; std::min_element picks the first), a = 2 pi v.  Delta = 0 leaves the spin as it is.
__device__ __forceinline__ V3 sigma_heatbath(const V3 &sig, const V3 &Dl, double beta, double u, double v) {
  const double n2 = Dl.x * Dl.x + Dl.y * Dl.y + Dl.z * Dl.z;
  if (!(n2 > 0.0)) return sig;
  const double nrm = sqrt(n2);
  const V3 d{Dl.x / nrm, Dl.y / nrm, Dl.z / nrm};
  const double ax = fabs(d.x), ay = fabs(d.y), az = fabs(d.z);
  int idx = 0;
  double m = ax;
  if (ay < m) { idx = 1; m = ay; }
  if (az < m) { idx = 2; m = az; }
  const double r = 1.0 / sqrt(1.0 - m * m);
  V3 e;
  if (idx == 0) e = V3{0.0, -d.z * r, d.y * r};
  else if (idx == 1) e = V3{-d.z * r, 0.0, d.x * r};
  else e = V3{d.y * r, -d.x * r, 0.0};
  const V3 f{d.y * e.z - d.z * e.y, d.z * e.x - d.x * e.z, d.x * e.y - d.y * e.x};
  const double x = compact_exp_inverse(beta * nrm, u);
  const double t = 1.0 - x * x;
  const double rp = t > 0.0 ? sqrt(t) : 0.0;
  double sa, ca;
  sincos(kTwoPi * v, &sa, &ca);
  const double p = rp * ca, q = rp * sa;
  return V3{x * d.x + (p * e.x + q * f.x), x * d.y + (p * e.y + q * f.y), x * d.z + (p * e.z + q * f.z)};
}

// NonlinearSigmaAction::overrelaxation_update (nonlinearsigmaaction.cc:75-91): sigma' = 2 (sigma . D) D - sigma
__device__ __forceinline__ V3 sigma_overrelax(const V3 &sig, const V3 &Dl) {
  const double n2 = Dl.x * Dl.x + Dl.y * Dl.y + Dl.z * Dl.z;
  if (!(n2 > 0.0)) return sig;
  const double nrm = sqrt(n2);
  const V3 d{Dl.x / nrm, Dl.y / nrm, Dl.z / nrm};
  const double c = 2.0 * (sig.x * d.x + sig.y * d.y + sig.z * d.z);
  return V3{c * d.x - sig.x, c * d.y - sig.y, c * d.z - sig.z};
}

__device__ __forceinline__ V3 sigma_update(const V3 &sig, const V3 &Dl, bool heat, double beta, const RngKey &key,
                                           uint32_t site) {
  if (!heat) return sigma_overrelax(sig, Dl);
  double u, v;
  rng_uniforms(key, site, P_SIGMA_HB, 0, u, v);
  return sigma_heatbath(sig, Dl, beta, u, v);
}

__device__ __forceinline__ V3 add4(const V3 &a, const V3 &b, const V3 &c, const V3 &d) {
  return V3{((a.x + b.x) + c.x) + d.x, ((a.y + b.y) + c.y) + d.y, ((a.z + b.z) + c.z) + d.z};
}

// Action::heatbath_update / overrelaxation_update(state, l) of vertex l on the angles `p` of one chain, in place: the body of
// sigma_site_update_kernel and of the random-order sweep
__device__ __forceinline__ void sigma_site_update(double2 *p, uint32_t Mt, uint32_t Mx, uint32_t l, bool heat, double beta,
                                                  const RngKey &key) {
  const uint32_t i = l % Mt, j = l / Mt;
  const V3 Dl = add4(sigma_of(p[j * Mt + (i + 1 == Mt ? 0 : i + 1)]), sigma_of(p[j * Mt + (i == 0 ? Mt - 1 : i - 1)]),
                     sigma_of(p[(j + 1 == Mx ? 0 : j + 1) * Mt + i]), sigma_of(p[(j == 0 ? Mx - 1 : j - 1) * Mt + i]));
  p[l] = angles_of(sigma_update(sigma_of(p[l]), Dl, heat, beta, key, l));
}

}  // namespace mlmcpi
