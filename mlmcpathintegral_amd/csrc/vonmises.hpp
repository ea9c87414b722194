// vonmises.hpp -- the exact von Mises sampler of the heat-bath updates (wrapped-Cauchy envelope), the conditionals built on it
// (ExpCos, ExpSin2), the scaled Bessel I0, and the colour phase that draws a workgroup's cells with it (HbPool, heatbath_cells).
// Included by step_envelope.hpp, site_update.hpp, fillin.hpp and lattice_sweep.hpp, and by schwinger_sweeps.hip,
// rotor_sweeps.hip, path_twolevel.hip, lattice_twolevel.hip, test_hooks.hip and test_math.hip.
#pragma once
#include "device_common.hpp"

namespace mlmcpi {

// ---- heat-bath angle draws ------------------------------------------------------------------------
// Both heat-bath conditionals of the reference are von Mises laws p(x) ~ exp(kappa cos(x - c)):
//   ExpCosDistribution   kappa = tau = 2 beta |cos(dx/2)|      distribution/expcosdistribution.{hh:51-65,cc:7-21}
//   ExpSin2Distribution  kappa = sigma / 2                      distribution/expsin2distribution.{hh:45-58,cc:20-24}
// The reference draws them by rejection from a Gaussian envelope with acceptance rate
// sqrt(kappa/pi) I0(kappa) e^-kappa <= 0.27, -> 0 like sqrt(kappa) for flat conditionals: fine one
// site at a time on a CPU, but on a 64-wide wave the slowest lane sets the pace, and in a
// 1024^2 x batch sweep some link always has kappa ~ 1e-8 (~1e4 attempts) and stalls the whole
// launch.  The device samples the SAME distribution with the wrapped-Cauchy envelope of Best &
// Fisher (Appl. Statist. 28 (1979) 152-157): acceptance >= 0.65 for every kappa, one cosine per
// attempt, one arccosine per draw.
//
// Arithmetic.  Best & Fisher's envelope parameter r = (1 + rho^2) / (2 rho) simplifies to r = (1 + s) / (2 kappa) with
// s = sqrt(1 + 4 kappa^2); everything is written in R = kappa r = (1 + s) / 2 (one square root, no division, finite as
// kappa -> 0):   z = cos(pi u1),  f = cos(theta) = (kappa + R z) / (R + kappa z),  c = R - kappa f in (1/2, R + kappa],
// accept with probability c exp(1 - c).
//
// Random numbers.  ONE Philox call (counter word 3 = P_VONMISES << 24 | sub0 | t, t = 0, 1, ...) feeds TWO attempts,
// 2t from words (x, y) and 2t + 1 from (z, w).  Of the 64 bits v = hi:lo of an attempt
//     bits 12..63  u1 = (v >> 12) 2^-52           the proposal,
//     bit  0       the sign of the angle,
//     bits 1..11   b                               the leading 11 bits of the acceptance uniform u2 = (b + u2') / 2048.
// b alone decides the test unless c exp(1 - c) falls into [b, b + 1) / 2048 (about one attempt in 10^3); only then is
// the tail u2' (53 bits) taken from a second call (word 3 | kVmRefine), and the decision is the exact fp64 one
// (c (2 - c) > u2 or log(c / u2) + 1 - c >= 0).  The screening test runs in fp32 (hardware exp) with a guard band that
// covers the fp32 rounding, so whichever tier decides, the decision is the one the exact test would take for the c of the
// proposal f that is returned (c is one fma away from f; against the c of the ideal f(u1) it carries kappa times the
// rounding of f, 3e4 ulp at kappa = 1e4).  One exception: beyond c = 88 exp(1 - c) leaves the fp32 range, the screen sees
// a = 0 with a band of 0 and rejects; the exact test would accept at u2 = 0 alone, once in 2^64 attempts.

// cos(d / 2) for any |d| < 2^30: d / (4 pi) reduced to t in [-1/2, 1/2], cos(2 pi t) = cos(pi * 2|t|)
__device__ __forceinline__ double cos_half(double d) {
  const double v = d * (0.25 / kPi);
  const double t = v - rint(v);
  return cospi_unit(2.0 * fabs(t));
}

// The sampler in three pieces so that callers can run the (divergent) attempt loop as a per-lane
// work queue: vm_envelope once per draw, vm_attempt_pair until it returns true, vm_angle once.
__device__ __forceinline__ double vm_clamp(double kappa) {
  return fmax(kappa, 1e-12);  // also maps NaN to a finite concentration: every wave reaches its exit
}

__device__ __forceinline__ double vm_envelope(double kappa) {  // R = kappa r = (1 + sqrt(1 + 4 kappa^2)) / 2
  return fma(0.5, fast_sqrt(fma(4. * kappa, kappa, 1.)), 0.5);
}

constexpr uint32_t kMaxVmPairs = 512u;     // attempt bound (2 x 512 attempts): every lane leaves the loop
constexpr uint32_t kVmFillin = 1u << 23;   // sub0 of the two-level fill-in draws (sweeps: 0)
constexpr uint32_t kVmRefine = 1u << 22;   // the call that supplies the tails u2' of a pair's acceptance uniforms

// proposal uniform: the top 52 bits of hi:lo as the mantissa of a double in [1, 2), minus 1
__device__ __forceinline__ double u01_52(uint32_t lo, uint32_t hi) {
  return __hiloint2double((int)((hi >> 12) | 0x3FF00000u), (int)__builtin_amdgcn_alignbit(hi, lo, 12)) - 1.0;
}

// The fp32 screen of an attempt: the acceptance probability a = c exp(1 - c) and the guard band around it.  (A function of
// its own so that tests/test_device_math_gpu.py can read the two numbers vm_try compares with.)
__device__ __forceinline__ void vm_screen(double c, float &af, float &band) {
  const float cf = (float)c;
  af = cf * __expf(1.0f - cf);              // acceptance probability c exp(1 - c), fp32
  band = af * (1e-5f * (1.0f + cf));        // >> its fp32 error (~4e-7 (1 + c) relative)
}

// One attempt from the word pair (lo, hi): proposal f = cos(theta), c, and the screening decision:
// 1 accepted, 0 rejected, -1 open (the 11 leading bits of u2 do not decide).
__device__ __forceinline__ int vm_try(uint32_t lo, uint32_t hi, double kappa, double R, double &f, double &c) {
  const double z = cospi_unit(u01_52(lo, hi));
  f = fast_div(fma(R, z, kappa), fma(kappa, z, R));
  c = fma(-kappa, f, R);
  float af, band;
  vm_screen(c, af, band);
  const float lo_s = (float)((lo >> 1) & 0x7FFu) * (1.0f / 2048.0f), hi_s = lo_s + (1.0f / 2048.0f);  // u2 in [lo_s, hi_s)
  return hi_s <= af - band ? 1 : (lo_s >= af + band ? 0 : -1);
}

// the exact test with the full acceptance uniform u2 = (b + tail) / 2048
__device__ __forceinline__ int vm_exact(uint32_t lo, double tail, double c) {
  const double u2 = ((double)((lo >> 1) & 0x7FFu) + tail) * (1.0 / 2048.0);
  return (c * (2. - c) - u2 > 0. || log(c / u2) + 1. - c >= 0.) ? 1 : 0;
}

// Attempts 2 pair and 2 pair + 1; returns true when one of them is accepted (or when the attempt bound is hit).
// f = cos(theta).  sub0 separates streams that share (site, chain, step): 0 for sweeps, kVmFillin for two-level fill-ins.
template <class Keys>   // RngKey alone, or RngKey + PhiloxVKeys (hot loops)
__device__ __forceinline__ bool vm_attempt_pair_impl(const RngKey &k, const Keys *vk, uint32_t site, uint32_t pair, double kappa, double R,
                                                     double &f, bool &negative, uint32_t sub0) {
  const uint32_t w3 = (P_VONMISES << 24) | sub0 | pair;
  const U4 q = vk ? philox4x32_10(site, k.chain, k.step, w3, k.k0, k.k1, *vk) : philox4x32_10(site, k.chain, k.step, w3, k.k0, k.k1);
  double fa, ca, fb, cb;
  int sa = vm_try(q.x, q.y, kappa, R, fa, ca), sb = vm_try(q.z, q.w, kappa, R, fb, cb);
  if (sa < 0 || (sa == 0 && sb < 0)) {  // a decision that matters is open: fetch the tails
    const U4 e = philox4x32_10(site, k.chain, k.step, w3 | kVmRefine, k.k0, k.k1);
    if (sa < 0) sa = vm_exact(q.x, u01(e.x, e.y), ca);
    if (sa == 0 && sb < 0) sb = vm_exact(q.z, u01(e.z, e.w), cb);
  }
  f = sa == 1 ? fa : fb;
  negative = ((sa == 1 ? q.x : q.z) & 1u) != 0;
  return sa == 1 || sb == 1 || pair + 1 >= kMaxVmPairs;
}
__device__ __forceinline__ bool vm_attempt_pair(const RngKey &k, uint32_t site, uint32_t pair, double kappa, double R,
                                                double &f, bool &negative, uint32_t sub0 = 0) {
  return vm_attempt_pair_impl<PhiloxVKeys>(k, nullptr, site, pair, kappa, R, f, negative, sub0);
}
__device__ __forceinline__ bool vm_attempt_pair(const RngKey &k, const PhiloxVKeys *vk, uint32_t site, uint32_t pair, double kappa,
                                                double R, double &f, bool &negative, uint32_t sub0 = 0) {
  return vm_attempt_pair_impl<PhiloxVKeys>(k, vk, site, pair, kappa, R, f, negative, sub0);
}

__device__ __forceinline__ double vm_angle(double f, bool negative) {
  const double theta = fast_acos(fmin(1.0, fmax(-1.0, f)));
  return negative ? -theta : theta;
}

__device__ __forceinline__ double vonmises_draw(const RngKey &k, uint32_t site, double kappa, uint32_t sub0 = 0) {
  kappa = vm_clamp(kappa);
  const double R = vm_envelope(kappa);
  double f = 1.0;
  bool negative = false;
  for (uint32_t pair = 0; !vm_attempt_pair(k, site, pair, kappa, R, f, negative, sub0); ++pair) {
  }
  return vm_angle(f, negative);
}

// quenchedschwingeraction.cc:46-54 -> expcosdistribution.hh:51-65: the conditional of a link between staple angles
// x_p, x_m is exp(beta [cos(x - x_p) + cos(x - x_m)]) = exp(2 beta cos((x_m - x_p)/2) cos(x - (x_p + x_m)/2)): a von Mises
// law around the mean staple angle, shifted by pi when the cosine is negative.  The identity holds for any real
// x_p, x_m, so the staple sums need no mod_2pi of their own (the reference wraps them and tests |dx| > pi; same angle).
__device__ __forceinline__ void expcos_params(double beta, double x_p, double x_m, double &tau, double &centre) {
  const double ch = cos_half(x_m - x_p);
  tau = 2. * beta * fabs(ch);
  centre = fma(0.5, x_p + x_m, ch < 0.0 ? kPi : 0.0);
}

__device__ __forceinline__ double expcos_draw(const RngKey &k, uint32_t site, double beta, double x_p,
                                              double x_m, uint32_t sub0 = 0) {
  double tau, centre;
  expcos_params(beta, x_p, x_m, tau, centre);
  return mod_2pi_fast(vonmises_draw(k, site, tau, sub0) + centre);
}

// rotoraction.cc:20-37 -> expsin2distribution.hh:45-58
__device__ __forceinline__ double expsin2_draw(const RngKey &k, uint32_t site, double sigma) {
  return vonmises_draw(k, site, 0.5 * sigma);
}

// exp(-z) I0(z), z >= 0 (the normalisation of the rotor's conditioned fine action): power series in
// z^2/4 for z < 30 (all terms positive: no cancellation), Hankel asymptotic series beyond.  Relative accuracy: 1e-15 for
// z >= 30; below, (z + 123) 2^-53 <= 1.7e-14 by counting the roundings of the series (measured 1.7e-15 at z = 26.4,
// tests/test_device_math_gpu.py).  The reference calls gsl_sf_bessel_I0_scaled (expsin2distribution.cc:7-17).
__device__ __forceinline__ double bessel_i0_scaled(double z) {
  if (z < 30.0) {
    const double q = 0.25 * z * z;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 120; ++k) {
      term *= q / ((double)k * (double)k);
      sum += term;
      if (term < 1e-17 * sum) break;
    }
    return exp(-z) * sum;
  }
  const double w = 1.0 / (8.0 * z);
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 30; ++k) {
    const double odd = 2.0 * k - 1.0;
    term *= odd * odd * w / (double)k;
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum / sqrt(kTwoPi * z);
}

// ExpSin2Distribution::fast_2pi_I0_scaled (expsin2distribution.cc:7-17), including the reference's
// three-term expansion for z > 100
__device__ __forceinline__ double two_pi_i0_scaled(double z) {
  if (z > 100.) {
    const double zi = 1. / z;
    return sqrt(2. * kPi * zi) * (1. + 0.125 * zi + 0.0703125 * zi * zi);
  }
  return 2. * kPi * bessel_i0_scaled(z);
}

// Heat-bath colour phase.  Each thread owns up to S cells of the region (linear index tid + NT m).  Their conditional
// parameters are set up first (no divergence) and every cell gets its first PAIR of attempts (one Philox call) in
// straight-line code; about 97 % of the cells are done then.  What is left is a geometric tail: a few cells per wave
// that need one more call, a few per workgroup that need two.  Retrying them where they sit makes every wave run the
// whole attempt code with one or two live lanes, several times over.  Instead the leftovers of the whole workgroup are
// pushed into a small LDS pool (HbPool: concentration, centre, Philox site, LDS offset), and after a barrier the first
// threads of the workgroup finish them, one entry each, and write the angles straight to their cells.  Entries that do not fit (the pool
// holds `cap` of them; expected ~40 per 1280 cells at beta = 1) are retried by their own lane on the spot.  Cells
// accepted at once are written back at once (cells of one colour phase are not in each other's stencils), so nothing
// but the loop state lives across cells.  Which random numbers a cell consumes is fixed by (site, attempt), so the
// result does not depend on any of this scheduling.
struct HbPool {
  double *base;            // kap[cap] | cen[cap] | site[cap] | off[cap] | count[2]
  uint32_t cap, use;       // capacity (0: no pool); number of uses so far (uniform over the workgroup)
  // pushes of use u go to count[u & 1]; the other counter is cleared meanwhile
  static __host__ __device__ constexpr size_t bytes(uint32_t cap) { return (size_t)cap * 24 + 8; }
  __device__ double *kap() const { return base; }
  __device__ double *cen() const { return base + cap; }
  __device__ uint32_t *site() const { return (uint32_t *)(base + 2 * cap); }
  __device__ uint32_t *off() const { return (uint32_t *)(base + 2 * cap) + cap; }
  __device__ uint32_t *count() const { return (uint32_t *)(base + 2 * cap) + 2 * cap; }
  __device__ static HbPool carve(double *lds, uint32_t cap) {  // call from every thread; thread 0 clears the counters
    HbPool p{lds, cap, 0u};
    if (cap && threadIdx.x == 0) p.count()[0] = p.count()[1] = 0;  // visible after the caller's next barrier
    return p;
  }
};

template <int NT, int S, bool LEAN = false, class Setup, class Commit>   // LEAN: round keys on the scalar side (16 VGPRs less)
__device__ __forceinline__ void heatbath_cells(uint32_t total, const RngKey &key, HbPool &pool, Setup setup, Commit commit) {
  PhiloxVKeys vk_;
  if (!LEAN) vk_ = philox_vkeys(key.k0, key.k1);
  const PhiloxVKeys *const vk = LEAN ? nullptr : &vk_;
  for (uint32_t b0 = 0; b0 < total; b0 += S * NT) {  // uniform trip count: the barriers below need every thread
    uint32_t *cnt = pool.count() + (pool.use & 1u);
    // The other counter (the one of the previous and of the next use) is cleared HERE.  Invariant: a WORKGROUP BARRIER
    // separates the drain of use u from the start of use u + 1 -- every thread takes part in a drain, so program order in
    // thread 0 alone would not do.  Within a call that barrier is the one at the end of the b0 loop below; between two
    // calls it is the caller's barrier between colour phases (every call site has one: the next phase reads what this
    // one wrote).  The clear therefore follows every read of this counter in the previous use's drain, and precedes the
    // barrier of this use, which every push of the next use follows.
    if (pool.cap && threadIdx.x == 0) pool.count()[(pool.use + 1u) & 1u] = 0;
#pragma unroll
    for (int m = 0; m < S; ++m) {
      const uint32_t idx = b0 + m * NT + threadIdx.x;
      if (idx < total) {
        double tau, cen, f = 1.0;
        uint32_t site, off;
        bool neg = false;
        setup(idx, tau, cen, site, off);
        const double kap = vm_clamp(tau), env = vm_envelope(kap);
        bool done = vm_attempt_pair(key, vk, site, 0, kap, env, f, neg);
        if (!done && pool.cap) {
          const uint32_t slot = atomicAdd(cnt, 1u);
          if (slot < pool.cap) {
            pool.kap()[slot] = kap; pool.cen()[slot] = cen; pool.site()[slot] = site; pool.off()[slot] = off;
            continue;  // finished after the barrier, by whichever thread takes the entry
          }
        }
        // no pool, or pool full: retry here
        for (uint32_t pair = 1; !done; ++pair) done = vm_attempt_pair(key, vk, site, pair, kap, env, f, neg);
        commit(off, mod_2pi_fast(vm_angle(f, neg) + cen));
      }
    }
    if (pool.cap) {
      __syncthreads();
      {  // the first threads finish the pooled cells, one each (r03: wave 0 alone, 64 at a time)
        const uint32_t filled = min(*cnt, pool.cap);
        for (uint32_t e = threadIdx.x; e < filled; e += NT) {
          const double k_ = pool.kap()[e], c_ = pool.cen()[e], r_ = vm_envelope(k_);
          const uint32_t s_ = pool.site()[e], o_ = pool.off()[e];
          double f = 1.0;
          bool ng = false;
          for (uint32_t pair = 1; !vm_attempt_pair(key, vk, s_, pair, k_, r_, f, ng); ++pair) {
          }
          commit(o_, mod_2pi_fast(vm_angle(f, ng) + c_));
        }
      }
      ++pool.use;
      // Another pass of this phase follows (more than S NT cells: tiles larger than the default): its pushes reuse the
      // entry arrays the drain above is still reading, so it waits.  (Between two phases the caller's own barrier does that.)
      if (b0 + S * NT < total) __syncthreads();
    }
  }
}

}  // namespace mlmcpi
