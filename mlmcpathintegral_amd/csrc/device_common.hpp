// device_common.hpp -- gfx950 device helpers every translation unit uses: constants, mod_2pi and the lean fp64 primitives,
// the counter-based RNG (Philox4x32-10) with the RNG contract, the LDS reads that stay ds_read_b64 (the tile kernels and the
// step-envelope sampler issue them), and wave64 / workgroup reductions.  Device code only; the CPU
// oracle has its own, independently written restatement.  The samplers built on these live in vonmises.hpp,
// step_envelope.hpp, site_update.hpp and fillin.hpp, and only the units that draw from them include those.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mlmcpi {

constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 6.28318530717958647692;
constexpr int kWave = 64;

// p * x + c with the polynomial coefficient c in an SGPR pair (v_fma_f64 v, v, v, s[..]).  The compiler's own choice
// for fma(p, x, constant) is the two-address v_fmac_f64, which needs the constant copied into the destination VGPR
// pair first (one or two extra VALU instructions per Horner step); with the coefficient on the scalar side the step is
// a single VALU instruction and the copies become scalar moves, which issue beside the vector pipe.
__device__ __forceinline__ double fma_k(double p, double x, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(p), "v"(x), "s"(c));
  return r;
}

// common/auxilliary.hh:42-44, operation for operation (used where the VALUE matters: QoIs)
__device__ __forceinline__ double mod_2pi(double x) { return x - 2. * kPi * floor(0.5 * (x + kPi) / kPi); }

// Same map with the division replaced by a multiplication with 1/(2 pi): 3 fp64 instructions instead
// of ~16 (an fp64 division is a v_rcp_f64 plus two Newton steps plus scale / fixup).  The two forms
// can differ only when (x + pi)/(2 pi) lies within an ulp of an integer, and then by exactly 2 pi,
// i.e. they return the same angle.  Used inside the sweeps, where link angles only ever enter
// 2 pi-periodic functions or another mod_2pi.  Either form returns [-pi, pi] up to the rounding of 2 pi k at magnitude
// |x| + pi: mod_2pi(11 pi rounded up) is pi + 3.6e-15 (tests/test_device_math_gpu.py).
__device__ __forceinline__ double mod_2pi_fast(double x) {
  return fma(-kTwoPi, floor(fma(x, 1.0 / kTwoPi, 0.5)), x);  // 3 instructions: v_fma, v_floor, v_fma
}

// sin(d) for the leapfrog force of the rotor: two-term Cody-Waite reduction to |r| <= pi/2 (exact
// enough for |d| up to ~1e6, far beyond any angle difference a stable trajectory produces) and the
// degree-21 Taylor polynomial (truncation < 1.3e-18): ~20 fp64 instructions, against ~175 for the
// general sin() with its Payne-Hanek path.  Absolute error ~1e-16.
__device__ __forceinline__ double sin_reduced(double d) {
  const double n = rint(d * 0.31830988618379067154);           // d / pi
  double r = fma(-n, 3.14159265358979311600e+00, d);            // pi, high part
  r = fma(-n, 1.22464679914735317723e-16, r);                   // pi - high part
  const double r2 = r * r;
  double p = -1.9572941063391261231e-20;                        // -1/21!
  p = fma_k(p, r2, 8.2206352466243297170e-18);                    //  1/19!
  p = fma_k(p, r2, -2.8114572543455207632e-15);                   // -1/17!
  p = fma_k(p, r2, 7.6471637318198164759e-13);                    //  1/15!
  p = fma_k(p, r2, -1.6059043836821614599e-10);                   // -1/13!
  p = fma_k(p, r2, 2.5052108385441718775e-08);                    //  1/11!
  p = fma_k(p, r2, -2.7557319223985890653e-06);                   // -1/9!
  p = fma_k(p, r2, 1.9841269841269841270e-04);                    //  1/7!
  p = fma_k(p, r2, -8.3333333333333333333e-03);                   // -1/5!
  p = fma_k(p, r2, 1.6666666666666666667e-01);                    //  1/3!
  const double sr = fma(-r * r2, p, r);                          // r - r^3 (1/3! - r^2/5! + ...)
  // (-1)^n: n is an integer-valued double; its parity is the low bit of the converted integer
  return ((long long)n & 1) ? -sr : sr;
}

// cos(pi u) for u in [0, 1]: cos(pi u) = sin(x), x = pi (1/2 - u), |x| <= pi/2; degree-21 Taylor polynomial
// (truncation < 1.3e-18).  15 fp64 instructions against ~175 for the general cos().
__device__ __forceinline__ double cospi_unit(double u) {
  const double x = kPi * (0.5 - u);
  const double x2 = x * x;
  double p = -1.9572941063391261231e-20;                        // -1/21!
  p = fma_k(p, x2, 8.2206352466243297170e-18);                    //  1/19!
  p = fma_k(p, x2, -2.8114572543455207632e-15);                   // -1/17!
  p = fma_k(p, x2, 7.6471637318198164759e-13);                    //  1/15!
  p = fma_k(p, x2, -1.6059043836821614599e-10);                   // -1/13!
  p = fma_k(p, x2, 2.5052108385441718775e-08);                    //  1/11!
  p = fma_k(p, x2, -2.7557319223985890653e-06);                   // -1/9!
  p = fma_k(p, x2, 1.9841269841269841270e-04);                    //  1/7!
  p = fma_k(p, x2, -8.3333333333333333333e-03);                   // -1/5!
  p = fma_k(p, x2, 1.6666666666666666667e-01);                    //  1/3!
  return fma(-x * x2, p, x);                                     // x - x^3 (1/3! - x^2/5! + ...)
}

// cos(x) for |x| < 2^30 (plaquette angles: |x| <= 4 pi): x / (2 pi) reduced to t in [-1/2, 1/2], cos(2 pi t) = cos(pi * 2|t|).
// Absolute error ~|x| 2e-16 + 1e-16: ~25 instructions against ~130 for the general cos() with its Payne-Hanek path.
__device__ __forceinline__ double cos_reduced(double x) {
  const double v = x * (0.5 / kPi);
  const double t = v - rint(v);
  return cospi_unit(2.0 * fabs(t));
}

// ---- lean fp64 primitives for the heat-bath sampler ---------------------------------------------------
// The ocml division / sqrt / acos are correctly rounded over the whole double range (19 / 31 / ~95
// instructions).  The sampler's operands are benign (finite, far from the denormal range), so the
// scaling, fix-up and special-case code is dead weight; these versions keep the Newton / Goldschmidt
// cores only and stay within ~1 ulp.
__device__ __forceinline__ double fast_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  double e = fma(-x, y, 1.0);
  y = fma(y, e, y);
  e = fma(-x, y, 1.0);
  return fma(y, e, y);
}

__device__ __forceinline__ double fast_div(double a, double b) {
  const double y = fast_rcp(b);
  const double q = a * y;
  return fma(fma(-b, q, a), y, q);
}

__device__ __forceinline__ double fast_sqrt(double x) {  // x > 0, normal
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  return fma(fma(-g, g, x), h, g);
}

// acos on [-1, 1] after fdlibm's e_acos.c (rational approximation of (asin(x) - x) / x^3 in z),
// evaluated branch-free: z = x^2 for |x| < 1/2, z = (1 - |x|) / 2 otherwise.
__device__ __forceinline__ double fast_acos(double x) {
  const double ax = fabs(x);
  const bool small = ax < 0.5;
  const double z = small ? x * x : 0.5 * (1.0 - ax);
  double p = 3.47933107596021167570e-05;
  p = fma_k(p, z, 7.91534994289814532176e-04);
  p = fma_k(p, z, -4.00555345006794114027e-02);
  p = fma_k(p, z, 2.01212532134862925881e-01);
  p = fma_k(p, z, -3.25565818622400915405e-01);
  p = fma_k(p, z, 1.66666666666666657415e-01);
  p *= z;
  double q = 7.70381505559019352791e-02;
  q = fma_k(q, z, -6.88283971605453293030e-01);
  q = fma_k(q, z, 2.02094576023350569471e+00);
  q = fma_k(q, z, -2.40339491173441421878e+00);
  q = fma_k(q, z, 1.0);
  const double R = fast_div(p, q);
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
  // |x| < 1/2: pi/2 - (x + x R)
  const double r_small = pio2_hi - (x - (pio2_lo - x * R));
  // |x| >= 1/2: 2 (s + s R) for x > 0, pi - 2 (s + s R) for x < 0, s = sqrt(z)
  const double s = (z > 0.0) ? fast_sqrt(z) : 0.0;
  const double t = fma(s, R, s);
  const double r_large = (x > 0.0) ? 2.0 * t : 2.0 * (pio2_hi - (t - pio2_lo));
  return small ? r_small : r_large;
}

// log(x) for x in (0, 1] (the Box-Muller radius): x = m 2^e with m in [sqrt(1/2), sqrt(2)),
// log m = 2 atanh(s), s = (m - 1)/(m + 1), |s| <= 0.1716: 10 odd terms (< 2e-17 truncation).  ~35
// instructions instead of ~100; relative accuracy also near x = 1, where log -> 0.
__device__ __forceinline__ double log_unit(double x) {
  int e;
  double m = frexp(x, &e);  // m in [0.5, 1)
  if (m < 0.70710678118654752440) {
    m *= 2.0;
    e -= 1;
  }
  const double s = fast_div(m - 1.0, m + 1.0);
  const double z = s * s;
  double p = 1.0 / 19.0;
  p = fma_k(p, z, 1.0 / 17.0);
  p = fma_k(p, z, 1.0 / 15.0);
  p = fma_k(p, z, 1.0 / 13.0);
  p = fma_k(p, z, 1.0 / 11.0);
  p = fma_k(p, z, 1.0 / 9.0);
  p = fma_k(p, z, 1.0 / 7.0);
  p = fma_k(p, z, 1.0 / 5.0);
  p = fma_k(p, z, 1.0 / 3.0);
  p = fma_k(p, z, 1.0);
  return fma((double)e, 0.69314718055994530942, 2.0 * s * p);
}

// (cos, sin)(2 pi v) for v in [0, 1): quadrant from the nearest multiple of 1/4 turn, Taylor kernels on
// |x| <= pi/4, rotation by the quadrant.  ~35 instructions instead of ~190 for sincos().
__device__ __forceinline__ void sincos_2pi_unit(double v, double &sn, double &cs) {
  const double a = 4.0 * v;           // quarter turns, [0, 4)
  const double q = rint(a);           // 0..4
  const double x = (0.5 * kPi) * (a - q);  // |x| <= pi/4
  const double x2 = x * x;
  double sp = -7.6471637318198164759e-13;
  sp = fma_k(sp, x2, 1.6059043836821614599e-10);
  sp = fma_k(sp, x2, -2.5052108385441718775e-08);
  sp = fma_k(sp, x2, 2.7557319223985890653e-06);
  sp = fma_k(sp, x2, -1.9841269841269841270e-04);
  sp = fma_k(sp, x2, 8.3333333333333333333e-03);
  sp = fma_k(sp, x2, -1.6666666666666666667e-01);
  const double s0 = fma(x * x2, sp, x);
  double cp = 4.7794773323873852974e-14;
  cp = fma_k(cp, x2, -1.1470745597729724714e-11);
  cp = fma_k(cp, x2, 2.0876756987868098979e-09);
  cp = fma_k(cp, x2, -2.7557319223985890653e-07);
  cp = fma_k(cp, x2, 2.4801587301587301587e-05);
  cp = fma_k(cp, x2, -1.3888888888888888889e-03);
  cp = fma_k(cp, x2, 4.1666666666666666667e-02);
  cp = fma_k(cp, x2, -0.5);
  const double c0 = fma(cp, x2, 1.0);
  const int k = (int)q & 3;  // rotation by k quarter turns
  const double cr = (k & 1) ? -s0 : c0, sr = (k & 1) ? c0 : s0;
  cs = (k & 2) ? -cr : cr;
  sn = (k & 2) ? -sr : sr;
}

// Box-Muller from two uniforms in [0, 1): radius from 1 - u (in (0, 1]), angle 2 pi v
__device__ __forceinline__ void box_muller(double u, double v, double &n0, double &n1) {
  const double t = -2.0 * log_unit(1.0 - u);
  const double r = (t > 0.0) ? fast_sqrt(t) : 0.0;
  double sn, cs;
  sincos_2pi_unit(v, sn, cs);
  n0 = r * cs;
  n1 = r * sn;
}

// ---- RNG contract ------------------------------------------------------------------
enum Purpose : uint32_t {
  P_MOMENTUM = 1,
  P_ACCEPT = 2,
  P_GFF_NORMAL = 3,
  P_VONMISES = 4,
  P_INIT = 6,
  P_FILLIN = 7,   // two-level step: Gaussian fill-in of the fine-only sites
  P_ACCEPT2 = 8,  // two-level step: Metropolis uniform
  P_BESSEL = 9,   // two-level step, Schwinger coarsened in both directions: Bessel-product fill-in, sub = call counter
  P_EXACT = 10,   // exact Gaussian sampler of the harmonic oscillator: normals of entries (2 m, 2 m + 1) from site m
  P_GAUSSFILL = 13,  // two-level step, Schwinger coarsened in both directions, Gaussian fill-in: sub 0 (xi, omega), 1, 2 normals
  P_SIGMA_HB = 14,   // O(3) sigma model heat bath: (u, v) of vertex l = (projection on the neighbour sum, azimuth), sub 0
  P_CLUSTER_REFLECT = 15,  // cluster update, site 0, step = update counter: xbar = 2 pi u - pi, seed site = min(floor(v M), M - 1)
  P_CLUSTER_BOND = 16,     // cluster update, site l >> 1, step = update counter: u decides link l even, v link l odd
  P_GAUGE = 17,            // Schwinger cluster draw, site vertex >> 1, step = draw counter: g = 2 pi (u | v by parity) - pi
  P_SWEEP_ORDER = 18,      // random-order sweep (random_sweep.hip), site l >> 2, step = the sweep's counter, sub 0: word l & 3 of the
                           // call is the 32-bit key of index l; the sweep visits the indices of a chain in ascending (key, l)
  P_SIGMA_REFLECT = 19,    // sigma-model Wolff update (sigma_cluster.hip), site 0, step = update counter: sub 0 (u, v) -> normal r with
                           // r_z = 1 - 2 u, azimuth 2 pi v - pi; sub 1 u -> seed vertex min(floor(u N), N - 1) (N: the level's vertices)
  P_SIGMA_BOND = 20,       // sigma-model Wolff update, site = vertex l, step = update counter, sub 0: u decides link (l, 0) (to the +i
                           // neighbour), v decides link (l, 1) (to the +j neighbour).  On a rotated level (sigma_cluster.hip):
                           // site = the E vertex e of the link, sub d >> 1 (0 or 1): u decides link (e, d) for d even, v for d odd
  P_SIGMA_SW_REFLECT = 21, // sigma-model Swendsen-Wang update (sigma_sw.hip), site 0, step = update counter, sub 0: (u, v) -> normal r
                           // by the map of purpose 19 sub 0
  P_SIGMA_SW_BOND = 22,    // Swendsen-Wang update, site = vertex l, sub 0: u decides link (l, 0), v decides link (l, 1).  On a rotated
                           // level (sigma_sw.hip): site = the E vertex e of the link, sub d >> 1: u decides link (e, d) for d even,
                           // v for d odd
  P_SIGMA_SW_FLIP = 23,    // Swendsen-Wang update, site = the root (smallest vertex; on a rotated level the smallest LEVEL index) of a
                           // cluster, sub 0: reflected iff u < 0.5
  P_SIGMA_FILLIN = 24,     // sigma-model two-level step (sigma_twolevel.hip), site = the fine-only vertex's index on the fine level, sub 0:
                           // (u, v) of its heat-bath draw from the four coarse neighbours
};

struct RngKey {
  uint32_t k0, k1;  // seed low / high word
  uint32_t chain;   // global chain index
  uint32_t step;    // sweep or trajectory counter
};

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one v_mad_u64_u32 per product (hi and lo together) instead of v_mul_hi_u32 + v_mul_lo_u32
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    c1 = (uint32_t)p1;
    c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

// Round keys in VECTOR registers.  MI355X issues a 32-bit VALU instruction whose operands are all VGPRs (or literals) at
// 2.4 - 2.8 cycles per wave, the same instruction with an SGPR operand at 4.1 (tools/valu_issue_bench.hip,
// profiles/r04_valu_issue_cost.txt: v_xor_b32 2.4 / 4.1, v_bitop3_b32 2.8 / 4.1).  The compiler keeps wave-uniform values --
// the round keys -- in SGPRs, where the scalar unit bumps them for free, and pays for that in every one of the 2 x 10
// key xors of a call.  Here the keys of rounds 2 .. 9 sit in 16 VGPRs (an opaque v_mov, so that they stay there) and a
// round's  hi ^ counter ^ key  is ONE three-input v_bitop3_b32: 16 instructions at 2.8 cycles instead of 32 at 2.4 / 4.1.
// Rounds 0 and 1 stay as they are: half of their operands are uniform and fold away on the scalar side.  Same function.
struct PhiloxVKeys { uint32_t k[16]; };
__device__ __forceinline__ uint32_t to_vgpr(uint32_t s) {
  uint32_t v;
  asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}
__device__ __forceinline__ PhiloxVKeys philox_vkeys(uint32_t k0, uint32_t k1) {
  PhiloxVKeys vk;
#pragma unroll
  for (int r = 2; r < 10; ++r) {
    vk.k[2 * (r - 2)] = to_vgpr(k0 + (uint32_t)r * 0x9E3779B9u);
    vk.k[2 * (r - 2) + 1] = to_vgpr(k1 + (uint32_t)r * 0xBB67AE85u);
  }
  return vk;
}
__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                            const PhiloxVKeys &vk) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    if (r < 2) {
      c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
      c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    } else {
      c0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, vk.k[2 * (r - 2)], 0x96);       // a ^ b ^ c
      c2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, vk.k[2 * (r - 2) + 1], 0x96);
    }
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ double u01(uint32_t lo, uint32_t hi) {
  uint64_t v = ((uint64_t)hi << 32) | lo;
  return (double)(v >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ void rng_uniforms(const RngKey &k, uint32_t site, uint32_t purpose, uint32_t sub,
                                             double &a, double &b) {
  U4 r = philox4x32_10(site, k.chain, k.step, (purpose << 24) | (sub & 0xFFFFFFu), k.k0, k.k1);
  a = u01(r.x, r.y);
  b = u01(r.z, r.w);
}

__device__ __forceinline__ void rng_normals(const RngKey &k, uint32_t site, uint32_t purpose, uint32_t sub,
                                            double &n0, double &n1) {
  double u, v;
  rng_uniforms(k, site, purpose, sub, u, v);
  box_muller(u, v, n0, n1);
}

// the same with the round keys in vector registers (philox_vkeys: hot loops that draw once per cell)
__device__ __forceinline__ void rng_normals(const RngKey &k, const PhiloxVKeys &vk, uint32_t site, uint32_t purpose, uint32_t sub,
                                            double &n0, double &n1) {
  const U4 r = philox4x32_10(site, k.chain, k.step, (purpose << 24) | (sub & 0xFFFFFFu), k.k0, k.k1, vk);
  box_muller(u01(r.x, r.y), u01(r.z, r.w), n0, n1);
}

// cosine branch only (one normal per call)
__device__ __forceinline__ double rng_normal0(const RngKey &k, uint32_t site, uint32_t purpose, uint32_t sub) {
  double u, v, n0, n1;
  rng_uniforms(k, site, purpose, sub, u, v);
  box_muller(u, v, n0, n1);  // (the unused sine branch is dead code the compiler removes)
  return n0;
}

// ---- LDS reads that stay ds_read_b64 ---------------------------------------------------------------------
// hipcc merges neighbouring 8-byte LDS loads into ds_read2_b64, which the LDS serves at a quarter of the
// ds_read_b64 rate (MI355X_MICROARCH.md, LDS table: 16 cycles for 16 bytes per lane against 2 x 2).  The
// stencil kernels are LDS-issue bound, so their loads are issued through inline asm, which the merger
// does not see.  The caller issues a group of reads and then ONE lds_wait7() before the first use (the
// compiler does not track inline-asm loads, cdna_hip_programming.md 5.7).  `addr` is the LDS byte address
// (the callers add the LDS address of their dynamic array: the low word of a flat LDS address is the LDS offset).
template <int OFF>
__device__ __forceinline__ double lds_read_f64(uint32_t addr) {
  double v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
// The wait names every loaded value as an in/out operand: the compiler sees the asm outputs of the reads
// as ready immediately and would otherwise schedule their consumers ABOVE the s_waitcnt.
__device__ __forceinline__ void lds_wait7(double &a, double &b, double &c, double &d, double &e, double &f, double &g) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g) : : "memory");
}

// the same for the six values of a heat-bath stencil, and for those of two cells at once
__device__ __forceinline__ void lds_wait6(double (&a)[6]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]) : : "memory");
}
__device__ __forceinline__ void lds_wait12(double (&a)[6], double (&b)[6]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                 "+v"(b[4]), "+v"(b[5])
               :
               : "memory");
}

// ---- reductions -------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;  // valid in lane 0
}

// Sum over the workgroup in a fixed order (lane tree, then waves 0..n-1): bitwise reproducible.
// `scratch` needs blockDim.x/64 doubles per value.  Result valid in thread 0.
// Rotate a value through the 64 lanes of a wave by one lane (DPP wave_ror:1 / wave_rol:1, gfx9 family): no LDS, no
// barrier.  "up": lane l receives the value of lane l - 1 and lane 0 that of lane 63; "down": lane l receives lane l + 1.
__device__ __forceinline__ double wave_rotate_up(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x13C, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x13C, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_rotate_down(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x134, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x134, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *scratch) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwave = (blockDim.x + kWave - 1) / kWave;
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) scratch[q * nwave + wave] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      double s = 0.0;
      for (int w = 0; w < nwave; ++w) s += scratch[q * nwave + w];
      v[q] = s;
    }
  }
}

// what a 2-D lattice reduction sums: the sweep kernels (fused QoI) and the kernels of lattice_reduce.hip share the numbering
enum LatOp { L_GFF_ENERGY = 0, L_PHI2 = 1, L_SCHW_ENERGY = 2, L_PLAQ = 3, L_CHARGE = 4 };

// The state a launch writes is read next by another launch, from HBM either way (one chain's state is 16 MiB against 4 MiB of
// L2 per XCD): a non-temporal store keeps it from pushing the halos the resident workgroups share out of the L2
// (measured on the one-launch Schwinger draw: -3.5 %).
__device__ __forceinline__ void store_streaming(double2 *p, double x, double y) {
  typedef double d2_t __attribute__((ext_vector_type(2)));
  const d2_t v = {x, y};
  __builtin_nontemporal_store(v, reinterpret_cast<d2_t *>(p));
}

// stats->record_sample of one value into a chain's packed sums a[5] = [n, sum v, sum v^2, sum v^3, sum v^4]: the one recurrence of
// mlmcpi_stats_accumulate and of every kernel that records a QoI it has just finished.  The roundings are spelled out (one fused
// multiply-add per sum, on products rounded on their own), so that a unit compiled without fp contraction records the same bits as
// one compiled with it: a fused record equals mlmcpi_stats_accumulate on the same value whatever kernel wrote it.
__device__ __forceinline__ void record_moments(double *a, double v) {
  const double v2 = __dmul_rn(v, v), v3 = __dmul_rn(v, v2);
  a[0] += 1.0;
  a[1] += v;
  a[2] = __fma_rn(v, v, a[2]);
  a[3] = __fma_rn(v, v2, a[3]);
  a[4] = __fma_rn(v, v3, a[4]);
}

}  // namespace mlmcpi
