// step_envelope.hpp -- the von Mises sampler with a tabulated step envelope, for launches whose concentrations stay below
// kVsKappaMax: the table's layout (host and device; step_envelope_tables.hip builds it), one attempt pair, and the colour phases that draw
// a workgroup's cells with it.  Included by site_update.hpp and lattice_sweep.hpp, and by schwinger_sweeps.hip,
// rotor_sweeps.hip, lattice2d.hip, random_sweep.hip, step_envelope_tables.hip and test_hooks.hip.
#pragma once
#include "device_common.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// ---- heat-bath angle draws, tabulated step envelope (launches whose concentrations stay below kVsKappaMax) ----------
// The wrapped-Cauchy sampler above pays, per draw, an envelope square root, a division and an fp64 cosine per attempt
// and an arccosine for the accepted one: ~300 fp64-class instructions of a ~520-instruction cell (388 lane
// instructions per link update, the heat bath = half the step).  For moderate concentrations -- the Schwinger model at
// beta <= 8, the rotor at 2 m0 / a <= 16 (kVsKappaMax): every BASELINE configuration -- the same von Mises law p(x) ~ exp(kappa cos x)
// is drawn here from a piecewise-constant envelope taken from a small table, so that an attempt costs no fp64
// arithmetic at all and the accepted angle is a linear function of random bits:
//     bins of |x|     edges (0, 1, 2, 3, 4, 6, 8, 12, 16) pi/16: eight bins, finer where the density is high;
//     bin k is proposed with probability q_k / 64 (six random bits through a 64-entry selector), |x| uniform inside it
//                     (35 random bits), sign from one more bit;
//     accepted with probability  exp(kappa (cos x - 1)) 2^lw[k],   2^lw[k] = (w_k / q_k) / max_j (H_j w_j / q_j),
// i.e. target / (proposal density x envelope constant), H_j = the target at the left edge of bin j (its maximum there).
// The q_k follow the shape of the target, which depends on kappa; so there are kVsClasses tables, for eight ranges of
// kappa, and a cell picks its table by an exact fp64 comparison: with t = |(x_m - x_p)/(4 pi)| reduced to [0, 1/2],
// kappa = scale |cos(2 pi t)| = scale sin(2 pi v), v = |t - 1/4| in [0, 1/4], class = floor(32 v): the table of class c
// is built for kappa_min = scale sin(2 pi c / 32) and is a valid envelope for every larger kappa (the normalised target
// only gets narrower).  Acceptance 0.70 ... 0.89 (0.79 on average; wrapped Cauchy: 0.82).  The tables are built by the
// host for the action's scale (step_envelope_tables.hip, vs_build_tables; exported as mlmcpi_vs_table so that the oracle's own
// construction can be compared with it) and copied to LDS by the kernels: 512 selector bytes + 8 x 16 floats.
// The test is screened in fp32 (24 bits of |x|, one polynomial cosine, v_exp_f32) against the kVsU2Bits = 22 leading bits of
// u2 with a guard band that covers every fp32 rounding on the way; when the band does not decide (one attempt in ~3 10^4),
// the exact fp64 test with the full u2 takes over, as for the wrapped-Cauchy sampler, so the decision is always the one of
// the exact test -- which is what the oracle computes (oracle.cc, dev_vonmises_table).  (With 11 leading bits, as the
// wrapped-Cauchy sampler has them, one attempt in 2048 was open and 4-6 % of the wave iterations took the detour through
// the exact test -- a Philox call, an fp64 logarithm and cosine behind a function call: measured at 8 % of the fused
// sweep launch.)  Random numbers: the same Philox calls (word pair = one attempt), fields: bit 0 sign, bits 1..22 leading
// bits of u2, bits 23..57 position inside the bin (35 bits: 2 10^-11 rad), bits 58..63 selector.
// host rule (lattice2d.hip / rotor_sweeps.hip; the oracle applies the same): this sampler where the action's largest concentration,
// 2 beta or 2 m0 / a, is <= kVsKappaMax; the wrapped-Cauchy sampler beyond.  r05: 16 (4 until then).  The eight classes split
// [0, scale] by sin(2 pi c / 32), so they get wider in kappa with the scale and a table, built for the smallest
// concentration of its class, fits the largest one less well: acceptance per attempt 0.78 on average at scale 2, 0.74 at 4,
// 0.67 at 8, 0.59 at 12, 0.58 at 16 (0.24 at worst), a pair fails for 5 / 7 / 11 / 18 / 20 % of the cells.  Even so a draw of
// the fused Schwinger launch (1024^2 x 32) takes 0.70 ms at beta = 4, 0.82 at 6 and 0.75 at 8 against 1.18 - 1.19 ms with the
// wrapped-Cauchy sampler; beyond 16 the eight bins (the finest pi / 16 wide) are too coarse for the target.  The error
// budget of the screening test below scales with kappa' = scale log2 e through the band, and |log2 a| <= 2 kappa' + |lw| <= 55
// is far from fp32's exponent range.
constexpr double kVsKappaMax = 16.0;
constexpr int kVsClasses = 8, kVsBins = 8, kVsSel = 64;
constexpr uint32_t kVsU2Bits = 22;  // leading bits of the acceptance uniform carried by the attempt itself
// The 64 bits (lo, hi) of an attempt (r04 layout: every field is one shift or one conversion away from its use):
//   lo[31..10]  b, the 22 leading bits of the acceptance uniform u2 = (b + tail) / 2^22 (tail: the refine call, rarely);
//               (float)lo is u2 2^32 to within 2^10, which is all the screening test needs
//   lo[9]       sign of the angle
//   lo[8..0]    the low 9 of the 35 position bits
//   hi[31..26]  bin selector
//   hi[25..0]   the high 26 position bits; (float)(hi << 6) is the position 2^32, rounded to 24 bits
// Device image of the tables (bytes; built by the host for the action's scale, step_envelope_tables.hip vs_device_image):
//   code[class][64]   1 B   8 x (bin of the selector value): a byte offset into the next two tables
//   scr[bin]          8 B   float2 {pi/2 - edge, -width 2^-32}: y = pi/2 - |x| = fma(scr.y, (float)(hi << 6), scr.x), cos|x| = sin y
//   lw[class][bin]    8 B   float log2 of the bin's acceptance factor (+ 4 B of padding: lw and code share the class offset 64 cls)
//   fin[bin]          16 B  double2 {64 width, edge - 64 width} in units of pi/16: |x| = (pi/16) fma(fin.x, m, fin.y), m = 1 + position / 64
//   consts            16 B  float {s_acc, s_rej, 0, 0}: thresholds of the screening test for this scale (below)
constexpr uint32_t kVsCodeOff = 0, kVsScrOff = 512, kVsLwOff = 576, kVsFinOff = 1088, kVsConstOff = 1216, kVsTableBytes = 1232;
// host side of the same encoding: left edge and width of bin k in units of pi/16 (edges 0 1 2 3 4 6 8 12, widths 1 1 1 1 2 2 4 4)
__host__ __device__ constexpr uint32_t vs_edge16(uint32_t k) { return (0xC8643210u >> (4u * k)) & 15u; }
__host__ __device__ constexpr uint32_t vs_width16(uint32_t k) { return (0x44221111u >> (4u * k)) & 15u; }
// Screening test.  a = the acceptance probability in fp32 (error budget below), L = (float)lo.  The exact u2 2^32 lies within
// 2^10 (1 + 2^-22) of L, so
//     accepted for sure   L <= a 2^32 (1 - band) - kVsU2Slack,       rejected for sure   L >= a 2^32 (1 + band) + kVsU2Slack;
// neither: the exact fp64 test with the full u2 decides (one attempt in ~10^4).  Error budget of log2(a): |x| to 24 bits
// (1e-7 kappa'), the sine polynomial (1.2e-7 kappa'), kappa' itself (2e-7 kappa' from the fp32 cosine behind it), the fma (1e-6
// at |log2 a| <= 16): < 4e-7 (1 + kappa'), i.e. < 3e-7 (1 + kappa') relative on a, plus v_exp_f32's own ~2e-7 and 2^-23 for
// the conversion of lo and the threshold's own rounding.  The band is 1e-5 (1 + kappa'_max) for the whole launch (kappa'_max =
// scale log2 e): more than 20 times that, and two constants (s_acc = 2^32 (1 - band), s_rej = 2^32 (1 + band)) instead of
// five instructions per cell.
constexpr float kVsU2Slack = 1100.0f;
__host__ __device__ inline float vs_band_of_scale(double scale) { return (float)(1e-5 * (1.0 + scale * 1.4426950408889634)); }

struct VsTable {
  const uint8_t *base;   // LDS in the sweeps; global memory in the site-at-a-time kernels and the test hook
  float s_acc, s_rej;
  __device__ static VsTable at(const void *image, const uint32_t *__restrict__ d_table) {
    VsTable t{(const uint8_t *)image, 0.f, 0.f};
    if (d_table) {  // uniform address: scalar loads; then into vector registers, where a v_fma_f32 on them issues at full rate
      t.s_acc = __uint_as_float(to_vgpr(d_table[kVsConstOff / 4]));
      t.s_rej = __uint_as_float(to_vgpr(d_table[kVsConstOff / 4 + 1]));
    }
    return t;
  }
  // the workgroup copies the action's table from global memory (visible after the caller's next barrier)
  __device__ static VsTable stage(void *lds, const uint32_t *__restrict__ d_table) {
    if (d_table)
      for (uint32_t i = threadIdx.x; i < kVsTableBytes / 4; i += blockDim.x) ((uint32_t *)lds)[i] = d_table[i];
    return at(lds, d_table);
  }
  __device__ static VsTable in_global(const uint32_t *__restrict__ d_table) { return at(d_table, d_table); }
};

// sin(y), |y| <= pi/2, fp32: odd minimax polynomial of degree 9 (approximation error 4.6e-9; 1.2e-7 with the fp32 rounding,
// measured over 2 10^6 arguments -- the degree-11 Taylor polynomial this replaces: 1.6e-7)
__device__ __forceinline__ float sinf_half_pi(float y) {
  const float y2 = y * y;
  float p = 2.600053086e-06f;
  p = fmaf(p, y2, -1.980661437e-04f);
  p = fmaf(p, y2, 8.333017279e-03f);
  p = fmaf(p, y2, -1.666665710e-01f);
  return fmaf(y * y2, p, y);
}

struct VsCell {
  double centre;   // the draw is mod_2pi(centre +- |x|)
  float kp;        // kappa log2(e), fp32: screening only
  uint32_t cls;    // 64 x (which table): the byte offset of the class in code[][] and lw[][]
  uint32_t site;   // Philox counter word 0
};

// Cell set-up shared by the Schwinger links (x_p, x_m = the two staple sums, scale = 2 beta) and the rotor sites
// (x_p, x_m = the neighbours, scale = 2 m0 / a): conditional exp(scale/2 [cos(x - x_p) + cos(x - x_m)])
// = exp(kappa cos(x - centre)), kappa = scale |cos((x_m - x_p)/2)|, centre = (x_p + x_m)/2 (+ pi where the cosine is
// negative, i.e. for t > 1/4: an exact fp64 comparison); kappa itself is needed in fp32 only.
__device__ __forceinline__ void vs_cell(double scale, double x_p, double x_m, VsCell &c) {
  const double v = (x_m - x_p) * (0.25 / kPi);
  const double t = fabs(v - rint(v));
  c.centre = fma(0.5, x_p + x_m, t > 0.25 ? kPi : 0.0);
  const double w = fabs(t - 0.25);                                          // [0, 1/4]; NaN for a NaN state
  c.cls = min((uint32_t)(32.0 * w), (uint32_t)(kVsClasses - 1)) * kVsSel;  // (uint32_t)NaN = 0
  // |cos(2 pi t)| = |sin(pi/2 - 2 pi t)|, t in [0, 1/2]
  c.kp = fmaxf((float)scale * fabsf(sinf_half_pi(fmaf(-6.28318531f, (float)t, 1.57079633f))), 0.0f) * 1.44269504f;   // fmaxf: NaN -> 0
}
__device__ __forceinline__ double vs_kappa_exact(double scale, double x_p, double x_m) {
  return vm_clamp(scale * fabs(cos_half(x_m - x_p)));
}

// |x| of the attempt (lo, hi), fp64: (pi/16) (edge + width pos), pos = the 35 position bits / 2^35; code = 8 x the bin
__device__ __forceinline__ double vs_theta(uint32_t lo, uint32_t hi, uint32_t code, const VsTable &tab) {
  // mantissa = 000000 | 26 bits of hi | 9 bits of lo | 11 zeros: m = 1 + pos / 64
  const double m = __hiloint2double((int)(((hi >> 12) & 0x3FFFu) | 0x3FF00000u), (int)__builtin_amdgcn_alignbit(hi, lo << 23, 12));
  const double2 f = *(const double2 *)(tab.base + kVsFinOff + 2u * code);
  return (kPi / 16.0) * fma(f.x, m, f.y);   // edge + width pos is exact in fp64: one rounding, as in the oracle
}

// acceptance probability of one attempt in fp32; the bin's code comes back for the caller
__device__ __forceinline__ float vs_accept_prob(uint32_t hi, float kp, uint32_t cls, const VsTable &tab, uint32_t &code) {
  const uint8_t *row = tab.base + cls;   // the class's rows of code[][] and (kVsLwOff further on) of lw[][]
  code = row[hi >> 26];
  const float2 scr = *(const float2 *)(tab.base + kVsScrOff + code);
  const float sn = sinf_half_pi(fmaf(scr.y, (float)(hi << 6), scr.x));   // cos|x|
  return __builtin_amdgcn_exp2f(fmaf(kp, sn - 1.0f, *(const float *)(row + kVsLwOff + code)));
}

// the exact test: u2 = (b + tail) / 2^22 against exp(kappa (cos x - 1)) 2^lw, in logarithms
__device__ __forceinline__ int vs_exact(uint32_t lo, uint32_t hi, uint32_t code, double tail, double kappa, float lw, const VsTable &tab) {
  const double u2 = ((double)(lo >> (32 - kVsU2Bits)) + tail) * (1.0 / (double)(1u << kVsU2Bits));
  const double la = fma(kappa, cospi_unit(vs_theta(lo, hi, code, tab) * (1.0 / kPi)) - 1.0, 0.69314718055994531 * (double)lw);
  return (u2 <= 0.0 || log_unit(u2) <= la) ? 1 : 0;
}

// The open decisions of a pair of attempts, taken exactly (one attempt in ~10^4 gets here).  Not inlined: the fp64
// polynomial coefficients of this path would otherwise be hoisted into scalar registers for the whole kernel and push
// the hot loop's own constants out (the hot loop then reloads them with v_readlane every iteration).
__device__ __attribute__((noinline)) uint32_t vs_exact_pair(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t step, uint32_t site,
                                                            uint32_t w3, U4 q, uint32_t codes, float lwa, float lwb, double kappa,
                                                            int sa, int sb, const uint8_t *tab_base) {
  const VsTable tab{tab_base, 0.f, 0.f};
  const U4 e = philox4x32_10(site, chain, step, w3 | kVmRefine, k0, k1);
  if (sa < 0) sa = vs_exact(q.x, q.y, codes & 0xFFu, u01(e.x, e.y), kappa, lwa, tab);
  if (sa == 0 && sb < 0) sb = vs_exact(q.z, q.w, codes >> 8, u01(e.z, e.w), kappa, lwb, tab);
  return (uint32_t)(sa & 3) | ((uint32_t)(sb & 3) << 2);   // two's complement in two bits each: 3 = open (cannot remain), 1, 0
}

// attempts 2 pair and 2 pair + 1 of `site`; kappa_exact() is evaluated only when a screening decision is open.
// Returns true when one of them is accepted (or the attempt bound is hit); |x| and its sign come back either way.
template <class KappaExact>
__device__ __forceinline__ bool vs_attempt_pair(const RngKey &k, const PhiloxVKeys *vk, uint32_t site, uint32_t pair, float kp, uint32_t cls,
                                                const VsTable &tab, KappaExact kappa_exact, double &theta, bool &negative,
                                                uint32_t sub0 = 0) {
  const uint32_t w3 = (P_VONMISES << 24) | sub0 | pair;
  // vk == NULL (a compile-time fact at every call site): round keys on the scalar side -- 16 VGPRs less, for kernels that
  // live on occupancy
  const U4 q = vk ? philox4x32_10(site, k.chain, k.step, w3, k.k0, k.k1, *vk) : philox4x32_10(site, k.chain, k.step, w3, k.k0, k.k1);
  uint32_t ca, cb;
  const float pa = vs_accept_prob(q.y, kp, cls, tab, ca), pb = vs_accept_prob(q.w, kp, cls, tab, cb);
  const float la = (float)q.x, lb = (float)q.z;
  bool acc_a = la <= fmaf(pa, tab.s_acc, -kVsU2Slack), acc_b = lb <= fmaf(pb, tab.s_acc, -kVsU2Slack);  // lane masks
  if (!acc_a) {
    const bool rej_a = la >= fmaf(pa, tab.s_rej, kVsU2Slack), rej_b = lb >= fmaf(pb, tab.s_rej, kVsU2Slack);
    // open: the first attempt undecided, or rejected and the second undecided
    if (!rej_a || (!acc_b && !rej_b)) {
      const uint8_t *row = tab.base + cls + kVsLwOff;
      const uint32_t r = vs_exact_pair(k.k0, k.k1, k.chain, k.step, site, w3, q, ca | (cb << 8), *(const float *)(row + ca),
                                       *(const float *)(row + cb), kappa_exact(), rej_a ? 0 : -1, acc_b ? 1 : rej_b ? 0 : -1, tab.base);
      acc_a = (r & 3u) == 1u;
      acc_b = (r >> 2) == 1u;
    }
  }
  const bool first = acc_a;
  const uint32_t lo = first ? q.x : q.z, hi = first ? q.y : q.w;
  theta = vs_theta(lo, hi, first ? ca : cb, tab);
  negative = (lo & 0x200u) != 0;
  return acc_a || acc_b || pair + 1 >= kMaxVmPairs;
}

// Open cells of a step-envelope colour phase.  After the first pair of attempts ~5 % of the cells are still open.  Retrying
// them where they sit makes every wave run the whole attempt code again and again with two or three live lanes.  Instead
// they go on a list in LDS -- an entry is just the cell's LDS offset and the index of its next pair; stencil, centre and
// kappa are recomputed from the tile image, which the phase does not change under the cell -- and behind ONE barrier the
// first threads of the workgroup take one entry each and finish it where it is, however many pairs that takes.
// (r03 worked the list off in rounds -- one pair per entry, what is still open onto a second list, a barrier, and so on
// until a round fitted one wave: with ~110 entries per phase that was a barrier and a round more than this, and 7 % of
// the fused launch.  Measured on one box, r04: 0.8175 ms with rounds down to 64 entries, 0.7863 down to 128, 0.7626 with
// none, profiles/r04_ab_tail.txt.  Handing the cells of a phase out through a queue, so that retries ride along with
// fresh cells and no list is needed until the queue runs dry, was built and measured too: 3 % slower than the rounds --
// the returning atomic and the hand-out arithmetic per wave and iteration cost more than the rounds they replace.)
template <class E>  // uint16_t: offset in 12 bits, next pair in 4 (compile-time 64 x 32 tiles); uint32_t: 16 + 16
struct VsPool {
  static constexpr uint32_t kOffBits = sizeof(E) == 2 ? 12 : 16;
  static constexpr uint32_t kMaxPair = (1u << (8 * sizeof(E) - kOffBits)) - 1;
  E *buf;                // `cap` entries
  uint32_t *count;       // [2]: list lengths of even / odd uses
  uint32_t cap, use;     // capacity (0: no list, every cell is finished by its own lane); uses so far (uniform)
  VsTable tab;
  // LDS bytes: table | counters | list
  static __host__ __device__ constexpr size_t bytes(uint32_t cap) { return kVsTableBytes + 16 + ((size_t)cap * sizeof(E) + 7) / 8 * 8; }
  // call from every thread; visible after the caller's next barrier.  d_table == NULL: a kernel instance that never draws
  // from the step envelope -- nothing in LDS is touched.
  __device__ static VsPool carve(double *lds, uint32_t cap, const uint32_t *d_table) {
    VsPool p;
    p.tab = VsTable::stage(lds, d_table);
    p.count = (uint32_t *)((uint8_t *)lds + kVsTableBytes);
    p.buf = (E *)(p.count + 4);
    p.cap = cap;
    p.use = 0;
    if (d_table && threadIdx.x < 2) p.count[threadIdx.x] = 0;
    return p;
  }
};

// One colour phase.  off_of(idx) = LDS offset of cell idx of the phase; setup(off, cell) = centre, class, kappa', Philox
// site from the tile image; kappa_exact(off) = the fp64 concentration (rare); commit(off, angle).  The caller puts a
// barrier behind the call (every call site has one: the next phase reads what this one wrote).
// Pass 0 walks the cells of the phase (thread t: cells t, t + NT, ...), pass 1 the list (the rare exact test is a function
// call, vs_exact_pair, so that the two copies of the attempt code stay small).  S (cells per thread and pass of
// heatbath_cells, whose signature the call sites share) is not used here.
// LEAN (the 1-D rotor sweeps, whose 256-thread workgroups live on occupancy): one copy of the cell code with a run-time flag and
// the round keys on the scalar side -- 59 instead of 97 VGPRs, 7 instead of 4 waves per SIMD (the fast form cost the rotor
// sweeps 10 %; it gains the fused Schwinger launch, which LDS holds at 4 waves per SIMD anyway, 3 %).
template <int NT, int S, class E, int LEAN = 0, class OffOf, class Setup, class KappaExact, class Commit>   // LEAN: 1 = scalar round keys, 2 = + one copy of the cell code
__device__ __forceinline__ void heatbath_cells_step(uint32_t total, const RngKey &key, VsPool<E> &pool, OffOf off_of, Setup setup,
                                                    KappaExact kappa_exact, Commit commit) {
  using P = VsPool<E>;
  constexpr uint32_t kOffMask = (1u << P::kOffBits) - 1;
  uint32_t *const cnt = pool.count + (pool.use & 1u);
  // the counter of the NEXT use: last read in the previous use, which ended before the caller's barrier behind it
  if (pool.cap && threadIdx.x == 0) pool.count[(pool.use & 1u) ^ 1u] = 0;
  PhiloxVKeys vk_;
  if (!LEAN) vk_ = philox_vkeys(key.k0, key.k1);
  const PhiloxVKeys *const vk = LEAN ? nullptr : &vk_;
  // One cell: pairs of attempts until one is accepted -- or, with on_list, one pair and then onto the list.  Two copies of
  // this (pass 0 and pass 1) on purpose: with one copy and run-time flags the hot loop of pass 0 carries the list's
  // branches and loads (measured: +2.4 % on the fused launch).
  auto cell = [&](uint32_t off, uint32_t pair, auto on_list) {
    VsCell c;
    setup(off, c);
    double th = 0.0;
    bool neg = false;
    for (;;) {
      if (vs_attempt_pair(key, vk, c.site, pair, c.kp, c.cls, pool.tab, [&] { return kappa_exact(off); }, th, neg)) {
        commit(off, mod_2pi_fast(c.centre + (neg ? -th : th)));
        return;
      }
      ++pair;
      if ((bool)on_list && pair == 1 && pool.cap) {   // (kMaxPair >= 1: the entry can hold it)
        const uint32_t slot = atomicAdd(cnt, 1u);
        if (slot < pool.cap) {
          pool.buf[slot] = (E)(off | (pair << P::kOffBits));
          return;
        }
      }
    }
  };
  // Pass 0 takes whole rounds of NT cells only: the cells left over (130 of the 2178 of a phase of the fused kernel, NT =
  // 512) would cost the first waves a fifth iteration with the others waiting at the barrier; they join the list instead,
  // where threads are idle anyway.
  const uint32_t n_main = pool.cap ? total / NT * NT : total;
  if (LEAN >= 2) {   // one loop over both passes, one copy of the cell code
    uint32_t n = n_main, n_list = 0;
    for (int pass = 0; pass < 2; ++pass) {
      for (uint32_t i = threadIdx.x; i < n; i += NT) {
        uint32_t off, pair = 0;
        if (pass == 0) {
          off = off_of(i);
        } else if (i < n_list) {
          const uint32_t e = pool.buf[i];
          off = e & kOffMask;
          pair = e >> P::kOffBits;
        } else {
          off = off_of(n_main + (i - n_list));
        }
        cell(off, pair, pass == 0);
      }
      if (!pool.cap) break;
      if (pass == 0) {
        __syncthreads();
        n_list = min(*cnt, pool.cap);
        n = n_list + (total - n_main);
      }
    }
    ++pool.use;
    return;
  }
  for (uint32_t i = threadIdx.x; i < n_main; i += NT) cell(off_of(i), 0u, std::true_type{});
  if (pool.cap) {
    __syncthreads();
    const uint32_t n_list = min(*cnt, pool.cap);   // (the same value in every thread: nothing is pushed behind the barrier)
    const uint32_t n = n_list + (total - n_main);
    for (uint32_t i = threadIdx.x; i < n; i += NT) {
      uint32_t off, pair = 0;
      if (i < n_list) {
        const uint32_t e = pool.buf[i];
        off = e & kOffMask;
        pair = e >> P::kOffBits;
      } else {
        off = off_of(n_main + (i - n_list));
      }
      cell(off, pair, std::false_type{});
    }
  }
  ++pool.use;
}

// The same colour phase for callers that know a closed-form map thread -> cells (the fused Schwinger launch: a wave takes
// whole rows of the tile image).  heatbath_cells_step above hands out cells by their linear index, so every cell pays an
// integer division for its (row, column), a second one inside setup() for the Philox site, and the wraps of both
// coordinates: ~30 integer instructions of a ~200-instruction cell.  Here pass 0 is NIT rounds of NT cells whose LDS offset
// and Philox site the caller advances itself -- main_cell(off, site) is called NIT times by every thread, in order -- and
// only what the map leaves over (n_left cells: left_off(i), i < n_left) joins the list pass, whose cells get their site from
// site_of(off) as before.  Which cell a lane works on does not enter any result (a cell's random numbers are fixed by
// (site, attempt)): bit for bit the results of heatbath_cells_step.  stencil_load(off, v) issues the six reads of the cell's
// stencil (lds_read_f64: no wait), stencil_cell(v, cell) = centre, class, kappa' from them (not the site).
template <int NT, int NIT, class E, class Main, class Left, class SiteOf, class StencilLoad, class StencilCell, class KappaExact, class Commit>
__device__ __forceinline__ void heatbath_cells_step_mapped(uint32_t n_left, const RngKey &key, VsPool<E> &pool, Main main_cell, Left left_off,
                                                           SiteOf site_of, StencilLoad stencil_load, StencilCell stencil_cell,
                                                           KappaExact kappa_exact, Commit commit) {
  using P = VsPool<E>;
  constexpr uint32_t kOffMask = (1u << P::kOffBits) - 1;
  uint32_t *const cnt = pool.count + (pool.use & 1u);
  // the counter of the NEXT use (see heatbath_cells_step); this form needs the list: pool.cap > 0
  if (threadIdx.x == 0) pool.count[(pool.use & 1u) ^ 1u] = 0;
  const PhiloxVKeys vk_ = philox_vkeys(key.k0, key.k1);
  const PhiloxVKeys *const vk = &vk_;
  auto cell = [&](uint32_t off, uint32_t site, uint32_t pair, auto on_list) {   // two copies, as in heatbath_cells_step
    VsCell c;
    double sv[6];
    stencil_load(off, sv);
    lds_wait6(sv);
    stencil_cell(sv, c);
    double th = 0.0;
    bool neg = false;
    for (;;) {
      if (vs_attempt_pair(key, vk, site, pair, c.kp, c.cls, pool.tab, [&] { return kappa_exact(off); }, th, neg)) {
        commit(off, mod_2pi_fast(c.centre + (neg ? -th : th)));
        return;
      }
      ++pair;
      if ((bool)on_list && pair == 1) {
        const uint32_t slot = atomicAdd(cnt, 1u);
        if (slot < pool.cap) {
          pool.buf[slot] = (E)(off | (pair << P::kOffBits));
          return;
        }
      }
    }
  };
#ifndef MLMCPI_HB_CELLS1
  // Two cells per lane and round, stage by stage (stencils, Philox calls, table look-ups, screening tests of both, then the
  // rare exact test of either behind ONE branch): a cell is one dependency chain with four LDS round trips in it, and a SIMD
  // holds four waves -- two of them this stage's --, so the second chain fills what the first one waits for
  static_assert(NIT % 2 == 0, "rounds come in pairs");
  for (int k = 0; k < NIT; k += 2) {
    uint32_t off[2], site[2], ca[2], cb[2];
    VsCell c[2];
    U4 q[2];
    float pa[2], pb[2];
    bool acc_a[2], acc_b[2], rej_a[2], rej_b[2];
    double sv[2][6];
#pragma unroll
    for (int j = 0; j < 2; ++j) main_cell(off[j], site[j]);
    // the twelve stencil reads (single ds_read_b64: callers issue them through lds_read_f64) are in flight under the two
    // Philox calls, which need nothing but the sites
#pragma unroll
    for (int j = 0; j < 2; ++j) stencil_load(off[j], sv[j]);
    const uint32_t w3 = (P_VONMISES << 24);
#pragma unroll
    for (int j = 0; j < 2; ++j) q[j] = philox4x32_10(site[j], key.chain, key.step, w3, key.k0, key.k1, vk_);
    lds_wait12(sv[0], sv[1]);
#pragma unroll
    for (int j = 0; j < 2; ++j) stencil_cell(sv[j], c[j]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      pa[j] = vs_accept_prob(q[j].y, c[j].kp, c[j].cls, pool.tab, ca[j]);
      pb[j] = vs_accept_prob(q[j].w, c[j].kp, c[j].cls, pool.tab, cb[j]);
    }
    bool open = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float la = (float)q[j].x, lb = (float)q[j].z;
      acc_a[j] = la <= fmaf(pa[j], pool.tab.s_acc, -kVsU2Slack);
      acc_b[j] = lb <= fmaf(pb[j], pool.tab.s_acc, -kVsU2Slack);
      rej_a[j] = la >= fmaf(pa[j], pool.tab.s_rej, kVsU2Slack);
      rej_b[j] = lb >= fmaf(pb[j], pool.tab.s_rej, kVsU2Slack);
      // open: the first attempt undecided, or rejected and the second undecided
      open = open || (!acc_a[j] && (!rej_a[j] || (!acc_b[j] && !rej_b[j])));
    }
    if (open) {   // (one attempt in ~10^4: the exact test, as in vs_attempt_pair)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (!acc_a[j] && (!rej_a[j] || (!acc_b[j] && !rej_b[j]))) {
          const uint8_t *row = pool.tab.base + c[j].cls + kVsLwOff;
          const uint32_t r = vs_exact_pair(key.k0, key.k1, key.chain, key.step, site[j], w3, q[j], ca[j] | (cb[j] << 8), *(const float *)(row + ca[j]),
                                           *(const float *)(row + cb[j]), kappa_exact(off[j]), rej_a[j] ? 0 : -1, acc_b[j] ? 1 : rej_b[j] ? 0 : -1,
                                           pool.tab.base);
          acc_a[j] = (r & 3u) == 1u;
          acc_b[j] = (r >> 2) == 1u;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (acc_a[j] || acc_b[j]) {
        const bool first = acc_a[j];
        const uint32_t lo = first ? q[j].x : q[j].z, hi = first ? q[j].y : q[j].w;
        const double th = vs_theta(lo, hi, first ? ca[j] : cb[j], pool.tab);
        commit(off[j], mod_2pi_fast(c[j].centre + ((lo & 0x200u) ? -th : th)));
      } else {
        const uint32_t slot = atomicAdd(cnt, 1u);
        if (slot < pool.cap) pool.buf[slot] = (E)(off[j] | (1u << P::kOffBits));
        else cell(off[j], site[j], 1u, std::false_type{});   // list full: finished where it is
      }
    }
  }
#else
  for (int k = 0; k < NIT; ++k) {
    uint32_t off, site;
    main_cell(off, site);
    cell(off, site, 0u, std::true_type{});
  }
#endif
  __syncthreads();
  const uint32_t n_list = min(*cnt, pool.cap);
  const uint32_t n = n_list + n_left;
  for (uint32_t i = threadIdx.x; i < n; i += NT) {
    uint32_t off, pair = 0;
    if (i < n_list) {
      const uint32_t e = pool.buf[i];
      off = e & kOffMask;
      pair = e >> P::kOffBits;
    } else {
      off = left_off(i - n_list);
    }
    cell(off, site_of(off), pair, std::false_type{});
  }
  ++pool.use;
}

// one draw x ~ exp(kappa cos(x - centre)) for the conditional between x_p and x_m (test hook; the sweeps go through
// heatbath_cells_step): returns mod_2pi(centre + x)
__device__ __forceinline__ double vs_draw(const RngKey &k, uint32_t site, double scale, double x_p, double x_m, const VsTable &tab) {
  VsCell c;
  vs_cell(scale, x_p, x_m, c);
  double th = 0.0;
  bool neg = false;
  for (uint32_t pair = 0; !vs_attempt_pair(k, (const PhiloxVKeys *)nullptr, site, pair, c.kp, c.cls, tab, [&] { return vs_kappa_exact(scale, x_p, x_m); }, th, neg); ++pair) {
  }
  return mod_2pi_fast(c.centre + (neg ? -th : th));
}

}  // namespace mlmcpi
