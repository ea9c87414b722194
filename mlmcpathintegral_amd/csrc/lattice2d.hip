// lattice2d.hip -- sweeps of the 2-D lattice actions: Gaussian free field (vertex field, 5-point stencil),
// quenched Schwinger model (U(1) link angles, plaquette action) and O(3) sigma model, batched over B chains in the
// reference's own SampleState layout (vertex l = Mt*j + i; link l = 2*Mt*j + 2*i + mu, i.e. one
// double2 {theta_0, theta_1} per site, which is exactly a 16-byte-per-lane coalesced load).
//
// Sweeps are overlapped-tile kernels: a workgroup stages its tile plus a halo of 2 sites per fused
// sweep in LDS, runs all colours of all fused sweeps there, and writes only the tile it owns to a
// second buffer.  Halo updates are recomputed by every workgroup that needs them; the counter-based
// RNG makes those recomputations bit-identical.  Per sweep HBM sees ~(1 + halo overhead) reads and
// one write of every entry -- instead of the 4-5 passes of one-kernel-per-colour -- and k fused
// sweeps divide that by k.
// This file is the action-agnostic part of the sweep path: the launch plan (make_sweep_plan, next_launch), its executor
// (sweep_draw_impl), the entry points and the site-at-a-time updates.  The sweep kernels of an action and the function that
// launches them are in schwinger_sweeps.hip, gff_sweeps.hip and sigma2d.hip; lattice_sweep.hpp holds the launcher interface and
// the sizes planner and kernels agree on.
// Reductions, force and HMC, level transfers and the two-level step, and the exact GFF sampler are in lattice_reduce.hip,
// lattice_hmc.hip, lattice_twolevel.hip and gff_exact.hip.
#include <algorithm>

#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include "lattice_sweep.hpp"
#include "step_envelope.hpp"

namespace mlmcpi {

// hipFuncSetAttribute applies to the current device: once per device, under a lock (one process may drive several GPUs)
static DeviceOnce g_lds_attr_once;
static int init_sweep_kernels() {
  return once_per_device(g_lds_attr_once, []() -> int {
    if (int rc = schwinger_allow_lds()) return rc;
    if (int rc = gff_allow_lds()) return rc;
    return MLMCPI_OK;
  });
}

// ---- launch plan: the per-draw constants; next_launch is the only place that chooses kernels.  No HIP call in here. ----
struct SweepPlan {
  int32_t kind;
  uint32_t Mt, Mx, B, n_overrelax, n_heatbath;
  double coupling;                   // beta; GFF: mu2
  Tuning tune;                       // ONE snapshot per draw: mlmcpi_set_option on another thread cannot split a launch plan
  uint32_t tile_w, tile_h, tile_nt;  // generic tile kernels and the sigma model: 64 x 32 owned sites, 256 threads (4 workgroups
                                     // per CU at one sweep); MLMCPI_SWEEP_TILE=TWxTHxNT overrides (results never depend on it)
  bool schw, or_blocks, gff_blocks32, perm, perm64, step;  // step: the heat bath's sampler, a property of the action, not a knob
  int gff_T;                         // the GFF register-block tile (0: the generic kernels)
  uint32_t perm_th;
  uint32_t fuse, fuse_arg;           // sweeps per launch in effect / as the caller gave it
};

// sigma model (profiles/sigma_fuse_tile.json, 1024^2 x 32, 10 + 1 sweeps): 64 x 32 tiles of 256 threads, 2 sweeps
// per launch -- 8.78 ms per draw against 9.94 ms at fuse = 1 and 10.25 ms on 32 x 32 tiles; the kernel is issue-bound, so
// deeper fusion buys little (fuse 3: 8.75 ms) and at fuse 4 the 92 KB tile leaves one workgroup per CU
constexpr uint32_t kSigmaFuse = 2;
static size_t sigma_lds_bytes(const SweepPlan &p, uint32_t K) {  // three planes of tile + halo
  return (size_t)(p.tile_w + 4 * K) * (p.tile_h + 4 * K) * 3 * sizeof(double); }

// The argument checks every draw makes, then the constants.  `fuse` = 0: the library default.
static int make_sweep_plan(const mlmcpi_lattice_action *act, uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath, uint32_t fuse,
                           const Tuning &tune, SweepPlan *out) {
  if (int rc = check_lattice(act)) return rc;
  MLMCPI_REQUIRE(B > 0, "bad arguments");
  MLMCPI_REQUIRE(act->Mt % 2 == 0 && act->Mx % 2 == 0, "multicolour sweeps need even Mt, Mx (got %u x %u)", act->Mt, act->Mx);
  SweepPlan &p = *out;
  const uint32_t Mt = act->Mt, Mx = act->Mx;
  p = SweepPlan{act->kind, Mt, Mx, B, n_overrelax, n_heatbath, act->beta, tune};
  p.tile_w = tune.tile_w ? tune.tile_w : 64;
  p.tile_h = tune.tile_w ? tune.tile_h : 32;
  p.tile_nt = tune.tile_w && (tune.tile_nt == 1024 || tune.tile_nt == 512) ? tune.tile_nt : 256;
  p.fuse_arg = fuse;
  if (act->kind == MLMCPI_NONLINEAR_SIGMA) {
    p.fuse = std::min(fuse ? fuse : kSigmaFuse, kMaxFuse);
    while (p.fuse > 1 && sigma_lds_bytes(p, p.fuse) > kSigmaLdsMax) --p.fuse;
    if (sigma_lds_bytes(p, p.fuse) > kSigmaLdsMax)
      return fail(MLMCPI_ERR_INVALID, "sigma sweep tile %u x %u does not fit in LDS", p.tile_w, p.tile_h);
    return MLMCPI_OK;
  }
  const bool schw = p.schw = act->kind == MLMCPI_SCHWINGER;
  p.coupling = schw ? act->beta : gff_mu2(*act);
  p.step = schw && 2. * act->beta <= kVsKappaMax;
  // 4 x 4 register-block overrelaxation on 64 x 64 tiles where they divide the lattice: the GFF default; for the Schwinger
  // action the sweep-by-sweep plan (MLMCPI_OR_KERNEL=block, lattices the closed form does not take)
  p.or_blocks = !tune.tile_w && Mt % 64 == 0 && Mx % 64 == 0;
  // GFF lattices that 32 x 32 tiles divide and 64 x 64 ones do not (or that are below 128, where the 64-tile fused launch
  // does not apply): the register-block kernels on 32 x 32 tiles, same launch plan
  // (r05: also lattices no tile divides -- edge tiles computed whole and written in part -- unless the padding would more
  // than double the work)
  const uint32_t g32_tx = (Mt + 31) / 32, g32_ty = (Mx + 31) / 32;
  p.gff_blocks32 = !schw && !tune.tile_w && Mt >= 64 && Mx >= 64 && !(p.or_blocks && Mt >= 128 && Mx >= 128) &&
                   (uint64_t)g32_tx * g32_ty * 1024 <= (uint64_t)2 * Mt * Mx + (uint64_t)Mt * Mx / 5;
  // 64 only on lattices of at least 128 x 128 (else gff_blocks32)
  p.gff_T = schw ? 0 : p.gff_blocks32 ? 32 : p.or_blocks ? 64 : 0;
  // Schwinger overrelaxation in closed form (schwinger_perm_kernel, schwinger_perm_heat_kernel): the default;
  // MLMCPI_OR_KERNEL=block selects the sweep-by-sweep kernels
  // r05: any even lattice of at least one tile.  Tiles on the upper / right edge of a lattice the tiles do not divide reach
  // beyond it; what lies there are periodic images of vertices other tiles own (the plane wraps as often as needed):
  // computed like any halo, not written.  64 x 64 tiles where they divide Mx and wherever the fused launch applies (both
  // extents >= 128: its image must not wrap onto itself), else 64 x 32 (the heat bath is then a launch of its own);
  // lattices that would more than double the work through padding stay with the sweep-by-sweep kernels.
  const bool perm_shape = schw && Mt >= 64 && Mx >= 32 && (uint64_t)Mt * Mx < (1ull << 28);   // (32-bit byte offsets)
  p.perm64 = perm_shape && (Mx % 64 == 0 || (Mt >= 128 && Mx >= 128));
  p.perm_th = p.perm64 ? 64 : 32;
  const uint32_t perm_tx = (Mt + 63) / 64, perm_ty = (Mx + p.perm_th - 1) / p.perm_th;
  p.perm = perm_shape && !tune.or_block && !tune.tile_w &&
           (uint64_t)perm_tx * 64 * perm_ty * p.perm_th <= (uint64_t)2 * Mt * Mx + (uint64_t)Mt * Mx / 5;
  // library default: best measured whole-step time -- up to 6 sweeps per launch where the 4 x 4
  // register-block kernels apply, 4 otherwise
  p.fuse = std::min(fuse ? fuse : (p.or_blocks || p.gff_blocks32) ? 6u : 4u, kMaxFuse);
  return MLMCPI_OK;
}

// The launch that begins at sweep s < n_overrelax + n_heatbath of the draw.  Stateless; allocates nothing.
// Overrelaxation sweeps are fused: they are bound by the passes over the state, and a fused launch trades halo
// recomputation (cheap for them) for passes.  A heat-bath sweep is bound by its sampler arithmetic, which a wider halo
// would only multiply: no sweep follows it inside a launch.  As the LAST sweep of an overrelaxation launch it needs no
// halo of its own beyond the two rings it reads (schwinger_perm_heat_kernel, gff_or_heat_kernel); otherwise it gets a
// launch to itself.  (The sigma model's kernel takes both kinds of sweep, up to `fuse` of them.)
static int next_launch(const SweepPlan &p, uint32_t s, SweepLaunch *out) {
  SweepLaunch &l = *out;
  l = {};
  const uint32_t Mt = p.Mt, Mx = p.Mx, rem = s < p.n_overrelax ? p.n_overrelax - s : 0;
  auto tiles = [&](uint32_t TW, uint32_t TH) {  // the owned tile and the workgroups per chain
    l.tile_w = TW, l.tile_h = TH, l.tiles_x = (Mt + TW - 1) / TW;
    l.grid_x = l.tiles_x * ((Mx + TH - 1) / TH);
  };
  if (p.kind == MLMCPI_NONLINEAR_SIGMA) {
    const uint32_t K = std::min(p.n_overrelax + p.n_heatbath - s, p.fuse);
    l.kernel = MLMCPI_K_SIGMA_SWEEP;
    l.n_overrelax = std::min(rem, K);
    l.n_heatbath = K - l.n_overrelax;
    l.threads = p.tile_nt;
    tiles(p.tile_w, p.tile_h);
    l.lds_bytes = (uint32_t)sigma_lds_bytes(p, K);
    return MLMCPI_OK;
  }
  if (p.perm && rem) {
    // as few launches as kPermMaxK (or the caller's `fuse`) allows, of equal depth
    const uint32_t kmax = p.fuse_arg ? std::min(p.fuse_arg, kPermMaxK) : kPermMaxK;
    const uint32_t launches = (rem + kmax - 1) / kmax, K = (rem + launches - 1) / launches;
    l.n_overrelax = K;
    tiles(64, p.perm_th);
    if (p.perm64 && !p.tune.or_heat_split && K == rem && p.n_heatbath >= 1 && Mt >= 128 && Mx >= 128) {
      // the last overrelaxation launch takes the heat-bath sweep behind it along, and the QoI if that ends the draw
      // at most one workgroup per CU: sixteen waves (MLMCPI_OR_HEAT=wide|narrow forces)
      const bool wide = p.tune.or_heat_wide ? p.tune.or_heat_wide > 0 : (uint64_t)l.grid_x * p.B <= kComputeUnits;
      // (the packed plane of either workgroup size lies inside the image's LDS at every depth: one build, planes = 1)
      l.planes = 1;
      l.kernel = MLMCPI_K_SCHWINGER_PERM_HEAT;
      l.n_heatbath = 1;
      l.threads = wide ? 1024 : 512;
      l.step = p.step;
      l.lds_bytes = (uint32_t)PermHeatGeom<512, true>::lds_bytes;
    } else {
      l.kernel = MLMCPI_K_SCHWINGER_PERM;
      l.threads = 512;
      l.planes = 1;
      l.lds_bytes = (uint32_t)(p.perm64 ? perm_lds_bytes<64>() : perm_lds_bytes<32>());
    }
    return MLMCPI_OK;
  }
  // register blocks: as few launches as `fuse` allows, of equal depth (10 sweeps, fuse 6: 5 + 5, not 6 + 4)
  const uint32_t launches = (rem + p.fuse - 1) / p.fuse;
  uint32_t n = !rem ? 1 : (p.or_blocks || p.gff_blocks32) ? (rem + launches - 1) / launches : std::min(rem, p.fuse);
  const bool heat = !rem, overridden = p.tune.tile_w != 0;  // a heat-bath sweep is a launch of its own: n == 1
  // the generic tile: Schwinger two link angles per site; GFF heat bath field + parked normal per site
  const uint32_t TW = std::min(Mt, p.tile_w), TH = std::min(Mx, p.tile_h), bytes_per_cell = (p.schw || heat) ? 16 : 8;
  auto tile_lds = [&](uint32_t k) { return (size_t)(TW + 4 * k) * (TH + 4 * k) * bytes_per_cell; };
  while (n > 1 && tile_lds(n) > 160 * 1024 - 256) --n;  // shrink the fused count until the tile + halo fits in LDS
  if (!heat && !overridden && n <= 6 && (p.schw ? p.or_blocks : p.gff_T != 0)) {
    // 4 x 4 register blocks, sweep by sweep.  Schwinger: 64 x 64 tiles (bit-identical to the generic kernel and the closed
    // form).  GFF: gff_T x gff_T tiles; the last overrelaxation launch of the draw takes the heat-bath sweep behind it
    // along (and the QoI, if that ends the draw): gff_or_heat_kernel, bit-identical to the two launches (MLMCPI_OR_HEAT=split)
    const uint32_t T = p.schw ? 64 : (uint32_t)p.gff_T;
    const bool fused = !p.schw && !p.tune.or_heat_split && n == rem && p.n_heatbath >= 1 && n <= 5;
    l.kernel = p.schw ? MLMCPI_K_SCHWINGER_OR_BLOCK : fused ? MLMCPI_K_GFF_OR_HEAT : MLMCPI_K_GFF_OR_BLOCK;
    l.n_overrelax = n;
    l.n_heatbath = fused;
    tiles(T, T);
    with_depth<6>(n, [&](auto kc) {
      constexpr int K = decltype(kc)::value, KH = K < 5 ? K : 5;  // (fused: n <= 5)
      auto size = [&](uint32_t nt, size_t lds) { l.threads = nt, l.lds_bytes = (uint32_t)lds; };
      if (p.schw) size(OrBlockGeom<K>::NT, OrBlockGeom<K>::lds_bytes);
      else if (fused && T == 32) size(GffHeatGeom<KH, 32>::NT, GffHeatGeom<KH, 32>::lds_bytes);
      else if (fused) size(GffHeatGeom<KH, 64>::NT, GffHeatGeom<KH, 64>::lds_bytes);
      else if (T == 32) size(GffBlockGeom<K, 32>::NT, GffBlockGeom<K, 32>::lds_bytes);
      else size(GffBlockGeom<K, 64>::NT, GffBlockGeom<K, 64>::lds_bytes);
      return 0;
    });
    return MLMCPI_OK;
  }
  // the generic tile kernels; launches without a heat-bath sweep use the lean instantiation (no sampler code, fewer VGPRs)
  l.kernel = p.schw ? MLMCPI_K_SCHWINGER_SWEEP : MLMCPI_K_GFF_SWEEP;
  l.n_overrelax = heat ? 0 : n;
  l.n_heatbath = l.kinds = heat;
  l.threads = p.tile_nt;
  tiles(TW, TH);
  // single heat-bath sweep on a lattice the default tiles divide: compile-time tile geometry (bit-identical results)
  l.fixed_tile = heat && !overridden && Mt % 64 == 0 && Mx % 32 == 0 && Mt >= 128 && Mx >= 64;
  l.step = heat && p.step;
  size_t lds = tile_lds(n);
  if (p.schw && heat) {
    // room for the tables and the list of open cells in front of the tile image, as many entries as still keep the workgroup's
    // LDS footprint within a quarter of the CU's 160 KiB (4 workgroups per CU), at least one wave's worth
    const bool step = l.step, fixed = l.fixed_tile;
    const size_t quarter = 40 * 1024 - 64;  // (the kernel's static LDS: the QoI reduction scratch)
    const size_t entry = step ? (fixed ? sizeof(uint16_t) : sizeof(uint32_t)) : 24, fixed_part = (step ? kVsTableBytes + 16 : 8) + 16;
    uint32_t cap = 64;
    if (lds + fixed_part + entry * cap <= quarter) cap = (uint32_t)((quarter - lds - fixed_part) / entry) & ~7u;
    if (cap > (step ? 256u : 1024u)) cap = step ? 256u : 1024u;
    if (lds + sweep_pool_bytes(step, fixed && step, cap) > 160 * 1024 - 256) cap = 0;
    l.pool_cap = cap;
    lds += sweep_pool_bytes(step, fixed && step, cap);
  }
  l.lds_bytes = (uint32_t)lds;
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

// The launches read `src` and write `dst`; after each one src <- dst and dst <- the other work buffer.  d_phi is only
// read unless it is also d_w1.  result_in (may be NULL: then the result is copied into d_phi, which must be writable):
// 0 -> the result is in d_w0, 1 -> in d_w1, -1 -> no sweep was run (result is the input).
// qoi_kind != 0 (1 average plaquette, 2 Q^2 / 4 pi^2, 3 phi^2, 4 chi_m): the QoI of the final state, summed inside the last
// launch (so the draw must end with a heat-bath sweep) into d_qoi[b].
static int sweep_draw_impl(const mlmcpi_lattice_action *act, double *d_phi, double *d_w0, double *d_w1, uint32_t B,
                           uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                           uint32_t fuse, int32_t *result_in, void *stream, int qoi_kind = 0, double *d_qoi = nullptr,
                           double *d_acc = nullptr) {
  SweepPlan p;
  if (int rc = make_sweep_plan(act, B, n_overrelax, n_heatbath, fuse, tuning(), &p)) return rc;
  const bool sigma = act->kind == MLMCPI_NONLINEAR_SIGMA;
  if (qoi_kind) {
    MLMCPI_REQUIRE(d_qoi && qoi_kind >= 1 && qoi_kind <= 4, "bad QoI arguments");
    const int own = act->kind == MLMCPI_GFF ? 3 : sigma ? 4 : 0;
    if (own ? qoi_kind != own : qoi_kind > 2)
      return fail(MLMCPI_ERR_UNSUPPORTED, "fused QoI %d does not belong to this action", qoi_kind);
    if (n_heatbath == 0) return fail(MLMCPI_ERR_UNSUPPORTED, "the fused QoI needs a draw that ends with a heat-bath sweep");
  }
  MLMCPI_REQUIRE(d_phi && d_w0 && d_w1 && d_phi != d_w0 && d_w0 != d_w1, "bad arguments");
  if (int rc = sigma ? sigma_init_sweep_kernels() : init_sweep_kernels()) return rc;
  const hipStream_t st = as_stream(stream);
  const uint32_t total = n_overrelax + n_heatbath;
  const int qoi_op = qoi_kind == 1 ? (int)L_PLAQ : qoi_kind == 2 ? (int)L_CHARGE : (int)L_PHI2;  // (the sigma model has one QoI: any op != 0)
  const auto launch = sigma ? sigma_sweep_launch : act->kind == MLMCPI_SCHWINGER ? schwinger_sweep_launch : gff_sweep_launch;
  double *src = d_phi, *dst = d_w0;
  for (uint32_t s = 0; s < total;) {
    SweepLaunch l;
    if (int rc = next_launch(p, s, &l)) return rc;
    const uint32_t sweeps = l.n_overrelax + l.n_heatbath;
    const bool with_qoi = qoi_kind && s + sweeps == total;  // the launch ends the draw: it sums the QoI per tile and finishes it
    const SweepArgs a = {p.Mt, p.Mx, B, p.coupling, src, dst, make_key(seed, chain0, sweep0 + s), with_qoi ? qoi_op : 0, d_qoi, d_acc, st};
    if (int rc = launch(l, a)) return rc;
    src = dst;  // the buffer just written becomes the input; the next output is the other work buffer
    dst = (dst == d_w0) ? d_w1 : d_w0;
    s += sweeps;
  }
  if (result_in)
    *result_in = total == 0 ? -1 : (src == d_w0 ? 0 : 1);
  else if (src != d_phi)
    MLMCPI_HIP_TRY(hipMemcpyAsync(d_phi, src, (size_t)B * p.Mt * p.Mx * (act->kind == MLMCPI_GFF ? 8 : 16), hipMemcpyDeviceToDevice, st));
  return MLMCPI_OK;
}

// The launches of that draw, in order, without touching a device: same argument checks, same planner.
int mlmcpi_lattice_sweep_plan(const mlmcpi_lattice_action *act, uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath,
                              uint32_t fuse, mlmcpi_sweep_launch *out, uint32_t capacity, uint32_t *count) {
  SweepPlan p;
  if (int rc = make_sweep_plan(act, B, n_overrelax, n_heatbath, fuse, tuning(), &p)) return rc;
  MLMCPI_REQUIRE(count && (out || capacity == 0), "bad arguments");
  uint32_t n = 0;
  for (uint32_t s = 0; s < n_overrelax + n_heatbath; ++n) {
    SweepLaunch l;
    if (int rc = next_launch(p, s, &l)) return rc;
    if (n < capacity) out[n] = l;
    s += l.n_overrelax + l.n_heatbath;
  }
  *count = n;
  if (n > capacity) return fail(MLMCPI_ERR_INVALID, "the plan has %u launches, capacity is %u", n, capacity);
  return MLMCPI_OK;
}

int mlmcpi_lattice_sweep_draw(const mlmcpi_lattice_action *act, double *d_phi, double *d_scratch, uint32_t B,
                              uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                              uint32_t sweep0, uint32_t fuse, void *stream) {
  return sweep_draw_impl(act, d_phi, d_scratch, d_phi, B, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse, nullptr, stream);
}

int mlmcpi_lattice_sweep_draw_pingpong(const mlmcpi_lattice_action *act, double *d_a, double *d_b, uint32_t B,
                                       uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                                       uint32_t sweep0, uint32_t fuse, int32_t *result_in_b, void *stream) {
  MLMCPI_REQUIRE(result_in_b, "result_in_b is NULL");
  int32_t where = 0;
  if (int rc = sweep_draw_impl(act, d_a, d_b, d_a, B, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse, &where, stream)) return rc;
  *result_in_b = where == 0 ? 1 : 0;  // work buffer 0 is d_b; no sweeps (-1) or work buffer 1: the result is in d_a
  return MLMCPI_OK;
}

int mlmcpi_lattice_sweep_draw_from(const mlmcpi_lattice_action *act, const double *d_src, double *d_w0, double *d_w1,
                                   uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                                   uint32_t sweep0, uint32_t fuse, int32_t *result_in, void *stream) {
  MLMCPI_REQUIRE(result_in, "result_in is NULL");
  MLMCPI_REQUIRE(n_overrelax + n_heatbath > 0, "no sweeps requested: the result would be the (read-only) input");
  // the input is only ever the `src` of the first launch (or a work buffer when the caller passes d_w1 == d_src)
  return sweep_draw_impl(act, const_cast<double *>(d_src), d_w0, d_w1, B, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse,
                         result_in, stream);
}

int mlmcpi_lattice_sweep_draw_qoi(const mlmcpi_lattice_action *act, const double *d_src, double *d_w0, double *d_w1, uint32_t B,
                                  uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                                  uint32_t fuse, int32_t qoi_kind, double *d_qoi, int32_t *result_in, void *stream) {
  MLMCPI_REQUIRE(result_in, "result_in is NULL");
  MLMCPI_REQUIRE(qoi_kind >= 1 && qoi_kind <= 4, "qoi_kind %d: 1 = average plaquette, 2 = Q^2 / (4 pi^2), 3 = phi^2 (GFF), 4 = chi_m (sigma model)", qoi_kind);
  return sweep_draw_impl(act, const_cast<double *>(d_src), d_w0, d_w1, B, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse,
                         result_in, stream, qoi_kind, d_qoi);
}

int mlmcpi_lattice_sweep_draw_qoi_record(const mlmcpi_lattice_action *act, const double *d_src, double *d_w0, double *d_w1,
                                         uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                                         uint32_t sweep0, uint32_t fuse, int32_t qoi_kind, double *d_qoi, double *d_acc,
                                         int32_t *result_in, void *stream) {
  MLMCPI_REQUIRE(result_in && d_acc, "result_in or d_acc is NULL");
  MLMCPI_REQUIRE(qoi_kind >= 1 && qoi_kind <= 4, "qoi_kind %d: 1 = average plaquette, 2 = Q^2 / (4 pi^2), 3 = phi^2 (GFF), 4 = chi_m (sigma model)", qoi_kind);
  return sweep_draw_impl(act, const_cast<double *>(d_src), d_w0, d_w1, B, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse,
                         result_in, stream, qoi_kind, d_qoi, d_acc);
}

int mlmcpi_lattice_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites,
                                uint32_t n, uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step,
                                void *stream) {
  if (int rc = check_lattice(act)) return rc;
  MLMCPI_REQUIRE(d_state && B > 0, "bad arguments");
  uint32_t size = 0;
  mlmcpi_lattice_state_size(act, &size);
  if (!d_sites) {
    MLMCPI_REQUIRE(site < size, "site %u out of range (%u entries)", site, size);
    n = 1;
  }
  if (n == 0) return MLMCPI_OK;
  if (act->kind == MLMCPI_NONLINEAR_SIGMA) {  // l is a vertex
    MLMCPI_REQUIRE(d_sites || site < act->Mt * act->Mx, "vertex %u out of range (%u vertices)", site, act->Mt * act->Mx);
    return sigma_site_updates(act, d_state, B, d_sites, n, site, heat, seed, chain0, step, as_stream(stream));
  }
  if (act->kind == MLMCPI_SCHWINGER)
    return schwinger_site_updates(act, d_state, B, d_sites, n, site, heat, seed, chain0, step, as_stream(stream));
  hipLaunchKernelGGL((lattice_site_update_kernel<false>), dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), act->Mt, act->Mx, gff_mu2(*act),
                     d_state, B, d_sites, n, site, (int)heat, make_key(seed, chain0, step), (const uint32_t *)nullptr);
  MLMCPI_LAUNCH_CHECK("lattice_site_update_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
