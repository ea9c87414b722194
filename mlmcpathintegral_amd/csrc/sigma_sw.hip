// sigma_sw.hip -- the Swendsen-Wang multi-cluster update of the O(3) nonlinear sigma model (gfx950, wave64), on the unrotated
// lattice (mlmcpi_sigma_sw_*) and on the levels of its CoarsenRotate hierarchy (mlmcpi_sigma_level_sw_*; an unrotated level IS
// the lattice and takes its entry point).  This unit has the launch plan, the workspace layout, the draw and the entry points;
// the kernels and their launches are in sigma_sw_tiled.hip, sigma_sw_chain.hip and sigma_sw_correlator.hip, where the improved
// estimators are described too.  The geometry lives in sigma_cluster_device.hpp (LatticeGeometry, RotatedGeometry).
//
// The multi-cluster form of the embedding sigma_cluster.hip grows one cluster of: one update tests ALL 2 N links once, labels
// EVERY connected component of the graph of bonded links and reflects each component with probability 1/2.  The reference has
// no such sampler; like the Wolff update it is the project's own (tests/sigma_sw_model.py).
//
// The update, restated.  Vertex l = Mt j + i; link (l, 0) joins l to its +i neighbour, link (l, 1) to its +j neighbour
// (periodic, 2 N links; on an extent of 2 the two links between a pair are two links with a uniform each).  With r the
// reflection normal and a_l = r . sigma_l of the field BEFORE the update, a link (x, y) is bonded iff a_x a_y > 0 and its
// uniform < 1 - exp(min(0, -2 beta (a_x a_y))) (the product first: the same bits from either end).  The root of a cluster is
// its smallest vertex index; the cluster is reflected iff the root's coin says so, sigma' = sigma - 2 a r for every vertex of
// it, stored in the canonical form (sigma2d.hip).  Every decision is a function of (link or root, chain, update counter,
// field before the update): the state does not depend on the launch plan, the tile, the batch split or chain0.
//
// RNG contract, step = global update counter update0 + k:
//   P_SIGMA_SW_REFLECT  site 0, sub 0: (u, v) -> r_z = 1 - 2 u, azimuth 2 pi v - pi (the map of P_SIGMA_REFLECT sub 0)
//   P_SIGMA_SW_BOND     site l, sub 0: u decides link (l, 0), v decides link (l, 1)
//   P_SIGMA_SW_FLIP     site root, sub 0: reflected iff u < 0.5
#include <stdio.h>
#include <string.h>

#include "sigma_sw_host.hpp"

#include "sigma_sw_device.hpp"  // the chain plan's bound

namespace mlmcpi {
namespace {

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// Launch plan; it chooses and calls nothing.  The chain plan where a chain fits its LDS bound and one
// workgroup per chain fills the device (B >= kComputeUnits: a chain's workgroup is 16 waves and takes more than half a CU's
// LDS, so one is resident per CU), the tiled plan otherwise.  Knobs (bit-identical results): MLMCPI_SIGMA_SW_PLAN=chain|tiled,
// MLMCPI_SIGMA_SW_TILE=WxH (vertices; on a rotated level cells).  ok = false: the chain plan was forced beyond its bound.
template <class Geometry>
SwPlan sw_plan(const Geometry &g, uint32_t B, const Tuning &tune) {
  SwPlan p{};
  const uint32_t N = g.nvert();
  uint32_t pw, ph;
  sw_tiling(g, pw, ph, p.W, p.H);
  p.chain = tune.sigma_sw_plan ? tune.sigma_sw_plan == 1 : (N <= kSwChainMaxN && B >= kComputeUnits);
  p.ok = !p.chain || N <= kSwChainMaxN;
  if (tune.sigma_sw_tile_w) p.W = tune.sigma_sw_tile_w;
  if (tune.sigma_sw_tile_h) p.H = tune.sigma_sw_tile_h;
  p.ntx = (pw + p.W - 1) / p.W;
  p.nty = (ph + p.H - 1) / p.H;
  p.merge_blocks = (sw_crossing(g, p) + kClusterThreads - 1) / kClusterThreads;
  p.resolve_blocks = (N + kClusterThreads - 1) / kClusterThreads;
  p.lds_bytes = p.chain ? (size_t)N * kSwChainBytesPerVertex : sw_tile_lds(g, p.W, p.H);
  return p;
}

// ---- the workspace ----------------------------------------------------------------------------------------------------------
constexpr uint32_t kSwStructureSlots = 4;
constexpr size_t kSwStatusBytes = 256;

// the sections of SwWorkspace (sigma_sw_host.hpp), one after the other
template <class Geometry>
int sw_layout(const Geometry &g, uint32_t B, SwFlavour flavour, SwWorkspace &ws) {
  const uint32_t N = g.nvert(), M0 = g.extent(0), M1 = g.extent(1);
  const bool structure = flavour == SwFlavour::kStructure, correlator = flavour == SwFlavour::kCorrelator;
  const size_t fixed = align256((size_t)B * N * sizeof(long long));
  size_t end = 0;
  const auto take = [&end](size_t bytes) {
    const SwSection s{end, bytes};
    end += bytes;
    return s;
  };
  ws = SwWorkspace{};
  ws.status = take(kSwStatusBytes);
  ws.label = take(align256((size_t)B * N * sizeof(uint32_t)));
  ws.qa = take(fixed);
  ws.sum = take(fixed);
  ws.slots = take(structure ? kSwStructureSlots * fixed : 0);
  ws.bits = take(align256((size_t)B * g.nowners()));
  // the chain plan's table of weights lies over qa, sum and slots: 48 B per vertex and chain hold 16 (M_0 + M_1) B per chain
  // (on every level: both extents are even and >= 2)
  ws.weights = SwSection{ws.qa.offset, structure ? (size_t)B * 2 * (M0 + M1) * sizeof(double) : 0};
  MLMCPI_REQUIRE(!structure || (uint64_t)3 * N >= (uint64_t)M0 + M1, "the table of weights does not fit the workspace");
  const SwLagScale lags = sw_lag_scale(N, M0, M1);
  ws.n_out = lags.n_out;
  ws.s = lags.s;
  ws.lg = 1;
  while ((1ull << ws.lg) < 2ull * N) ++ws.lg;
  ws.table = take(correlator ? align256(((size_t)2 * B << ws.lg) * 16) : 0);
  ws.count = take(correlator ? align256((size_t)2 * B * N * sizeof(uint32_t)) : 0);
  ws.acc = take(correlator ? align256((size_t)B * ws.n_out * sizeof(long long)) : 0);
  return MLMCPI_OK;
}

// ---- the draw -------------------------------------------------------------------------------------------------------------------
DeviceOnce g_sw_attr_once;

// dynamic LDS above 64 KiB, once per device: the chain kernels up to their bound, the rotated launch 1 at the largest tile
int sw_init_attrs() {
  return once_per_device(g_sw_attr_once, []() -> int {
    if (int rc = sw_chain_init_attrs()) return rc;
    if (int rc = sw_tiled_init_attrs()) return rc;
    return MLMCPI_OK;
  });
}

inline const char *sw_chain_kernel_name(const LatticeGeometry &) { return "sigma_sw_chain_kernel"; }
inline const char *sw_chain_kernel_name(const RotatedGeometry &) { return "sigma_rot_sw_chain_kernel"; }

// The draw on either geometry, arguments checked: the workspace laid out, the launches issued, the status word read back.
// r.d_structure: the structure instances of the kernels and the larger workspace; r.d_corr (never with d_structure): the
// improved correlator's launches after every update, its workspace behind the plain draw's (the entry point has checked the size
// of either).
template <class Geometry>
int sw_draw(const Geometry &g, const SwRequest &r) {
  const uint32_t N = g.nvert(), B = r.B;
  const SwFlavour flavour = r.d_corr ? SwFlavour::kCorrelator : r.d_structure ? SwFlavour::kStructure : SwFlavour::kPlain;
  const SwPlan p = sw_plan(g, B, tuning());
  if (!p.ok)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: MLMCPI_SIGMA_SW_PLAN=chain holds a chain of at most %u vertices in LDS, this %s has %u", r.what,
                kSwChainMaxN, strcmp(r.what, "mlmcpi_sigma_sw_draw") ? "level" : "lattice", N);
  const uint64_t widest = (uint64_t)B * (p.ntx * p.nty > p.resolve_blocks ? p.ntx * p.nty : p.resolve_blocks);
  MLMCPI_REQUIRE(p.chain || (widest < (1ull << 31) && (uint64_t)B * p.merge_blocks < (1ull << 31)), "too many workgroups for one launch: split the batch");
  SwWorkspace ws;
  if (int rc = sw_layout(g, B, flavour, ws)) return rc;
  MLMCPI_REQUIRE(!r.d_corr || ((uint64_t)B * p.resolve_blocks < (1ull << 31) && ((uint64_t)2 * B << ws.lg) / kClusterThreads < (1ull << 31) &&
                               (uint64_t)B * ws.n_out < (1ull << 31)),
                 "too many workgroups for one launch: split the batch");
  if (r.n_updates == 0) return MLMCPI_OK;
  if (int rc = sw_init_attrs()) return rc;
  const hipStream_t st = as_stream(r.stream);
  uint32_t *status = ws.status.in<uint32_t>(r.d_work);
  MLMCPI_HIP_TRY(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
  if (p.chain) {
    // what a launch error shows: the kernel's name on this geometry and its instance
    char name[64];
    snprintf(name, sizeof(name), "%s%s", sw_chain_kernel_name(g), r.d_corr ? " (roots)" : r.d_structure ? " (structure)" : "");
    // with the correlator one update per launch (the same bits as one launch of all: the call-split property), its roots and q(a)
    // left in the workspace
    const uint32_t per_launch = r.d_corr ? 1u : r.n_updates;
    for (uint32_t k = 0; k < r.n_updates; k += per_launch) {
      if (int rc = sw_chain_launch(g, flavour, p, ws, r, per_launch, make_key(r.seed, r.chain0, r.update0 + k), name)) return rc;
      if (r.d_corr)
        if (int rc = sw_corr_update(g, p, ws, r)) return rc;
    }
  } else {
    // the four structure slots are zeroed here once (sigma_sw_tiled.hip keeps them zero from update to update)
    if (r.d_structure) MLMCPI_HIP_TRY(hipMemsetAsync(ws.slots.in<char>(r.d_work), 0, ws.slots.bytes, st));
    for (uint32_t k = 0; k < r.n_updates; ++k) {
      if (int rc = sw_tiled_update(g, p, ws, r, make_key(r.seed, r.chain0, r.update0 + k))) return rc;
      if (r.d_corr)
        if (int rc = sw_corr_update(g, p, ws, r)) return rc;
    }
  }
  // a find or union loop that ran into its cap (it cannot, by the argument of sigma_sw_device.hpp): an error, never a hang
  uint32_t h_status = 0;
  MLMCPI_HIP_TRY(hipMemcpyAsync(&h_status, status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MLMCPI_HIP_TRY(hipStreamSynchronize(st));
  if (h_status) return fail(MLMCPI_ERR_HIP, "%s: a labelling loop reached its iteration cap (status %u); the state is undefined", r.what, h_status);
  return MLMCPI_OK;
}

// ---- what the entry points share ------------------------------------------------------------------------------------------------
int sw_check(const mlmcpi_lattice_action *act, const char *what) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind != MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: the Swendsen-Wang update is built for the O(3) nonlinear sigma model only "
                "(action kind %d)", what, act->kind);
  if (int rc = check_lattice(act)) return rc;
  if (!(act->beta > 0.0)) return fail(MLMCPI_ERR_INVALID, "beta must be positive");
  return MLMCPI_OK;
}

// f(geometry of the level): the lattice for an unrotated level, the rotated level otherwise
template <class F>
int sw_on_level(const mlmcpi_sigma_level *level, F &&f) {
  if (!level->rotated) return f(LatticeGeometry{level->Mt, level->Mx});
  return f(RotatedGeometry(make_level(*level)));
}

template <class Geometry>
int sw_workspace_bytes(const Geometry &g, uint32_t B, SwFlavour flavour, size_t *bytes) {
  SwWorkspace ws;
  if (int rc = sw_layout(g, B, flavour, ws)) return rc;
  *bytes = ws.bytes();
  return MLMCPI_OK;
}

// the workspace query of a level entry point `what`; an unrotated level passes the checks of the lattice as well
int sw_level_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, SwFlavour flavour, size_t *bytes, const char *what) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    if (int rc = sw_check(&act, what)) return rc;
  }
  return sw_on_level(level, [&](const auto &g) { return sw_workspace_bytes(g, B, flavour, bytes); });
}

// The argument checks of a draw, behind those of its action or level: the pointers and the batch; for the draws with a further
// output that output and the size of the workspace (`need`: what the flavour's query asks for); the update counter.
int sw_check_request(const SwRequest &r, SwFlavour flavour, size_t work_bytes, size_t need) {
  MLMCPI_REQUIRE(r.d_phi && r.d_work && r.B > 0, "bad arguments");
  if (flavour == SwFlavour::kStructure) {
    MLMCPI_REQUIRE(r.d_structure, "d_structure is NULL: mlmcpi_sigma_level_sw_draw is the entry point without structure sums");
    MLMCPI_REQUIRE(work_bytes >= need, "the workspace is smaller than mlmcpi_sigma_level_sw_structure_workspace_bytes asks for");
  } else if (flavour == SwFlavour::kCorrelator) {
    MLMCPI_REQUIRE(r.d_corr, "d_corr is NULL: mlmcpi_sigma_level_sw_draw is the entry point without the improved correlator");
    MLMCPI_REQUIRE(work_bytes >= need, "the workspace is smaller than mlmcpi_sigma_level_sw_correlator_workspace_bytes asks for");
  }
  MLMCPI_REQUIRE((uint64_t)r.update0 + r.n_updates <= 0xFFFFFFFFull, "update counter overflows");
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_sw_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  if (int rc = sw_check(act, "mlmcpi_sigma_sw_workspace_bytes")) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  return sw_workspace_bytes(LatticeGeometry{act->Mt, act->Mx}, B, SwFlavour::kPlain, bytes);
}

int mlmcpi_sigma_sw_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed, uint32_t chain0,
                         uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved, void *d_work, void *stream) {
  if (int rc = sw_check(act, "mlmcpi_sigma_sw_draw")) return rc;
  const SwRequest r{"mlmcpi_sigma_sw_draw", act->beta, d_phi, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved,
                    nullptr, nullptr, d_work, stream};
  if (int rc = sw_check_request(r, SwFlavour::kPlain, 0, 0)) return rc;
  return sw_draw(LatticeGeometry{act->Mt, act->Mx}, r);
}

int mlmcpi_sigma_level_sw_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  // an unrotated level asks the lattice's query, under its name
  return sw_level_workspace_bytes(level, B, SwFlavour::kPlain, bytes, "mlmcpi_sigma_sw_workspace_bytes");
}

int mlmcpi_sigma_level_sw_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                               uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                               void *d_work, void *stream) {
  if (int rc = check_cluster_level(level)) return rc;
  const SwRequest r{"mlmcpi_sigma_level_sw_draw", level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters,
                    d_improved, nullptr, nullptr, d_work, stream};
  if (int rc = sw_check_request(r, SwFlavour::kPlain, 0, 0)) return rc;
  if (!level->rotated) {                                   // the lattice's entry point, and its name in the messages
    const mlmcpi_lattice_action act = level_as_lattice(level);
    return mlmcpi_sigma_sw_draw(&act, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved, d_work, stream);
  }
  return sw_draw(RotatedGeometry(make_level(*level)), r);
}

int mlmcpi_sigma_level_sw_structure_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  return sw_level_workspace_bytes(level, B, SwFlavour::kStructure, bytes, "mlmcpi_sigma_level_sw_structure_workspace_bytes");
}

int mlmcpi_sigma_level_sw_structure_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                                         uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                                         double *d_structure, void *d_work, size_t work_bytes, void *stream) {
  size_t need = 0;
  if (int rc = mlmcpi_sigma_level_sw_structure_workspace_bytes(level, B ? B : 1, &need)) return rc;
  const SwRequest r{"mlmcpi_sigma_level_sw_structure_draw", level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped,
                    d_clusters, d_improved, d_structure, nullptr, d_work, stream};
  if (int rc = sw_check_request(r, SwFlavour::kStructure, work_bytes, need)) return rc;
  return sw_on_level(level, [&](const auto &g) { return sw_draw(g, r); });
}

int mlmcpi_sigma_level_sw_correlator_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  return sw_level_workspace_bytes(level, B, SwFlavour::kCorrelator, bytes, "mlmcpi_sigma_level_sw_correlator_workspace_bytes");
}

int mlmcpi_sigma_level_sw_correlator_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                                          uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                                          double *d_corr, void *d_work, size_t work_bytes, void *stream) {
  size_t need = 0;
  if (int rc = mlmcpi_sigma_level_sw_correlator_workspace_bytes(level, B ? B : 1, &need)) return rc;
  const SwRequest r{"mlmcpi_sigma_level_sw_correlator_draw", level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped,
                    d_clusters, d_improved, nullptr, d_corr, d_work, stream};
  if (int rc = sw_check_request(r, SwFlavour::kCorrelator, work_bytes, need)) return rc;
  return sw_on_level(level, [&](const auto &g) { return sw_draw(g, r); });
}

}  // extern "C"
