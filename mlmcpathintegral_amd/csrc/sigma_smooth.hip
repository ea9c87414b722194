// sigma_smooth.hip -- the one driver of the smoothers of an O(3) sigma-model field (sigma_smooth_host.hpp).
//
// Launches of a call:
//   1. field_stage: sigma_of(angles) -> buffer A of the workspace (point 0 of the list's scale).
//   2. the smoother's launch, K fused units from one vector buffer to the other: K <= the plan's fuse depth, and a launch never
//      runs past the next listed point (smooth_walk).
//   3. at each listed point: field_measure (charge, energy, finish).
//   4. field_angles with d_out.
// The driver owns no kernel: the field's are sigma_field.hip's, a smoother launches its own.
#include <algorithm>

#include "sigma_smooth_host.hpp"

#include "sigma_field_device.hpp"

namespace mlmcpi {

namespace {

// Tile, workgroup size and fuse depth: the option, else the smoother's default; the tile never exceeds the plane.
SmoothPlan smooth_plan(const SigmaLevel &L, const Smoother &s, const Tuning &t) {
  uint32_t v[4];
  for (int i = 0; i < 4; ++i) v[i] = t.*s.knob[i] ? t.*s.knob[i] : s.dflt[i];
  SmoothPlan p{v[0], v[1], v[2], v[3], 0, 0};
  const uint32_t PW = L.rot ? L.ht : L.Mt, PH = L.rot ? L.hx : L.Mx;
  if (p.tw > PW) p.tw = PW;
  if (p.th > PH) p.th = PH;
  p.tiles_a = (PW + p.tw - 1) / p.tw;
  p.tiles = p.tiles_a * ((PH + p.th - 1) / p.th);
  return p;
}

// the schedule of a call, the one copy: launch(K) for every launch, point(k) once list[k] units are done
template <class Launch, class Point>
int smooth_walk(const uint32_t *list, uint32_t n, uint32_t fuse, Launch launch, Point point) {
  uint32_t done = 0;
  for (uint32_t k = 0; k < n; ++k) {
    while (done < list[k]) {
      const uint32_t K = list[k] - done < fuse ? list[k] - done : fuse;
      if (int rc = launch(K)) return rc;
      done += K;
    }
    if (int rc = point(k)) return rc;
  }
  return MLMCPI_OK;
}

}  // namespace

int smooth_check(const Smoother &s, const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *list, uint32_t n, SmoothPlan *plan) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(n_chains > 0, "%s needs n_chains > 0", s.who);
  MLMCPI_REQUIRE(list, "%s needs a list of %ss (%s is NULL)", s.who, s.item, s.list);
  MLMCPI_REQUIRE(n >= 1 && n <= s.max_items, "%s takes 1 .. %u %ss (got %u)", s.who, s.max_items, s.item, n);
  for (uint32_t k = 0; k < n; ++k) {
    MLMCPI_REQUIRE(k == 0 || list[k] > list[k - 1], "the %s %ss must be strictly ascending (%s[%u] = %u after %u)", s.adj, s.item, s.list, k,
                   list[k], k ? list[k - 1] : 0);
    MLMCPI_REQUIRE(list[k] <= s.max_count, "a %s %s is at most %u (%s[%u] = %u)", s.adj, s.item, s.max_count, s.list, k, list[k]);
  }
  const SigmaLevel L = make_level(*level);
  const SmoothPlan p = *plan = smooth_plan(L, s, tuning());
  // the widest launch of a call: the vertex groups (stage, energy, angles), the smoother's tiles or the charge tiles
  const uint64_t most = (uint64_t)n_chains * std::max({(L.nvert() + kGroup - 1) / kGroup, p.tiles, topo_plan(L).tiles});
  MLMCPI_REQUIRE(most <= kTopoMaxBlocks, "%s takes at most %llu workgroups per launch (these chains need %llu)", s.who,
                 (unsigned long long)kTopoMaxBlocks, (unsigned long long)most);
  return MLMCPI_OK;
}

uint32_t smooth_schedule(const Smoother &s, const SigmaLevel &L, const SmoothPlan &p, const uint32_t *list, uint32_t n, uint8_t *launches,
                         uint32_t *n_launches) {
  uint32_t deepest = 0;
  *n_launches = 0;
  smooth_walk(
      list, n, p.fuse,
      [&](uint32_t K) -> int {
        launches[(*n_launches)++] = (uint8_t)K;
        if (K > deepest) deepest = K;
        return MLMCPI_OK;
      },
      [](uint32_t) -> int { return MLMCPI_OK; });
  return deepest ? (uint32_t)s.lds(L, p, deepest) : 0;
}

int smooth_workspace_bytes(const Smoother &s, const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(bytes, "the %s workspace query needs somewhere to write (bytes is NULL)", s.adj);
  MLMCPI_REQUIRE(n_chains > 0, "%s needs n_chains > 0", s.who);
  *bytes = field_work(make_level(*level), n_chains).total;
  return MLMCPI_OK;
}

int smooth_run(const Smoother &s, const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, double eps, const uint32_t *list,
               uint32_t n, double *d_q, double *d_chi, double *d_energy, double *d_out, void *d_work, size_t work_bytes, void *stream) {
  SmoothPlan p;
  if (int rc = smooth_check(s, level, n_chains, list, n, &p)) return rc;
  MLMCPI_REQUIRE(d_state, "%s needs a state (d_state is NULL)", s.who);
  MLMCPI_REQUIRE(d_q || d_chi || d_energy, "%s needs d_q, d_chi or d_energy (all three are NULL)", s.who);
  MLMCPI_REQUIRE(d_work, "%s needs its workspace (d_work is NULL)", s.who);
  const SigmaLevel L = make_level(*level);
  const FieldWork w = field_work(L, n_chains);
  MLMCPI_REQUIRE(work_bytes >= w.total, "the %s workspace is too small: %zu bytes given, %zu needed", s.adj, work_bytes, w.total);
  if (int rc = once_per_device(*s.once, [&s]() -> int {  // the smoother's kernel may take the whole LDS (of the current device)
        for (const void *kernel : s.kernels) MLMCPI_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
        return MLMCPI_OK;
      }))
    return rc;
  hipStream_t st = as_stream(stream);
  FieldBuffers b = field_carve(w, d_work);
  const uint64_t blocks = (uint64_t)n_chains * p.tiles;

  if (int rc = field_stage(L, w, n_chains, d_state, b.cur, st)) return rc;
  if (int rc = smooth_walk(
          list, n, p.fuse,
          [&](uint32_t K) -> int {
            if (int rc = s.launch[L.rot ? 1 : 0](L, p, K, eps, blocks, b.cur, b.other, st)) return rc;
            std::swap(b.cur, b.other);
            return MLMCPI_OK;
          },
          [&](uint32_t k) -> int { return field_measure(L, w, n_chains, b.cur, b.part_q, b.part_e, n, k, d_q, d_chi, d_energy, st); }))
    return rc;
  if (d_out)
    if (int rc = field_angles(L, w, n_chains, b.cur, d_out, st)) return rc;
  return MLMCPI_OK;
}

}  // namespace mlmcpi
