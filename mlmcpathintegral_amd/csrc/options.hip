// options.hip -- the tuning knobs (Tuning, internal.hpp): ONE table of {name, parser}, which mlmcpi_set_option looks a name up
// in and the loading from the environment walks, so a knob is settable by both or by neither.
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <string>

#include "internal.hpp"

namespace mlmcpi {

namespace {
std::mutex g_tuning_mutex;
Tuning g_tuning;
bool g_tuning_loaded = false;

// TWxTHxNTxK: tile extents 1 .. 128, workgroup size, 1 .. kMaxFuse units fused per launch, and an LDS image that fits
bool parse_plan(const std::string &v, uint32_t &tw, uint32_t &th, uint32_t &nt, uint32_t &fuse, bool (*fits)(size_t a, size_t b, size_t k)) {
  unsigned a = 0, b = 0, c = 0, k = 0;
  char rest = 0;
  tw = th = nt = fuse = 0;
  if (v.empty()) return true;
  if (sscanf(v.c_str(), "%ux%ux%ux%u%c", &a, &b, &c, &k, &rest) == 4 && a >= 1 && a <= 128 && b >= 1 && b <= 128 &&
      (c == 256 || c == 512 || c == 1024) && k >= 1 && k <= kMaxFuse && fits(a, b, k)) {
    tw = a; th = b; nt = c; fuse = k;
    return true;
  }
  return false;
}

// A parser puts its knob back to the default first, then takes the value: false (value refused) leaves the default in force.
struct Option { const char *name; bool (*parse)(Tuning &t, const std::string &v); };
const Option kOptions[] = {
  {"MLMCPI_SWEEP_TILE", [](Tuning &t, const std::string &v) {
    unsigned a = 0, b = 0, c = 0;
    t.tile_w = t.tile_h = t.tile_nt = 0;
    if (v.empty()) return true;
    if (sscanf(v.c_str(), "%ux%ux%u", &a, &b, &c) == 3 && a >= 2 && b >= 2 && a % 2 == 0 && b % 2 == 0 && (c == 256 || c == 512 || c == 1024)) {
      t.tile_w = a; t.tile_h = b; t.tile_nt = c;
      return true;
    }
    return false;
  }},
  {"MLMCPI_OR_KERNEL", [](Tuning &t, const std::string &v) {
    t.or_block = v == "block";
    return v.empty() || v == "block" || v == "perm";
  }},
  {"MLMCPI_OR_HEAT", [](Tuning &t, const std::string &v) {
    t.or_heat_split = v == "split";
    t.or_heat_wide = v == "wide" ? 1 : v == "narrow" ? -1 : 0;
    return v.empty() || v == "split" || v == "fused" || v == "wide" || v == "narrow";
  }},
  {"MLMCPI_RANDOM_SWEEP_HOME", [](Tuning &t, const std::string &v) {
    t.random_sweep_global = v == "global";
    return v.empty() || v == "global" || v == "lds";
  }},
  {"MLMCPI_RANDOM_SWEEP_CHUNK", [](Tuning &t, const std::string &v) {
    unsigned k = 0;
    t.random_sweep_chunk = 0;
    if (v.empty()) return true;
    if (sscanf(v.c_str(), "%u", &k) == 1 && k >= 1 && k <= 254) {
      t.random_sweep_chunk = k;
      return true;
    }
    return false;
  }},
  {"MLMCPI_SIGMA_CLUSTER_TEAM", [](Tuning &t, const std::string &v) {
    t.sigma_cluster_team = v == "wave" ? 1 : v == "block" ? 2 : 0;
    return v.empty() || v == "auto" || v == "wave" || v == "block";
  }},
  {"MLMCPI_SIGMA_CLUSTER_BITMAP", [](Tuning &t, const std::string &v) {
    t.sigma_cluster_map_global = v == "global";
    return v.empty() || v == "global" || v == "lds";
  }},
  {"MLMCPI_SIGMA_SW_PLAN", [](Tuning &t, const std::string &v) {
    t.sigma_sw_plan = v == "chain" ? 1 : v == "tiled" ? 2 : 0;
    return v.empty() || v == "auto" || v == "chain" || v == "tiled";
  }},
  {"MLMCPI_SIGMA_SW_TILE", [](Tuning &t, const std::string &v) {
    unsigned a = 0, b = 0;
    char rest = 0;
    t.sigma_sw_tile_w = t.sigma_sw_tile_h = 0;
    if (v.empty()) return true;
    auto extent = [](unsigned e) { return e == 8 || e == 16 || e == 32 || e == 64; };
    if (sscanf(v.c_str(), "%ux%u%c", &a, &b, &rest) == 2 && extent(a) && extent(b)) {
      t.sigma_sw_tile_w = a; t.sigma_sw_tile_h = b;
      return true;
    }
    return false;
  }},
  {"MLMCPI_SIGMA_LEVEL_PLAN", [](Tuning &t, const std::string &v) {
    return parse_plan(v, t.sigma_level_tw, t.sigma_level_th, t.sigma_level_nt, t.sigma_level_fuse, [](size_t a, size_t b, size_t k) { return (a + 2 * k) * (b + 2 * k) * 48 <= kSigmaLdsMax; });
  }},
  {"MLMCPI_SIGMA_COOL_PLAN", [](Tuning &t, const std::string &v) {  // the LDS image of a rotated level (halo K cells, 48 B) and of a plain one (halo 2 K vertices, 24 B)
    return parse_plan(v, t.sigma_cool_tw, t.sigma_cool_th, t.sigma_cool_nt, t.sigma_cool_fuse, [](size_t a, size_t b, size_t k) { return (a + 2 * k) * (b + 2 * k) * 48 <= kSigmaLdsMax && (a + 4 * k) * (b + 4 * k) * 24 <= kSigmaLdsMax; });
  }},
  {"MLMCPI_SIGMA_FLOW_PLAN", [](Tuning &t, const std::string &v) {  // the LDS image of a rotated level (halo 3 K cells, 144 B) and of a plain one (halo 3 K vertices, 72 B)
    return parse_plan(v, t.sigma_flow_tw, t.sigma_flow_th, t.sigma_flow_nt, t.sigma_flow_fuse, [](size_t a, size_t b, size_t k) { return (a + 6 * k) * (b + 6 * k) * 144 <= kSigmaLdsMax && (a + 6 * k) * (b + 6 * k) * 72 <= kSigmaLdsMax; });
  }},
  {"MLMCPI_SIGMA_TWOLEVEL_GROUPS", [](Tuning &t, const std::string &v) {
    unsigned g = 0;
    char rest = 0;
    t.sigma_twolevel_groups = 0;
    if (v.empty()) return true;
    if (sscanf(v.c_str(), "%u%c", &g, &rest) == 1 && g >= 1 && g <= 64) {
      t.sigma_twolevel_groups = g;
      return true;
    }
    return false;
  }},
};

bool apply_option(Tuning &t, const char *name, const char *value) {
  const std::string n = name ? name : "", v = value ? value : "";
  for (const Option &o : kOptions)
    if (n == o.name) return o.parse(t, v);
  return false;
}
void load_tuning_locked() {
  if (g_tuning_loaded) return;
  for (const Option &o : kOptions)
    if (const char *e = getenv(o.name)) o.parse(g_tuning, e);
  g_tuning_loaded = true;
}
}  // namespace

Tuning tuning() {
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  load_tuning_locked();
  return g_tuning;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_set_option(const char *name, const char *value) {
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  load_tuning_locked();
  if (!apply_option(g_tuning, name, value)) return fail(MLMCPI_ERR_INVALID, "unknown option or value: %s=%s", name ? name : "(null)", value ? value : "(null)");
  return MLMCPI_OK;
}

}  // extern "C"
