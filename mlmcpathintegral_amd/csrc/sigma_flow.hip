// sigma_flow.hip -- gradient flow of an O(3) sigma-model field on a level, rotated or not, and the charge, susceptibility and
// energy of the flowed field at a list of step counts (include/mlmcpi_hip.h: mlmcpi_sigma_level_flowed_charge).
//
//   F(Y)_l = Delta_l - (Y_l . Delta_l) Y_l,  Delta_l = add4 of the four neighbours' Y in the reference's order,  . = dot3
//   one step of size eps, on ALL sites from the previous stage's Y (Jacobi), A = 0 and Y = sigma at its start:
//     A <- a_i A + eps F(Y),  Y <- Y + b_i A,   i = 1, 2, 3,   a = (0, -17/32, -32/27),  b = (1/4, 8/9, 3/4)
//   then sigma <- Y / |Y|, |Y| = sqrt((x^2 + y^2) + z^2), three divisions.  Stage values are not normalised.
//
// The third-order 2N-storage Runge-Kutta scheme; flow time after s steps t = s eps.  The Markov chain's state is only read: the
// field lives in the caller's workspace as unit vectors in the layout of cooling (sigma_field_device.hpp) and is never converted
// back to angles between steps; A and the stage fields never leave a launch.
//
// Launches of a call:
//   1. sigma_cool_stage_kernel (cool_stage): sigma_of(angles) -> buffer A (step 0).
//   2. sigma_flow_kernel<ROT, NT>: one workgroup per tile per chain loads TW x TH vertices (rotated: plane cells, E and O) plus a
//      halo of 3 K (vertices or cells: a stage consumes one) from one buffer with modular loads, runs the 3 K stages of K steps in
//      LDS, one barrier per stage, stage m = 1 .. 3 K on the sites at least m from the edge of the loaded region, whose inputs
//      are still exact, the last stage exactly on the tile, and writes the tile to the other buffer.  K <= the plan's fuse depth
//      and a launch never runs past the next listed step.
//   3. at each listed step: the charge, energy and finish launches of cooling (cool_measure).
//   4. sigma_cool_angles_kernel (cool_angles) with d_flowed.
// LDS image per site: Y, the next Y (a stage reads the OLD Y of its neighbours) and A, 9 doubles = 72 B per vertex, 144 B per
// rotated cell.  A stage update is a pure function of the stored Y and A of the site and the stored Y of four neighbours, so a
// halo vertex recomputed by a neighbouring tile gets the bits its owner computes, and a vertex written to the buffer and loaded
// again is the vertex that stayed in LDS: the field of step s does not depend on the tile, the workgroup size, the fuse depth or
// the steps listed before s.  No atomics; workgroups of every launch ride one linear index over grid x and then y (topo_grid).
#include <math.h>

#include "internal.hpp"

#include "sigma_field_device.hpp"  // the field's layout, cooling's launches; fp contraction is off from here on

namespace mlmcpi {

constexpr double kFlowA[3] = {0.0, -17.0 / 32.0, -32.0 / 27.0};
constexpr double kFlowB[3] = {1.0 / 4.0, 8.0 / 9.0, 3.0 / 4.0};

// the geometry of a workgroup's region: W x HH entries per plane (P of them), S sites in all; local (la, lb) is the plane's entry
// ((sa + la) mod PW, (sb + lb) mod PH); the tile is [H, H + TW) x [H, H + TH), its origin (a0, b0) in the plane
struct FlowRegion {
  uint32_t W, HH, P, S, H, TW, TH, a0, b0, sa, sb, PW, PH;
};

// site s of the field at y[3][S]
__device__ __forceinline__ V3 flow_load(const double *y, uint32_t S, uint32_t s) { return V3{y[s], y[S + s], y[2 * S + s]}; }

__device__ __forceinline__ void flow_keep(double *y, uint32_t S, uint32_t s, const V3 &v) {
  y[s] = v.x;
  y[S + s] = v.y;
  y[2 * S + s] = v.z;
}

// Stage I + 1 of a step on the sites [m, W - 1 - m] x [m, HH - 1 - m] of every plane: y -> yn, A in place.  Stage 1 starts from
// A = 0 (a_1 = 0: 0 + eps F), stage 3 normalises and, with `out`, writes the sites of the tile that lie in the plane.
template <int ROT, int NT, int I>
__device__ __forceinline__ void flow_stage(const FlowRegion &R, uint32_t m, const double *y, double *yn, double *A, double eps, double *out,
                                           uint32_t n, uint32_t q) {
  constexpr uint32_t NP = ROT ? 2 : 1;
  const uint32_t rw = R.W - 2 * m, cnt = rw * (R.HH - 2 * m), W = R.W, P = R.P, S = R.S;
  for (uint32_t t = threadIdx.x; t < NP * cnt; t += NT) {
    const uint32_t p = ROT ? t / cnt : 0, r = t - p * cnt, la = m + r % rw, lb = m + r / rw, c = lb * W + la, s = p * P + c;
    uint32_t n0, n1, n2, n3;
    if constexpr (ROT) {  // the reference's order (+1,+1), (+1,-1), (-1,+1), (-1,-1): E reads O, O reads E
      n0 = p ? c + W + 1 : P + c;
      n1 = p ? c + 1 : P + c - W;
      n2 = p ? c + W : P + c - 1;
      n3 = p ? c : P + c - W - 1;
    } else {  // (+1, 0), (-1, 0), (0, +1), (0, -1)
      n0 = c + 1;
      n1 = c - 1;
      n2 = c + W;
      n3 = c - W;
    }
    const V3 Dl = add4(flow_load(y, S, n0), flow_load(y, S, n1), flow_load(y, S, n2), flow_load(y, S, n3));
    const V3 Y = flow_load(y, S, s);
    const double d = dot3(Y, Dl);
    const V3 F{Dl.x - d * Y.x, Dl.y - d * Y.y, Dl.z - d * Y.z};
    V3 a;
    if constexpr (I == 0) {
      a = V3{0.0 + eps * F.x, 0.0 + eps * F.y, 0.0 + eps * F.z};
    } else {
      const V3 o = flow_load(A, S, s);
      a = V3{kFlowA[I] * o.x + eps * F.x, kFlowA[I] * o.y + eps * F.y, kFlowA[I] * o.z + eps * F.z};
    }
    V3 v{Y.x + kFlowB[I] * a.x, Y.y + kFlowB[I] * a.y, Y.z + kFlowB[I] * a.z};
    if constexpr (I == 2) {
      const double nrm = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
      v = V3{v.x / nrm, v.y / nrm, v.z / nrm};
    } else {
      flow_keep(A, S, s, a);
    }
    flow_keep(yn, S, s, v);
    if constexpr (I == 2) {
      if (out && la >= R.H && la < R.H + R.TW && lb >= R.H && lb < R.H + R.TH && R.a0 + (la - R.H) < R.PW && R.b0 + (lb - R.H) < R.PH)
        cool_store(out, n, (size_t)p * q + (size_t)((R.sb + lb) % R.PH) * R.PW + (R.sa + la) % R.PW, v);
    }
  }
}

// ROT = 0: planes of Mt x Mx vertices; ROT = 1: the E and O planes of ht x hx cells (sigma_level_device.hpp).  LDS: Y [2][3][S]
// (the two stage fields, ping-pong), then A [3][S]; S = (ROT ? 2 : 1) (TW + 6 K) (TH + 6 K).
template <int ROT, int NT>
__global__ void __launch_bounds__(NT)
    sigma_flow_kernel(SigmaLevel L, uint64_t nblocks, const double *__restrict__ src, double *__restrict__ dst, uint32_t TW, uint32_t TH,
                      uint32_t tiles_a, uint32_t tiles, uint32_t K, double eps) {
  extern __shared__ double lds[];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint32_t tile = (uint32_t)(wg % tiles), tid = threadIdx.x, n = L.nvert();
  const double *s = src + (wg / tiles) * 3 * n;
  double *d = dst + (wg / tiles) * 3 * n;
  FlowRegion R;
  R.PW = ROT ? L.ht : L.Mt;
  R.PH = ROT ? L.hx : L.Mx;
  R.H = 3 * K;
  R.TW = TW;
  R.TH = TH;
  R.W = TW + 2 * R.H;
  R.HH = TH + 2 * R.H;
  R.P = R.W * R.HH;
  R.S = (ROT ? 2 : 1) * R.P;
  R.a0 = (tile % tiles_a) * TW;
  R.b0 = (tile / tiles_a) * TH;
  R.sa = R.a0 + (R.H / R.PW + 1) * R.PW - R.H;  // a0 - H mod PW, kept non-negative
  R.sb = R.b0 + (R.H / R.PH + 1) * R.PH - R.H;
  const uint32_t S = R.S;

  for (uint32_t c = tid; c < R.P; c += NT) {
    const uint32_t la = c % R.W, lb = c / R.W;
    const uint32_t l = ((R.sb + lb) % R.PH) * R.PW + (R.sa + la) % R.PW;
    flow_keep(lds, S, c, cool_fetch(s, n, l));
    if constexpr (ROT) flow_keep(lds, S, R.P + c, cool_fetch(s, n, L.q + l));
  }
  __syncthreads();

  double *y0 = lds, *y1 = lds + 3 * S, *A = lds + 6 * S;
  for (uint32_t k = 0; k < K; ++k) {  // three stages flip the two fields three times: every step starts from y0 <-> y1 swapped
    const uint32_t m = 3 * k;
    flow_stage<ROT, NT, 0>(R, m + 1, y0, y1, A, eps, nullptr, n, L.q);
    __syncthreads();
    flow_stage<ROT, NT, 1>(R, m + 2, y1, y0, A, eps, nullptr, n, L.q);
    __syncthreads();
    flow_stage<ROT, NT, 2>(R, m + 3, y0, y1, A, eps, k + 1 == K ? d : nullptr, n, L.q);
    if (k + 1 == K) break;
    __syncthreads();
    double *t = y0;
    y0 = y1;
    y1 = t;
  }
}

namespace {

struct FlowPlan {
  uint32_t tw, th, nt, fuse, tiles_a, tiles;
};

// Tile, workgroup size and fuse depth: the option, else 16 x 16 (vertices or cells), 512 threads, one step per launch (DESIGN.md
// 4.1h: 34 KB of LDS on a plain level, 68 KB on a rotated one); the tile never exceeds the plane.
FlowPlan flow_plan(const SigmaLevel &L, const Tuning &t) {
  FlowPlan p{t.sigma_flow_tw ? t.sigma_flow_tw : 16u, t.sigma_flow_th ? t.sigma_flow_th : 16u, t.sigma_flow_nt ? t.sigma_flow_nt : 512u,
             t.sigma_flow_fuse ? t.sigma_flow_fuse : 1u, 0, 0};
  const uint32_t PW = L.rot ? L.ht : L.Mt, PH = L.rot ? L.hx : L.Mx;
  if (p.tw > PW) p.tw = PW;
  if (p.th > PH) p.th = PH;
  p.tiles_a = (PW + p.tw - 1) / p.tw;
  p.tiles = p.tiles_a * ((PH + p.th - 1) / p.th);
  return p;
}

inline size_t flow_lds(const SigmaLevel &L, const FlowPlan &p, uint32_t K) {
  return (size_t)(p.tw + 6 * K) * (p.th + 6 * K) * (L.rot ? 18 : 9) * sizeof(double);
}

// what the call and its plan query refuse alike; the plan (one snapshot of the knobs per call) comes back through `plan`.  Its LDS
// image fits: the option table takes no plan whose images do not, the default's do, and flow_plan only shrinks tiles.
int flow_check(const mlmcpi_sigma_level *level, uint32_t n_chains, double eps, const uint32_t *steps, uint32_t n_steps, FlowPlan *plan) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(n_chains > 0, "the flow needs n_chains > 0");
  MLMCPI_REQUIRE(std::isfinite(eps) && eps > 0.0 && eps <= 0.25, "the flow takes a step size 0 < eps <= 0.25 (got %g)", eps);
  MLMCPI_REQUIRE(steps, "the flow needs a list of step counts (steps is NULL)");
  MLMCPI_REQUIRE(n_steps >= 1 && n_steps <= MLMCPI_SIGMA_FLOW_MAX_TIMES, "the flow takes 1 .. %d step counts (got %u)",
                 MLMCPI_SIGMA_FLOW_MAX_TIMES, n_steps);
  for (uint32_t k = 0; k < n_steps; ++k) {
    MLMCPI_REQUIRE(k == 0 || steps[k] > steps[k - 1], "the flow step counts must be strictly ascending (steps[%u] = %u after %u)", k,
                   steps[k], k ? steps[k - 1] : 0);
    MLMCPI_REQUIRE(steps[k] <= MLMCPI_SIGMA_FLOW_MAX_STEPS, "a flow step count is at most %d (steps[%u] = %u)", MLMCPI_SIGMA_FLOW_MAX_STEPS,
                   k, steps[k]);
  }
  const SigmaLevel L = make_level(*level);
  const FlowPlan p = *plan = flow_plan(L, tuning());
  uint32_t per_chain = (L.nvert() + kGroup - 1) / kGroup;
  if (p.tiles > per_chain) per_chain = p.tiles;
  if (topo_plan(L).tiles > per_chain) per_chain = topo_plan(L).tiles;
  const uint64_t most = (uint64_t)n_chains * per_chain;
  MLMCPI_REQUIRE(most <= kTopoMaxBlocks, "the flow takes at most %llu workgroups per launch (these chains need %llu)",
                 (unsigned long long)kTopoMaxBlocks, (unsigned long long)most);
  return MLMCPI_OK;
}

DeviceOnce g_flow_attr_once;

int flow_init_kernels() {  // the flow kernel may take the whole LDS (of the current device)
  return once_per_device(g_flow_attr_once, []() -> int {
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_flow_kernel<0, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_flow_kernel<0, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_flow_kernel<0, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_flow_kernel<1, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_flow_kernel<1, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_flow_kernel<1, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    return MLMCPI_OK;
  });
}

template <int ROT>
int flow_launch(const SigmaLevel &L, const FlowPlan &p, uint32_t K, double eps, uint64_t blocks, const double *src, double *dst, hipStream_t st) {
  const size_t lds = flow_lds(L, p, K);
#define MLMCPI_FLOW(NT) \
  hipLaunchKernelGGL((sigma_flow_kernel<ROT, NT>), topo_grid(blocks), dim3(NT), lds, st, L, blocks, src, dst, p.tw, p.th, p.tiles_a, p.tiles, K, eps)
  if (p.nt == 1024) MLMCPI_FLOW(1024);
  else if (p.nt == 512) MLMCPI_FLOW(512);
  else MLMCPI_FLOW(256);
#undef MLMCPI_FLOW
  MLMCPI_LAUNCH_CHECK("sigma_flow_kernel");
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_flow_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(bytes, "the flow workspace query needs somewhere to write (bytes is NULL)");
  MLMCPI_REQUIRE(n_chains > 0, "the flow needs n_chains > 0");
  *bytes = cool_work(make_level(*level), n_chains).total;
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_flow_plan(const mlmcpi_sigma_level *level, uint32_t n_chains, double eps, const uint32_t *steps, uint32_t n_steps,
                                 mlmcpi_sigma_flow_plan *plan) {
  MLMCPI_REQUIRE(plan, "the flow plan query needs somewhere to write (plan is NULL)");
  FlowPlan p;
  if (int rc = flow_check(level, n_chains, eps, steps, n_steps, &p)) return rc;
  const SigmaLevel L = make_level(*level);
  *plan = mlmcpi_sigma_flow_plan{};
  plan->tw = p.tw;
  plan->th = p.th;
  plan->nt = p.nt;
  plan->fuse = p.fuse;
  plan->tiles = p.tiles;
  plan->n_measurements = n_steps;
  uint32_t done = 0, deepest = 0;
  for (uint32_t k = 0; k < n_steps; ++k)
    while (done < steps[k]) {
      const uint32_t K = steps[k] - done < p.fuse ? steps[k] - done : p.fuse;
      plan->launch_steps[plan->n_launches++] = (uint8_t)K;
      if (K > deepest) deepest = K;
      done += K;
    }
  plan->lds_bytes = deepest ? (uint32_t)flow_lds(L, p, deepest) : 0;
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_flowed_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, double eps,
                                     const uint32_t *steps, uint32_t n_steps, double *d_q, double *d_chi, double *d_energy, double *d_flowed,
                                     void *d_work, size_t work_bytes, void *stream) {
  FlowPlan p;
  if (int rc = flow_check(level, n_chains, eps, steps, n_steps, &p)) return rc;
  MLMCPI_REQUIRE(d_state, "the flow needs a state (d_state is NULL)");
  MLMCPI_REQUIRE(d_q || d_chi || d_energy, "the flow needs d_q, d_chi or d_energy (all three are NULL)");
  MLMCPI_REQUIRE(d_work, "the flow needs its workspace (d_work is NULL)");
  const SigmaLevel L = make_level(*level);
  const CoolWork w = cool_work(L, n_chains);
  MLMCPI_REQUIRE(work_bytes >= w.total, "the flow workspace is too small: %zu bytes given, %zu needed", work_bytes, w.total);
  if (int rc = flow_init_kernels()) return rc;
  hipStream_t st = as_stream(stream);
  double *cur = (double *)d_work, *other = (double *)((char *)d_work + w.vec);
  double *part_q = (double *)((char *)d_work + 2 * w.vec), *part_e = (double *)((char *)d_work + 2 * w.vec + w.part_q);
  const uint64_t fblocks = (uint64_t)n_chains * p.tiles;

  if (int rc = cool_stage(L, w, n_chains, d_state, cur, st)) return rc;
  uint32_t done = 0;
  for (uint32_t k = 0; k < n_steps; ++k) {
    while (done < steps[k]) {
      const uint32_t K = steps[k] - done < p.fuse ? steps[k] - done : p.fuse;
      if (int rc = L.rot ? flow_launch<1>(L, p, K, eps, fblocks, cur, other, st) : flow_launch<0>(L, p, K, eps, fblocks, cur, other, st)) return rc;
      double *t = cur;
      cur = other;
      other = t;
      done += K;
    }
    if (int rc = cool_measure(L, w, n_chains, cur, part_q, part_e, n_steps, k, d_q, d_chi, d_energy, st)) return rc;
  }
  if (d_flowed)
    if (int rc = cool_angles(L, w, n_chains, cur, d_flowed, st)) return rc;
  return MLMCPI_OK;
}

}  // extern "C"
