// sigma_flow.hip -- gradient flow of an O(3) sigma-model field on a level, rotated or not, and the charge, susceptibility and
// energy of the flowed field at a list of step counts (include/mlmcpi_hip.h: mlmcpi_sigma_level_flowed_charge).
//
//   F(Y)_l = Delta_l - (Y_l . Delta_l) Y_l,  Delta_l = add4 of the four neighbours' Y in the reference's order,  . = dot3
//   one step of size eps, on ALL sites from the previous stage's Y (Jacobi), A = 0 and Y = sigma at its start:
//     A <- a_i A + eps F(Y),  Y <- Y + b_i A,   i = 1, 2, 3,   a = (0, -17/32, -32/27),  b = (1/4, 8/9, 3/4)
//   then sigma <- Y / |Y|, |Y| = sqrt((x^2 + y^2) + z^2), three divisions.  Stage values are not normalised.
//
// The third-order 2N-storage Runge-Kutta scheme; flow time after s steps t = s eps.  The Markov chain's state is only read: the
// field lives in the caller's workspace as unit vectors in the layout of sigma_field_device.hpp and is never converted
// back to angles between steps; A and the stage fields never leave a launch.
//
// The smoother of a call of the smoothing driver (sigma_smooth.hip: the field is staged, smoothed between two buffers, measured at
// each listed step count and turned back into angles by sigma_field.hip's launches) is
//   sigma_flow_kernel<ROT, NT>: one workgroup per tile per chain loads TW x TH vertices (rotated: plane cells, E and O) plus a
//   halo of 3 K (vertices or cells: a stage consumes one) from one buffer with modular loads, runs the 3 K stages of K steps in
//   LDS, one barrier per stage, stage m = 1 .. 3 K on the sites at least m from the edge of the loaded region, whose inputs
//   are still exact, the last stage exactly on the tile, and writes the tile to the other buffer.
// LDS image per site: Y, the next Y (a stage reads the OLD Y of its neighbours) and A, 9 doubles = 72 B per vertex, 144 B per
// rotated cell.  A stage update is a pure function of the stored Y and A of the site and the stored Y of four neighbours, so a
// halo vertex recomputed by a neighbouring tile gets the bits its owner computes, and a vertex written to the buffer and loaded
// again is the vertex that stayed in LDS: the field of step s does not depend on the tile, the workgroup size, the fuse depth or
// the steps listed before s.  No atomics; workgroups ride one linear index over grid x and then y (topo_grid).
#include <math.h>

#include "sigma_smooth_host.hpp"  // the driver; includes sigma_level_device.hpp: fp contraction is off from here on

#include "sigma_field_device.hpp"  // the field's layout

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
        field_store(out, n, (size_t)p * q + (size_t)((R.sb + lb) % R.PH) * R.PW + (R.sa + la) % R.PW, v);
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
    flow_keep(lds, S, c, field_fetch(s, n, l));
    if constexpr (ROT) flow_keep(lds, S, R.P + c, field_fetch(s, n, L.q + l));
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

// the default 16 x 16 x 512 x 1 takes 34 KB of LDS on a plain level, 68 KB on a rotated one
size_t flow_lds(const SigmaLevel &L, const SmoothPlan &p, uint32_t K) {
  return (size_t)(p.tw + 6 * K) * (p.th + 6 * K) * (L.rot ? 18 : 9) * sizeof(double);
}

template <int ROT>
int flow_launch(const SigmaLevel &L, const SmoothPlan &p, uint32_t K, double eps, uint64_t blocks, const double *src, double *dst, hipStream_t st) {
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

DeviceOnce g_flow_attr_once;

const Smoother kFlow = {
    "the flow", "flow", "step count", "steps", MLMCPI_SIGMA_FLOW_MAX_TIMES, MLMCPI_SIGMA_FLOW_MAX_STEPS,
    {&Tuning::sigma_flow_tw, &Tuning::sigma_flow_th, &Tuning::sigma_flow_nt, &Tuning::sigma_flow_fuse}, {16, 16, 512, 1},
    flow_lds, {flow_launch<0>, flow_launch<1>},
    {(const void *)sigma_flow_kernel<0, 256>, (const void *)sigma_flow_kernel<0, 512>, (const void *)sigma_flow_kernel<0, 1024>,
     (const void *)sigma_flow_kernel<1, 256>, (const void *)sigma_flow_kernel<1, 512>, (const void *)sigma_flow_kernel<1, 1024>}, &g_flow_attr_once};

// the flow's own argument, checked before the driver's
int flow_check_eps(double eps) {
  MLMCPI_REQUIRE(std::isfinite(eps) && eps > 0.0 && eps <= 0.25, "the flow takes a step size 0 < eps <= 0.25 (got %g)", eps);
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_flow_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes) {
  return smooth_workspace_bytes(kFlow, level, n_chains, bytes);
}

int mlmcpi_sigma_level_flow_plan(const mlmcpi_sigma_level *level, uint32_t n_chains, double eps, const uint32_t *steps, uint32_t n_steps,
                                 mlmcpi_sigma_flow_plan *plan) {
  if (int rc = flow_check_eps(eps)) return rc;
  return smooth_plan_query(kFlow, level, n_chains, steps, n_steps, plan, &mlmcpi_sigma_flow_plan::launch_steps);
}

int mlmcpi_sigma_level_flowed_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, double eps,
                                     const uint32_t *steps, uint32_t n_steps, double *d_q, double *d_chi, double *d_energy, double *d_flowed,
                                     void *d_work, size_t work_bytes, void *stream) {
  if (int rc = flow_check_eps(eps)) return rc;
  return smooth_run(kFlow, level, d_state, n_chains, eps, steps, n_steps, d_q, d_chi, d_energy, d_flowed, d_work, work_bytes, stream);
}

}  // extern "C"
