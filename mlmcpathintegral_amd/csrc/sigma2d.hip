// sigma2d.hip -- the O(3) nonlinear sigma model on the 2-D lattice (action/qft/nonlinearsigmaaction.{hh,cc}).
//
// State: two doubles per vertex, (theta, phi) = phi[b * 2 Mt Mx + 2 (Mt j + i) + {0, 1}], one double2 per vertex; the spin
// is sigma(theta, phi) = (sin theta cos phi, sin theta sin phi, cos theta).  S = -1/2 beta sum_n sigma_n . Delta_n, Delta_n
// the sum of the four neighbours (+i, -i, +j, -j: lattice2d.cc:137-155).
//
// CANONICAL FORM.  Every update reads its neighbours as sigma(theta, phi) recomputed from the stored angles (sigma_of), and
// stores the angles of its result (angles_of).  The sweep kernel keeps the canonical vectors sigma(angles_of(sigma')) in
// LDS between the fused sweeps of a launch, which is exactly what a later launch would recompute from the stored angles;
// so a draw gives the same bits whatever the fuse depth, tile or workgroup size (the GFF contract of mlmcpi_hip.h).  The
// file is compiled without fp contraction (below) so that the same expression cannot round differently in two kernels.
//
// Randomness: heat bath of vertex l in sweep s = ONE Philox call (site l, chain, step sweep0 + s, P_SIGMA_HB, sub 0) ->
// (u, v); initialise: P_INIT, one uniform per state entry (entry 2l -> cos theta = 1 - 2u, 2l + 1 -> phi = 2 pi u - pi).
#include "lattice_sweep.hpp"

#include "sigma_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

// ---- the multicolour sweep kernel ------------------------------------------------------------------------------------
// One workgroup = one TW x TH tile of one chain, loaded with a halo of H = 2 K vertices into LDS as three SoA planes of
// canonical unit vectors; K sweeps (k < k_heat overrelaxation, the rest heat bath), two colour phases each ((i + j) even,
// then odd), one barrier per phase.  Phase p of the launch updates the sites at least p + 1 from the edge of the loaded
// region (the region whose values are still exact); the last phase reaches exactly the tile.  The last sweep writes the
// tile's angles (non-temporal) and, with `partial`, the tile's magnetisation sums partial[(b * tiles + tile) * 3 + c].
// Tiles on the upper / right edge of a lattice the tiles do not divide reach beyond it: what lies there are periodic images
// (the plane wraps as often as needed, so any even lattice >= 2 x 2 works), updated like the halo and not written.
template <int NT>
__global__ void __launch_bounds__(NT)
    sigma_sweep_kernel(uint32_t Mt, uint32_t Mx, double beta, const double2 *__restrict__ src, double2 *__restrict__ dst,
                       uint32_t TW, uint32_t TH, uint32_t tiles_t, uint32_t K, uint32_t k_heat, RngKey key,
                       double *__restrict__ partial) {
  extern __shared__ double lds[];
  __shared__ double red[3][NT / kWave];
  const uint32_t H = 2 * K, W = TW + 2 * H, HH = TH + 2 * H, P = W * HH;
  double *sx = lds, *sy = lds + P, *sz = lds + 2 * P;
  const uint32_t b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const uint32_t i0 = (tile % tiles_t) * TW, j0 = (tile / tiles_t) * TH;
  // global coordinate of local (li, lj) = ((ai + li) mod Mt, (aj + lj) mod Mx); ai = i0 - H mod Mt, kept non-negative
  const uint32_t ai = i0 + (H / Mt + 1) * Mt - H, aj = j0 + (H / Mx + 1) * Mx - H;
  const size_t N = (size_t)Mt * Mx;
  const double2 *s = src + b * N;
  double2 *d = dst + b * N;
  key.chain += b;

  for (uint32_t q = tid; q < P; q += NT) {
    const uint32_t li = q % W, lj = q / W;
    const uint32_t gi = (ai + li) % Mt, gj = (aj + lj) % Mx;
    const V3 v = sigma_of(s[(size_t)gj * Mt + gi]);
    sx[q] = v.x;
    sy[q] = v.y;
    sz[q] = v.z;
  }
  __syncthreads();

  double mx = 0.0, my = 0.0, mz = 0.0;
  for (uint32_t k = 0; k < K; ++k) {
    const bool heat = k >= k_heat, last = k + 1 == K;
    RngKey kk = key;
    kk.step += k;
    for (uint32_t c = 0; c < 2; ++c) {
      const uint32_t m = 2 * k + c + 1, rw2 = (W - 2 * m) / 2, rh = HH - 2 * m;
      for (uint32_t t = tid; t < rw2 * rh; t += NT) {
        const uint32_t lj = m + t / rw2;
        const uint32_t li = m + 2 * (t % rw2) + ((c + ai + aj + lj + m) & 1u);
        const uint32_t q = lj * W + li;
        const V3 sig{sx[q], sy[q], sz[q]};
        const V3 Dl = add4(V3{sx[q + 1], sy[q + 1], sz[q + 1]}, V3{sx[q - 1], sy[q - 1], sz[q - 1]},
                           V3{sx[q + W], sy[q + W], sz[q + W]}, V3{sx[q - W], sy[q - W], sz[q - W]});
        const uint32_t gi = (ai + li) % Mt, gj = (aj + lj) % Mx;
        const double2 a = angles_of(sigma_update(sig, Dl, heat, beta, kk, gj * Mt + gi));
        const V3 cv = sigma_of(a);
        sx[q] = cv.x;
        sy[q] = cv.y;
        sz[q] = cv.z;
        if (last && li >= H && li < H + TW && lj >= H && lj < H + TH && i0 + (li - H) < Mt && j0 + (lj - H) < Mx) {
          __builtin_nontemporal_store(a.x, &d[(size_t)gj * Mt + gi].x);
          __builtin_nontemporal_store(a.y, &d[(size_t)gj * Mt + gi].y);
          mx += cv.x;
          my += cv.y;
          mz += cv.z;
        }
      }
      __syncthreads();
    }
  }
  if (partial) {
    mx = wave_sum(mx);
    my = wave_sum(my);
    mz = wave_sum(mz);
    if (tid % kWave == 0) {
      red[0][tid / kWave] = mx;
      red[1][tid / kWave] = my;
      red[2][tid / kWave] = mz;
    }
    __syncthreads();
    if (tid < 3) {
      double acc = 0.0;
      for (int w = 0; w < NT / kWave; ++w) acc += red[tid][w];
      partial[((size_t)b * gridDim.x + tile) * 3 + tid] = acc;
    }
  }
}

// ---- streaming kernels: evaluate, magnetisation, force, initialise ----------------------------------------------------
// per-workgroup partial sums over the vertices of chain b: OP 0 = sigma_n . (sigma_{n+i} + sigma_{n+j}) (the action's bond
// sum), OP 1 = sigma_n (three components); partial[(b * gridDim.x + blockIdx.x) * NV + c]
template <int OP>
__global__ void __launch_bounds__(256) sigma_reduce_kernel(uint32_t Mt, uint32_t Mx, const double2 *__restrict__ phi,
                                                           double *__restrict__ partial) {
  constexpr int NV = OP == 0 ? 1 : 3;
  __shared__ double red[NV][256 / kWave];
  const uint32_t b = blockIdx.y, N = Mt * Mx;
  const double2 *p = phi + (size_t)b * N;
  double acc[NV] = {};
  for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l < N; l += gridDim.x * 256) {
    const V3 s = sigma_of(p[l]);
    if constexpr (OP == 0) {
      const uint32_t i = l % Mt, j = l / Mt;
      const V3 a = sigma_of(p[j * Mt + (i + 1 == Mt ? 0 : i + 1)]);
      const V3 c = sigma_of(p[(j + 1 == Mx ? 0 : j + 1) * Mt + i]);
      acc[0] += s.x * (a.x + c.x) + s.y * (a.y + c.y) + s.z * (a.z + c.z);
    } else {
      acc[0] += s.x;
      acc[1] += s.y;
      acc[2] += s.z;
    }
  }
  for (int c = 0; c < NV; ++c) {
    const double w = wave_sum(acc[c]);
    if (threadIdx.x % kWave == 0) red[c][threadIdx.x / kWave] = w;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0.0;
    for (int w = 0; w < 256 / kWave; ++w) t += red[threadIdx.x][w];
    partial[((size_t)b * gridDim.x + blockIdx.x) * NV + threadIdx.x] = t;
  }
}

// one workgroup per chain: sums the nparts partials of chain b in a fixed order.  OP 0: out[b] = -beta * sum (evaluate);
// OP 1: out[b] = |M|^2 / N (QoI2DMagneticSusceptibility, qoi2dmagneticsusceptibility.cc:7-21) and, with acc, the
// record_sample moments acc[b][5] (mlmcpi_stats_accumulate's recurrence)
template <int OP>
__global__ void __launch_bounds__(256) sigma_finish_kernel(const double *__restrict__ partial, uint32_t nparts, double scale,
                                                           double *__restrict__ out, double *__restrict__ acc) {
  constexpr int NV = OP == 0 ? 1 : 3;
  __shared__ double red[NV][256 / kWave];
  const uint32_t b = blockIdx.x;
  double t[NV] = {};
  for (uint32_t k = threadIdx.x; k < nparts; k += 256)
    for (int c = 0; c < NV; ++c) t[c] += partial[((size_t)b * nparts + k) * NV + c];
  for (int c = 0; c < NV; ++c) {
    const double w = wave_sum(t[c]);
    if (threadIdx.x % kWave == 0) red[c][threadIdx.x / kWave] = w;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double v[NV];
  for (int c = 0; c < NV; ++c) {
    v[c] = 0.0;
    for (int w = 0; w < 256 / kWave; ++w) v[c] += red[c][w];
  }
  double q;
  if constexpr (OP == 0) q = scale * v[0];
  else q = (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) * scale;
  out[b] = q;
  if (acc) record_moments(acc + 5 * (size_t)b, q);
}

// NonlinearSigmaAction::force (nonlinearsigmaaction.cc:94-112): dS/dtheta, dS/dphi per vertex
__global__ void __launch_bounds__(256) sigma_force_kernel(uint32_t Mt, uint32_t Mx, double beta, const double2 *__restrict__ phi,
                                                          double2 *__restrict__ f) {
  const uint32_t b = blockIdx.y, N = Mt * Mx;
  const double2 *p = phi + (size_t)b * N;
  double2 *o = f + (size_t)b * N;
  for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l < N; l += gridDim.x * 256) {
    const uint32_t i = l % Mt, j = l / Mt;
    const V3 Dl = add4(sigma_of(p[j * Mt + (i + 1 == Mt ? 0 : i + 1)]), sigma_of(p[j * Mt + (i == 0 ? Mt - 1 : i - 1)]),
                       sigma_of(p[(j + 1 == Mx ? 0 : j + 1) * Mt + i]), sigma_of(p[(j == 0 ? Mx - 1 : j - 1) * Mt + i]));
    const double2 a = p[l];
    double st, ct, sp, cp;
    sincos(a.x, &st, &ct);
    sincos(a.y, &sp, &cp);
    const double dth = -beta * ((Dl.x * cp + Dl.y * sp) * ct - Dl.z * st);
    const double dph = -beta * (-Dl.x * sp + Dl.y * cp) * st;
    __builtin_nontemporal_store(dth, &o[l].x);
    __builtin_nontemporal_store(dph, &o[l].y);
  }
}

// initialise_state (nonlinearsigmaaction.cc:141-162): uniform on the sphere, cos theta = 1 - 2u, phi = 2 pi u' - pi, with
// u, u' the P_INIT uniforms of entries 2l, 2l + 1 (the same stream as the Schwinger links' initialisation)
__global__ void __launch_bounds__(256) sigma_init_kernel(uint32_t N, RngKey key0, double2 *__restrict__ x) {
  const uint32_t b = blockIdx.y;
  RngKey key = key0;
  key.chain += b;
  double2 *xb = x + (size_t)b * N;
  for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l < N; l += gridDim.x * 256) {
    double u, u2, dummy;
    rng_uniforms(key, 2 * l, P_INIT, 0, u, dummy);
    rng_uniforms(key, 2 * l + 1, P_INIT, 0, u2, dummy);
    xb[l] = make_double2(acos(1.0 - 2.0 * u), -kPi + 2.0 * kPi * u2);
  }
}

// Action::heatbath_update / overrelaxation_update(state, l) for a list of vertices: one thread per chain walks the list in
// order on the state in global memory (mlmcpi_lattice_site_updates), the sweep kernel's arithmetic and random numbers
__global__ void __launch_bounds__(64) sigma_site_update_kernel(uint32_t Mt, uint32_t Mx, double beta, double2 *__restrict__ phi,
                                                               uint32_t B, const uint32_t *__restrict__ sites, uint32_t n,
                                                               uint32_t site, int heat, RngKey key) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  key.chain += b;
  double2 *p = phi + (size_t)b * Mt * Mx;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t l = sites ? sites[k] : site;
    if (l >= Mt * Mx) continue;  // not a vertex: ignored (the list is device memory the host cannot check)
    sigma_site_update(p, Mt, Mx, l, heat != 0, beta, key);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {

uint32_t sigma_blocks(uint32_t N, uint32_t B) { return row_blocks((N + 255) / 256, B); }  // workgroups of 256 per chain

DeviceOnce g_sigma_attr_once;

template <int OP>
int sigma_reduce(uint32_t Mt, uint32_t Mx, const double *d_phi, uint32_t B, double scale, double *d_out, hipStream_t st) {
  constexpr int NV = OP == 0 ? 1 : 3;
  const uint32_t nb = sigma_blocks(Mt * Mx, B);
  void *part = nullptr;
  if (int rc = scratch((size_t)B * nb * NV * sizeof(double), &part, st)) return rc;
  hipLaunchKernelGGL(sigma_reduce_kernel<OP>, dim3(nb, B), dim3(256), 0, st, Mt, Mx, (const double2 *)d_phi, (double *)part);
  MLMCPI_LAUNCH_CHECK("sigma_reduce_kernel");
  hipLaunchKernelGGL(sigma_finish_kernel<OP>, dim3(B), dim3(256), 0, st, (const double *)part, nb, scale, d_out, (double *)nullptr);
  MLMCPI_LAUNCH_CHECK("sigma_finish_kernel");
  return MLMCPI_OK;
}

}  // namespace

int sigma_init_sweep_kernels() {  // once per draw: the sweep kernel may take the whole LDS (of the current device)
  return once_per_device(g_sigma_attr_once, []() -> int {
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sweep_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sweep_kernel<512>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sweep_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    return MLMCPI_OK;
  });
}

int sigma_evaluate(const mlmcpi_lattice_action *act, const double *d_phi, uint32_t B, double *d_S, hipStream_t st) {
  return sigma_reduce<0>(act->Mt, act->Mx, d_phi, B, -act->beta, d_S, st);
}

int sigma_force(const mlmcpi_lattice_action *act, const double *d_phi, double *d_f, uint32_t B, hipStream_t st) {
  hipLaunchKernelGGL(sigma_force_kernel, dim3(sigma_blocks(act->Mt * act->Mx, B), B), dim3(256), 0, st, act->Mt, act->Mx, act->beta,
                     (const double2 *)d_phi, (double2 *)d_f);
  MLMCPI_LAUNCH_CHECK("sigma_force_kernel");
  return MLMCPI_OK;
}

int sigma_initialise(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint64_t seed, uint32_t chain0, hipStream_t st) {
  hipLaunchKernelGGL(sigma_init_kernel, dim3(sigma_blocks(act->Mt * act->Mx, B), B), dim3(256), 0, st, act->Mt * act->Mx,
                     make_key(seed, chain0, 0), (double2 *)d_phi);
  MLMCPI_LAUNCH_CHECK("sigma_init_kernel");
  return MLMCPI_OK;
}

int sigma_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites, uint32_t n,
                       uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, hipStream_t st) {
  hipLaunchKernelGGL(sigma_site_update_kernel, dim3((B + 63) / 64), dim3(64), 0, st, act->Mt, act->Mx, act->beta, (double2 *)d_state,
                     B, d_sites, n, site, (int)heat, make_key(seed, chain0, step));
  MLMCPI_LAUNCH_CHECK("sigma_site_update_kernel");
  return MLMCPI_OK;
}

// one launch of a draw of mlmcpi_lattice_sweep_draw* (lattice2d.hip plans the draw and runs the loop): reads a.src, writes
// a.dst; a.key is that of the launch's first sweep.  a.qoi_op != 0 (the launch ends the draw): it sums the magnetisation, and one
// more launch finishes chi_m into a.d_qoi (and the record_sample moments with a.d_acc).
int sigma_sweep_launch(const SweepLaunch &l, const SweepArgs &a) {
  void *part = nullptr;
  if (int rc = a.qoi_op ? scratch((size_t)a.B * l.grid_x * 3 * sizeof(double), &part, a.st) : 0) return rc;
#define MLMCPI_SIGMA_SWEEP(NT)                                                                                                    \
  hipLaunchKernelGGL(sigma_sweep_kernel<NT>, dim3(l.grid_x, a.B), dim3(NT), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling,            \
                     (const double2 *)a.src, (double2 *)a.dst, l.tile_w, l.tile_h, l.tiles_x, l.n_overrelax + l.n_heatbath, l.n_overrelax, \
                     a.key, (double *)part)
  if (l.threads == 1024) MLMCPI_SIGMA_SWEEP(1024);
  else if (l.threads == 512) MLMCPI_SIGMA_SWEEP(512);
  else MLMCPI_SIGMA_SWEEP(256);
#undef MLMCPI_SIGMA_SWEEP
  MLMCPI_LAUNCH_CHECK("sigma_sweep_kernel");
  if (a.qoi_op) {
    hipLaunchKernelGGL(sigma_finish_kernel<1>, dim3(a.B), dim3(256), 0, a.st, (const double *)part, l.grid_x,
                       1.0 / ((double)a.Mt * a.Mx), a.d_qoi, a.d_acc);
    MLMCPI_LAUNCH_CHECK("sigma_finish_kernel");
  }
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

// QoI2DMagneticSusceptibility::evaluate (qoi/qft/qoi2dmagneticsusceptibility.cc:7-21): chi_m = |sum_n sigma_n|^2 / N
int mlmcpi_qoi_magnetic_susceptibility(const double *d_phi, uint32_t Mt, uint32_t Mx, uint32_t B, double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_phi && d_out && B > 0 && Mt > 1 && Mx > 1, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)Mt * Mx <= (1ull << 30), "lattice too large for 32-bit site indices");
  return sigma_reduce<1>(Mt, Mx, d_phi, B, 1.0 / ((double)Mt * Mx), d_out, as_stream(stream));
}

}  // extern "C"
