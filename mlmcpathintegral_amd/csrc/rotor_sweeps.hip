// rotor_sweeps.hip -- the topological rotor's overrelaxation / heat-bath sweeps (even / odd colouring) on LDS-resident
// segments, with both heat-bath samplers, and its site-at-a-time updates.  Both kernels stay in this unit: each reaches
// the step-envelope sampler's device functions that are not inlined, and the compiler specialises those for the callers a unit has.
#include "path_common.hpp"
#include "step_envelope.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// ---- rotor sweeps -----------------------------------------------------------------------------------
// Grid (nseg, B), 256 threads.  The segment plus a halo of 2 sites per fused sweep lives in LDS;
// every site whose two neighbours are inside the buffer is updated, so stale values creep inwards
// by at most two sites per sweep and never reach the owned range.  in != out (halo reads race with
// the neighbours' writes otherwise).  kinds bit s = 1 -> sweep s is a heat-bath sweep.
// rotoraction.cc:20-56, rotoraction.hh:195-213.
// HEAT = false: overrelaxation-only instantiation (no sampler code, few registers).  STEP: heat-bath draws from the step
// envelope (2 m0 / a <= kVsKappaMax, step_envelope.hpp) instead of the wrapped-Cauchy one; pool_cap then counts VsPool entries.
#ifndef MLMCPI_ROTOR_LEAN
#define MLMCPI_ROTOR_LEAN 2
#endif
#ifndef MLMCPI_ROTOR_WAVES
#define MLMCPI_ROTOR_WAVES 1
#endif
template <bool HEAT, bool STEP = false>
__global__ void __launch_bounds__(256, HEAT && STEP ? MLMCPI_ROTOR_WAVES : 1)
    rotor_sweep_kernel(PathP P, const double *__restrict__ in, double *__restrict__ out, uint32_t owned_len,
                       uint32_t nsweeps, uint32_t kinds, RngKey key0, uint32_t pool_cap, const uint32_t *__restrict__ vs_table,
                       double *__restrict__ winding_partial = nullptr, uint32_t n_closed = 0) {
  extern __shared__ double lds_all[];
  __shared__ double qoi_red[4];
  // winding_partial != NULL: the segment's share of sum_j mod_2pi(x_j - x_{j-1}) (qoi/qm/qoisusceptibility.cc:8-23) of the
  // NEW state goes out with it; the left neighbour of the first owned site has to be exact for that: one more pair of halo sites
  const uint32_t b = blockIdx.y, seg = blockIdx.x, M = P.M, halo = 2 * nsweeps + (winding_partial ? 2u : 0u);
  // the sampler's tables and the list of open cells at the START of the LDS (table look-ups are then instruction offsets, not
  // additions of a wave-uniform base at half rate: r04, -4 % on the sweeps), the segment image behind them
  HbPool pool = HbPool::carve(lds_all, HEAT && !STEP ? pool_cap : 0u);
  VsPool<uint32_t> vpool = VsPool<uint32_t>::carve(lds_all, HEAT && STEP ? pool_cap : 0u, STEP ? vs_table : nullptr);
  double *const buf = lds_all + (HEAT ? (STEP ? VsPool<uint32_t>::bytes(pool_cap) : HbPool::bytes(pool_cap)) / sizeof(double) : 0);
  const uint32_t o0 = seg * owned_len, olen = min(owned_len, M - o0);
  const uint32_t L = olen + 2 * halo;
  const uint32_t g0 = (uint32_t)(((uint64_t)o0 + M - (halo % M)) % M);
  const double *xin = in + (size_t)b * M;
  RngKey key = key0;
  key.chain += b;
  for (uint32_t k = threadIdx.x; k < L; k += blockDim.x) {
    uint32_t g = g0 + k;  // g0 < M and M < 2^31 for every supported lattice: no overflow; no 64-bit modulo per element
    while (g >= M) g -= M;
    buf[k] = xin[g];
  }
  __syncthreads();
  const double sig_scale = 2.0 * P.m0 / P.a;  // W'' = (2 m0 / a) |cos((x+ - x-)/2)|
  // The first n_closed sweeps of the launch -- overrelaxation sweeps -- in closed form.  The update x_j <- x_{j-1} + x_{j+1} - x_j
  // (rotoraction.cc:40-56) adds d_j - d_{j-1} to x_j, d_j = x_{j+1} - x_j, and leaves the two differences exchanged; in
  // even / odd order a sweep moves the difference at an even index two down and the one at an odd index two up, whatever
  // the path is, so K sweeps add to the pair of sites (j, j + 1), j = 2 p even,
  //     x_j     += X - S,     S = sum_{s<K} d(j - 1 - 2 s) = sum_s do[p - 1 - s],    X  = sum_{s<K} d(j + 2 s) = sum_s de[p + s],
  //     x_{j+1} += X' - S,                                                           X' = X - de[p] + de[p + K]
  // with the differences of the path the launch started from, split by parity (de[i] = d(2 i), do[i] = d(2 i + 1): every
  // sum is a run of consecutive LDS words, consecutive lanes read consecutive words).  The same map as K sweeps to the
  // rounding of 2 K additions (the 2-D counterpart: schwinger_perm.hpp, schwinger_perm_kernel); exact where the sweeps are
  // (buffer sites [2 K, L - 2 K)), the edge sites keep their values as they do under the sweeps' creeping halo.
  if (n_closed) {
    const uint32_t H2 = L / 2, K = n_closed;   // L is even (owned lengths, halos and M are) and at most 2048: <= 4 pairs per thread
    double xa[4], xb[4], dev[4], dov[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint32_t p = threadIdx.x + 256 * m;
      if (p < H2) {
        xa[m] = buf[2 * p];
        xb[m] = buf[2 * p + 1];
        dev[m] = xb[m] - xa[m];
        dov[m] = (2 * p + 2 < L ? buf[2 * p + 2] : xb[m]) - xb[m];
      }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint32_t p = threadIdx.x + 256 * m;
      if (p < H2) {
        buf[p] = dev[m];
        buf[H2 + p] = dov[m];
      }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint32_t p = threadIdx.x + 256 * m;
      if (p >= K && p + K < H2) {
        double S = 0.0, X = 0.0;
        const double *od = buf + H2 + p - 1, *ev = buf + p;
        for (uint32_t q = 0; q < K; ++q) {
          S += od[-(int)q];
          X += ev[q];
        }
        const double X2 = (X - ev[0]) + ev[K];
        xa[m] = mod_2pi_fast(xa[m] + (X - S));
        xb[m] = mod_2pi_fast(xb[m] + (X2 - S));
      }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint32_t p = threadIdx.x + 256 * m;
      if (p < H2) {
        buf[2 * p] = xa[m];
        buf[2 * p + 1] = xb[m];
      }
    }
    __syncthreads();
  }
  for (uint32_t s = n_closed; s < nsweeps; ++s) {
    const bool heat = HEAT && ((kinds >> s) & 1u);
    RngKey skey = key;
    skey.step += s;
    for (uint32_t colour = 0; colour < 2; ++colour) {
      // buffer parity == global parity (g0 is even because o0, halo and M are); sites k = k0, k0 + 2, ... < L - 1
      // with k0 = 2 for colour 0 and 1 for colour 1.  getWminimum (rotoraction.hh:206-213) in closed form:
      // atan2(sin x+ + sin x-, cos x+ + cos x-) = (x+ + x-)/2 (+ pi when cos((x+ - x-)/2) < 0), so that
      //   overrelaxation  mod_2pi(2 x0 - x) = mod_2pi(x+ + x- - x)                 (no transcendental at all)
      //   heat bath       mod_2pi(x0 + ExpSin2(2 W'')),  kappa = W'' = (2 m0/a) |cos((x+ - x-)/2)|  (one cosine)
      const uint32_t k0 = 2 - colour;
      const uint32_t count = (L > k0 + 1) ? (L - 1 - k0 + 1) / 2 : 0;
      if (!heat) {
        for (uint32_t idx = threadIdx.x; idx < count; idx += blockDim.x) {
          const uint32_t k = k0 + 2 * idx;
          buf[k] = mod_2pi_fast(buf[k - 1] + buf[k + 1] - buf[k]);
        }
      } else if (HEAT && STEP) {
        auto global_site = [&](uint32_t k) {
          uint32_t g = g0 + k;
          while (g >= M) g -= M;
          return g;
        };
        heatbath_cells_step<256, 4, uint32_t, MLMCPI_ROTOR_LEAN>(
            count, skey, vpool, [&](uint32_t idx) { return k0 + 2 * idx; },
            [&](uint32_t k, VsCell &cell) {
              vs_cell(sig_scale, buf[k + 1], buf[k - 1], cell);
              cell.site = global_site(k);
            },
            [&](uint32_t k) { return vs_kappa_exact(sig_scale, buf[k + 1], buf[k - 1]); },
            [&](uint32_t k, double angle) { buf[k] = angle; });
      } else if (HEAT) {
        heatbath_cells<256, 4, true>(
            count, skey, pool,
            [&](uint32_t idx, double &tau, double &centre, uint32_t &site, uint32_t &off) {
              const uint32_t k = k0 + 2 * idx;
              const double xm = buf[k - 1], xp = buf[k + 1];
              // |x+ - x-| / 2 <= pi: cos(d) = cos(pi u), u = |x+ - x-| / (2 pi) in [0, 1] (no libm range reduction)
              const double c = cospi_unit(fmin(fabs(xp - xm) * (0.5 / kPi), 1.0));
              tau = sig_scale * fabs(c);
              centre = 0.5 * (xp + xm) + (c < 0.0 ? kPi : 0.0);
              uint32_t g = g0 + k;
              while (g >= M) g -= M;
              site = g;
              off = k;
            },
            [&](uint32_t off, double angle) { buf[off] = angle; });
      }
      __syncthreads();
    }
  }
  double *xout = out + (size_t)b * M;
  double acc[1] = {0.0};
  for (uint32_t k = threadIdx.x; k < olen; k += blockDim.x) {
    xout[o0 + k] = buf[halo + k];
    if (winding_partial) acc[0] += mod_2pi(buf[halo + k] - buf[halo + k - 1]);
  }
  if (winding_partial) {
    block_sum<1>(acc, qoi_red);
    if (threadIdx.x == 0) winding_partial[(size_t)b * gridDim.x + seg] = acc[0];
  }
}

// Site-at-a-time rotor updates (rotoraction.cc:20-56 through Action::heatbath_update / overrelaxation_update,
// action/action.hh:73-96): one thread per chain walks the site list in order, on the state in global memory; arithmetic
// and random numbers of rotor_sweep_kernel.
__global__ void __launch_bounds__(64)
    rotor_site_update_kernel(PathP P, double *__restrict__ x_all, uint32_t B, const uint32_t *__restrict__ sites, uint32_t n,
                             uint32_t single, int heat, RngKey key0, const uint32_t *__restrict__ vs_table) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  RngKey key = key0;
  key.chain += b;
  double *x = x_all + (size_t)b * P.M;
  const double sig_scale = 2.0 * P.m0 / P.a;
  const bool step = sig_scale <= kVsKappaMax;
  const VsTable tab = VsTable::in_global(vs_table);
  for (uint32_t q = 0; q < n; ++q) {
    const uint32_t l = sites ? sites[q] : single;
    const double xm = x[l == 0 ? P.M - 1 : l - 1], xp = x[l + 1 == P.M ? 0 : l + 1];
    if (!heat) {
      x[l] = mod_2pi_fast(xm + xp - x[l]);
    } else if (step) {
      x[l] = vs_draw(key, l, sig_scale, xp, xm, tab);
    } else {
      const double c = cospi_unit(fmin(fabs(xp - xm) * (0.5 / kPi), 1.0));
      const double centre = 0.5 * (xp + xm) + (c < 0.0 ? kPi : 0.0);
      x[l] = mod_2pi_fast(vonmises_draw(key, l, sig_scale * fabs(c)) + centre);
    }
  }
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

// see sweep_draw_impl of lattice2d.hip: reads d_x first, then alternates between d_w0 and d_w1 (which may be d_x)
static int path_sweep_impl(const mlmcpi_path_action *act, double *d_x, double *d_w0, double *d_w1, uint32_t B,
                           uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                           uint32_t sweep0, int32_t *result_in, void *stream, double *d_qoi = nullptr, double *d_acc = nullptr) {
  if (int rc = check_action(act)) return rc;
  // action/action.hh:73-96: only the rotor implements local updates among the 1-D actions
  if (act->kind != MLMCPI_ROTOR)
    return fail(MLMCPI_ERR_UNSUPPORTED, "heat bath / overrelaxation update not implemented for this action");
  MLMCPI_REQUIRE(d_x && d_w0 && d_w1 && d_x != d_w0 && d_w0 != d_w1 && B > 0, "bad arguments");
  MLMCPI_REQUIRE(act->M % 2 == 0, "even/odd sweeps need an even number of sites (M_lat = %u)", act->M);
  // the chains are gridDim.y of every launch below
  MLMCPI_REQUIRE(B <= 65535, "at most 65535 chains per call (B = %u): split the batch", B);
  PathP P = make_params(*act);
  hipStream_t st = as_stream(stream);
  const uint32_t total = n_overrelax + n_heatbath;
  const Tuning tune = tuning();
  const bool split_heat = tune.or_heat_split, closed = !tune.or_block;
  double *src = d_x, *dst = d_w0;
  uint32_t s = 0;
  while (s < total) {
    // overrelaxation sweeps (they come first, sampler order) are fused up to 8 per launch: in one dimension the halo
    // of 2 sites per sweep costs next to nothing; a heat-bath sweep gets a launch of its own (sampler-bound)
    uint32_t n = 1, kinds = 0, n_closed = 0;
    if (s < n_overrelax) {
      // overrelaxation in closed form (rotor_sweep_kernel; MLMCPI_OR_KERNEL=block: sweep by sweep): up to 16 sweeps per launch
      const uint32_t cap = closed ? 16u : 8u;
      n = n_overrelax - s < cap ? n_overrelax - s : cap;
      if (closed) n_closed = n;
      // the last overrelaxation launch takes the heat-bath sweep behind it along (one pass over the state less; the sweeps
      // of a launch are numbered on from its key, so the draws are those of two launches: MLMCPI_OR_HEAT=split)
      if (!split_heat && s + n == n_overrelax && n_heatbath >= 1 && (n < cap || closed)) {
        kinds = 1u << n;
        ++n;
      }
    } else
      kinds = 1u;
    // the draw's last launch can sum the topological charge of the new state while the segment is in LDS (d_qoi)
    const bool with_qoi = d_qoi && s + n == total;
    const uint32_t halo = 2 * n + (with_qoi ? 2 : 0);
    uint32_t owned = 2048 - 2 * halo;  // even
    if (owned > P.M) owned = P.M;
    const uint32_t nseg = (P.M + owned - 1) / owned;
    owned = (P.M + nseg - 1) / nseg;
    owned += owned & 1;  // keep segment starts even
    const uint32_t nseg2 = (P.M + owned - 1) / owned;
    const size_t lds = (size_t)(owned + 2 * halo) * sizeof(double);
    // retry pool of the heat-bath phases (vonmises.hpp, step_envelope.hpp); which sampler: a property of the action (2 m0 / a), not a knob
    const bool step = 2.0 * P.m0 / P.a <= kVsKappaMax;
    const uint32_t pool_cap = 256;
    const uint32_t *vs_table = nullptr;
    if (kinds && step)
      if (int rc = vs_table_device(2.0 * P.m0 / P.a, &vs_table)) return rc;
    void *partial = nullptr;
    if (with_qoi)
      if (int rc = scratch((size_t)B * nseg2 * sizeof(double), &partial, st)) return rc;
    if (kinds && step)
      hipLaunchKernelGGL((rotor_sweep_kernel<true, true>), dim3(nseg2, B), dim3(256), lds + VsPool<uint32_t>::bytes(pool_cap), st, P,
                         (const double *)src, dst, owned, n, kinds, make_key(seed, chain0, sweep0 + s), pool_cap, vs_table, (double *)partial, n_closed);
    else if (kinds)
      hipLaunchKernelGGL(rotor_sweep_kernel<true>, dim3(nseg2, B), dim3(256), lds + HbPool::bytes(pool_cap), st, P,
                         (const double *)src, dst, owned, n, kinds, make_key(seed, chain0, sweep0 + s), pool_cap, vs_table, (double *)partial, n_closed);
    else
      hipLaunchKernelGGL(rotor_sweep_kernel<false>, dim3(nseg2, B), dim3(256), lds, st, P, (const double *)src, dst, owned, n,
                         kinds, make_key(seed, chain0, sweep0 + s), 0u, vs_table, (double *)partial, n_closed);
    MLMCPI_LAUNCH_CHECK("rotor_sweep_kernel");
    if (with_qoi) {
      if (int rc = path_finish((const double *)partial, nseg2, B, R_WINDING, 1.0 / act->T_final, d_qoi, d_acc, st)) return rc;
    }
    src = dst;
    dst = (dst == d_w0) ? d_w1 : d_w0;
    s += n;
  }
  if (result_in)
    *result_in = total == 0 ? -1 : (src == d_w0 ? 0 : 1);
  else if (src != d_x)
    MLMCPI_HIP_TRY(hipMemcpyAsync(d_x, src, (size_t)B * P.M * 8, hipMemcpyDeviceToDevice, st));
  return MLMCPI_OK;
}

int mlmcpi_path_site_updates(const mlmcpi_path_action *act, double *d_x, uint32_t B, const uint32_t *d_sites, uint32_t n,
                             uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, void *stream) {
  if (int rc = check_action(act)) return rc;
  if (act->kind != MLMCPI_ROTOR)
    return fail(MLMCPI_ERR_UNSUPPORTED, "heat bath / overrelaxation update not implemented for this action");
  MLMCPI_REQUIRE(d_x && B > 0, "bad arguments");
  if (!d_sites) {
    MLMCPI_REQUIRE(site < act->M, "site %u out of range (%u sites)", site, act->M);
    n = 1;
  }
  if (n == 0) return MLMCPI_OK;
  const PathP P = make_params(*act);
  const uint32_t *vs_table = nullptr;
  if (heat && 2.0 * P.m0 / P.a <= kVsKappaMax)
    if (int rc = vs_table_device(2.0 * P.m0 / P.a, &vs_table)) return rc;
  hipLaunchKernelGGL(rotor_site_update_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), P, d_x, B, d_sites, n, site,
                     (int)heat, make_key(seed, chain0, step), vs_table);
  MLMCPI_LAUNCH_CHECK("rotor_site_update_kernel");
  return MLMCPI_OK;
}

int mlmcpi_path_sweep_draw(const mlmcpi_path_action *act, double *d_x, double *d_scratch, uint32_t B,
                           uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                           uint32_t sweep0, void *stream) {
  return path_sweep_impl(act, d_x, d_scratch, d_x, B, n_overrelax, n_heatbath, seed, chain0, sweep0, nullptr, stream);
}

int mlmcpi_path_sweep_draw_from(const mlmcpi_path_action *act, const double *d_src, double *d_w0, double *d_w1, uint32_t B,
                                uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                                int32_t *result_in, void *stream) {
  MLMCPI_REQUIRE(result_in, "result_in is NULL");
  MLMCPI_REQUIRE(n_overrelax + n_heatbath > 0, "no sweeps requested: the result would be the (read-only) input");
  return path_sweep_impl(act, const_cast<double *>(d_src), d_w0, d_w1, B, n_overrelax, n_heatbath, seed, chain0, sweep0,
                         result_in, stream);
}

int mlmcpi_path_sweep_draw_qoi(const mlmcpi_path_action *act, const double *d_src, double *d_w0, double *d_w1, uint32_t B,
                               uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                               double *d_qoi, double *d_acc, int32_t *result_in, void *stream) {
  MLMCPI_REQUIRE(result_in && d_qoi, "result_in or d_qoi is NULL");
  MLMCPI_REQUIRE(n_overrelax + n_heatbath > 0, "no sweeps requested: the result would be the (read-only) input");
  return path_sweep_impl(act, const_cast<double *>(d_src), d_w0, d_w1, B, n_overrelax, n_heatbath, seed, chain0, sweep0,
                         result_in, stream, d_qoi, d_acc);
}

}  // extern "C"
