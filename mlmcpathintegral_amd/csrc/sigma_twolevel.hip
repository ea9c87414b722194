// sigma_twolevel.hip -- the conditioned fine action of the O(3) nonlinear sigma model and its two-level Metropolis step
// (include/mlmcpi_hip.h: mlmcpi_sigma_cfa_*, mlmcpi_sigma_twolevel_*).
//   NonlinearSigmaConditionedFineAction::{fill_fine_points, evaluate}   action/qft/nonlinearsigmaconditionedfineaction.cc:7-44
//   TwoLevelMetropolisStep::draw                                        montecarlo/twolevelmetropolisstep.cc:35-89
// Under CoarsenRotate every fine-only vertex X of a level has its four neighbours among the coarse vertices (geometry:
// sigma_level_device.hpp), so the fill is one independent heat-bath draw per X and every bond of the fine action joins an X to
// a coarse vertex: S_fine = -beta sum_X sigma_X . Delta_X.  The step is therefore ONE pass over the fine-only vertices: thread x
// builds the trial at X_x and at coarse vertex number x, and adds X_x's terms of the fine action and of the conditioned fine
// action, for the trial and for the current state, and bond term x of the coarse action for the restriction of the current
// state and for the proposal -- six sums per chain, no intermediate state in HBM beyond the trial.  It is a gather: a coarse
// spin is read (and converted, sigma_of) by each of its four fine-only neighbours and once more by the coarse bond term, about
// twenty conversions per thread for some five distinct spins; the repeats come from the cache, not from HBM (timings:
// DESIGN.md 7.6; staging a tile's unit vectors in LDS as the sweep kernel does is the open improvement).
#include "internal.hpp"

#include "sigma_level_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

enum { T_FINE_TRIAL = 0, T_FINE_CUR, T_CFA_TRIAL, T_CFA_CUR, T_COARSE_CUR, T_COARSE_PROP, T_COUNT };

__device__ __forceinline__ V3 delta4(const double2 *__restrict__ p, const uint32_t (&n)[4]) {
  return add4(sigma_of(p[n[0]]), sigma_of(p[n[1]]), sigma_of(p[n[2]]), sigma_of(p[n[3]]));
}

// sigma_0 . (sum of its neighbours) of bond term x of the coarse action, on the state `p` indexed by (i0, in)
__device__ __forceinline__ double coarse_bond(const SigmaLevel &L, const double2 *__restrict__ p, uint32_t i0, const uint32_t (&in)[4]) {
  const V3 s = sigma_of(p[i0]);
  if (L.rot) {  // coarse partner unrotated: the +i and +j neighbours, the expression of sigma_reduce_kernel<0>
    const V3 a = sigma_of(p[in[0]]), c = sigma_of(p[in[1]]);
    return s.x * (a.x + c.x) + s.y * (a.y + c.y) + s.z * (a.z + c.z);
  }
  return dot3(s, delta4(p, in));
}

// grid (ceil(ngroups / G), B), 256 threads; workgroup (w, b) takes groups w G .. w G + G - 1 of chain b, one after the other.
// MODE 0: the two-level pass (trial, six sums); 1: fill in place (theta = the state, no sums); 2: the conditioned fine action of
// theta (partial[.. * 1])
template <int MODE>
__global__ void __launch_bounds__(kGroup)
    sigma_twolevel_pass_kernel(SigmaLevel L, const double2 *__restrict__ coarse_all, double2 *__restrict__ theta_all,
                               double2 *__restrict__ trial_all, uint32_t ngroups, uint32_t G, RngKey key, double *__restrict__ partial) {
  constexpr int NV = MODE == 0 ? (int)T_COUNT : 1;
  __shared__ double red[NV * (kGroup / kWave)];
  const uint32_t b = blockIdx.y, nx = L.nfineonly(), ncb = L.q;
  double2 *theta = theta_all + (size_t)b * L.nvert();
  const double2 *coarse = MODE == 0 ? coarse_all + (size_t)b * nx : nullptr;
  double2 *trial = MODE == 0 ? trial_all + (size_t)b * L.nvert() : nullptr;
  key.chain += b;
  for (uint32_t g = blockIdx.x * G; g < ngroups && g < (blockIdx.x + 1) * G; ++g) {
    const uint32_t x = g * kGroup + threadIdx.x;
    double acc[NV] = {};
    if (x < nx) {
      uint32_t l, nf[4], nc[4];
      fineonly_site(L, x, l, nf, nc);
      if constexpr (MODE == 0) {
        const V3 cur = sigma_of(theta[l]), Dc = delta4(theta, nf), Dt = delta4(coarse, nc);
        double u, v;
        rng_uniforms(key, l, P_SIGMA_FILLIN, 0, u, v);
        const double2 ang = angles_of(sigma_heatbath(cur, Dt, L.beta, u, v));
        const V3 tr = sigma_of(ang);  // what an evaluation of the stored trial reads
        trial[l] = ang;
        uint32_t lc, cc;
        coarse_site(L, x, lc, cc);
        trial[lc] = coarse[cc];
        acc[T_FINE_TRIAL] = dot3(tr, Dt);
        acc[T_FINE_CUR] = dot3(cur, Dc);
        acc[T_CFA_TRIAL] = sigma_cfa_term(tr, Dt, L.beta);
        acc[T_CFA_CUR] = sigma_cfa_term(cur, Dc, L.beta);
        if (x < ncb) {
          uint32_t c0, f0, cn[4], fn[4];
          coarse_bond_site(L, x, c0, f0, cn, fn);
          acc[T_COARSE_CUR] = coarse_bond(L, theta, f0, fn);
          acc[T_COARSE_PROP] = coarse_bond(L, coarse, c0, cn);
        }
      } else if constexpr (MODE == 1) {
        double u, v;
        rng_uniforms(key, l, P_SIGMA_FILLIN, 0, u, v);
        theta[l] = angles_of(sigma_heatbath(sigma_of(theta[l]), delta4(theta, nf), L.beta, u, v));
      } else {
        acc[0] = sigma_cfa_term(sigma_of(theta[l]), delta4(theta, nf), L.beta);
      }
    }
    if constexpr (MODE != 1) {
      block_sum<NV>(acc, red);
      if (threadIdx.x == 0)
        for (int c = 0; c < NV; ++c) partial[((size_t)b * ngroups + g) * NV + c] = acc[c];
      __syncthreads();  // red is reused by the next group
    }
  }
}

// one workgroup per chain: the six sums, the three differences with the reference's signs (twolevelmetropolisstep.cc:46-70) and
// the Metropolis test of lattice_twolevel_accept_kernel (Philox site 0, purpose P_ACCEPT2)
__global__ void __launch_bounds__(kGroup)
    sigma_twolevel_decide_kernel(const double *__restrict__ partial, uint32_t ngroups, double beta, double beta_coarse,
                                 int32_t *__restrict__ accept, double *__restrict__ terms, RngKey key) {
  __shared__ double red[T_COUNT * (kGroup / kWave)];
  const uint32_t b = blockIdx.x;
  double v[T_COUNT];
  chain_sum<T_COUNT>(partial + (size_t)b * ngroups * T_COUNT, ngroups, v, red);
  if (threadIdx.x != 0) return;
  const double dS_fine = -beta * v[T_FINE_TRIAL] - (-beta * v[T_FINE_CUR]);
  const double dS_coarse = -beta_coarse * v[T_COARSE_CUR] - (-beta_coarse * v[T_COARSE_PROP]);
  const double dS_trial = v[T_CFA_CUR] - v[T_CFA_TRIAL];
  const double dS = dS_fine + dS_coarse + dS_trial;
  bool acc;
  if (dS < 0.0) {
    acc = true;
  } else {
    key.chain += b;
    double u, w;
    rng_uniforms(key, 0, P_ACCEPT2, 0, u, w);
    acc = u < exp(-dS);
  }
  accept[b] = acc ? 1 : 0;
  if (terms) {
    terms[3 * b + 0] = dS_fine;
    terms[3 * b + 1] = dS_coarse;
    terms[3 * b + 2] = dS_trial;
  }
}

// theta[b] <- trial[b] for the accepted chains
__global__ void __launch_bounds__(256) sigma_twolevel_copy_kernel(uint32_t n, double2 *__restrict__ theta, const double2 *__restrict__ trial,
                                                                  const int32_t *__restrict__ accept) {
  const uint32_t b = blockIdx.y;
  if (!accept[b]) return;
  const size_t off = (size_t)b * n;
  for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l < n; l += gridDim.x * 256) theta[off + l] = trial[off + l];
}

// one workgroup per chain: out[b] = the sum of the chain's group partials
__global__ void __launch_bounds__(kGroup) sigma_cfa_finish_kernel(const double *__restrict__ partial, uint32_t ngroups, double *__restrict__ out) {
  __shared__ double red[kGroup / kWave];
  double v[1];
  chain_sum<1>(partial + (size_t)blockIdx.x * ngroups, ngroups, v, red);
  if (threadIdx.x == 0) out[blockIdx.x] = v[0];
}

namespace {
uint32_t groups_of(const SigmaLevel &L) { return (L.nfineonly() + kGroup - 1) / kGroup; }
uint32_t groups_per_workgroup() {
  const uint32_t g = tuning().sigma_twolevel_groups;
  return g ? g : 1u;
}
}  // namespace

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_cfa_fill(const mlmcpi_sigma_level *fine, double *d_state, uint32_t B, uint64_t seed, uint32_t chain0,
                          uint32_t step, void *stream) {
  if (int rc = check_sigma_level(fine)) return rc;
  MLMCPI_REQUIRE(d_state && B > 0 && B <= 65535, "bad arguments");
  const SigmaLevel L = make_level(*fine);
  const uint32_t ng = groups_of(L), G = groups_per_workgroup();
  hipLaunchKernelGGL(sigma_twolevel_pass_kernel<1>, dim3((ng + G - 1) / G, B), dim3(kGroup), 0, as_stream(stream), L,
                     (const double2 *)nullptr, (double2 *)d_state, (double2 *)nullptr, ng, G, make_key(seed, chain0, step), (double *)nullptr);
  MLMCPI_LAUNCH_CHECK("sigma_twolevel_pass_kernel<fill>");
  return MLMCPI_OK;
}

int mlmcpi_sigma_cfa_evaluate(const mlmcpi_sigma_level *fine, const double *d_state, uint32_t B, double *d_S, void *stream) {
  if (int rc = check_sigma_level(fine)) return rc;
  MLMCPI_REQUIRE(d_state && d_S && B > 0 && B <= 65535, "bad arguments");
  hipStream_t st = as_stream(stream);
  const SigmaLevel L = make_level(*fine);
  const uint32_t ng = groups_of(L), G = groups_per_workgroup();
  void *part = nullptr;
  if (int rc = scratch((size_t)B * ng * sizeof(double), &part, st)) return rc;
  hipLaunchKernelGGL(sigma_twolevel_pass_kernel<2>, dim3((ng + G - 1) / G, B), dim3(kGroup), 0, st, L, (const double2 *)nullptr,
                     (double2 *)d_state, (double2 *)nullptr, ng, G, make_key(0, 0, 0), (double *)part);
  MLMCPI_LAUNCH_CHECK("sigma_twolevel_pass_kernel<cfa>");
  hipLaunchKernelGGL(sigma_cfa_finish_kernel, dim3(B), dim3(kGroup), 0, st, (const double *)part, ng, d_S);
  MLMCPI_LAUNCH_CHECK("sigma_cfa_finish_kernel");
  return MLMCPI_OK;
}

static int check_partner(const mlmcpi_sigma_level *fine, const mlmcpi_sigma_level *coarse) {
  if (int rc = check_sigma_level(fine)) return rc;
  if (int rc = check_sigma_level(coarse)) return rc;
  const bool ok = fine->rotated ? (!coarse->rotated && 2 * coarse->Mt == fine->Mt && 2 * coarse->Mx == fine->Mx)
                                : (coarse->rotated && coarse->Mt == fine->Mt && coarse->Mx == fine->Mx);
  if (!ok)
    return fail(MLMCPI_ERR_INVALID, "the coarse level (%u x %u%s) is not the CoarsenRotate partner of the fine level (%u x %u%s)", coarse->Mt,
                coarse->Mx, coarse->rotated ? ", rotated" : "", fine->Mt, fine->Mx, fine->rotated ? ", rotated" : "");
  return MLMCPI_OK;
}

// workspace: the trial | the group partials [B][ngroups][6]
int mlmcpi_sigma_twolevel_workspace_bytes(const mlmcpi_sigma_level *fine, uint32_t B, size_t *bytes) {
  if (int rc = check_sigma_level(fine)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0 && B <= 65535, "bad arguments");
  const SigmaLevel L = make_level(*fine);
  *bytes = align256((size_t)B * 2 * L.nvert() * 8) + align256((size_t)B * groups_of(L) * T_COUNT * 8);
  return MLMCPI_OK;
}

int mlmcpi_sigma_twolevel_draw(const mlmcpi_sigma_level *fine, const mlmcpi_sigma_level *coarse, const double *d_phi_coarse,
                               double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work,
                               int32_t *d_accept, double *d_terms, void *stream) {
  if (int rc = check_partner(fine, coarse)) return rc;
  MLMCPI_REQUIRE(d_phi_coarse && d_theta && d_work && d_accept && B > 0 && B <= 65535, "bad arguments");
  hipStream_t st = as_stream(stream);
  const SigmaLevel L = make_level(*fine);
  const uint32_t ng = groups_of(L), G = groups_per_workgroup();
  double2 *trial = (double2 *)d_work;
  double *partial = (double *)((char *)d_work + align256((size_t)B * 2 * L.nvert() * 8));
  const RngKey key = make_key(seed, chain0, step);
  hipLaunchKernelGGL(sigma_twolevel_pass_kernel<0>, dim3((ng + G - 1) / G, B), dim3(kGroup), 0, st, L,
                     (const double2 *)d_phi_coarse, (double2 *)d_theta, trial, ng, G, key, partial);
  MLMCPI_LAUNCH_CHECK("sigma_twolevel_pass_kernel");
  hipLaunchKernelGGL(sigma_twolevel_decide_kernel, dim3(B), dim3(kGroup), 0, st, (const double *)partial, ng, fine->beta, coarse->beta,
                     d_accept, d_terms, key);
  MLMCPI_LAUNCH_CHECK("sigma_twolevel_decide_kernel");
  hipLaunchKernelGGL(sigma_twolevel_copy_kernel, dim3(stream_blocks(L.nvert()), B), dim3(256), 0, st, L.nvert(), (double2 *)d_theta,
                     (const double2 *)trial, (const int32_t *)d_accept);
  MLMCPI_LAUNCH_CHECK("sigma_twolevel_copy_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
