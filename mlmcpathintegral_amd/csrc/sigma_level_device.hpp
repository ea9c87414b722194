// sigma_level_device.hpp -- what the level kernels of the O(3) sigma model share (sigma_levels.hip, sigma_twolevel.hip): the
// geometry of a level of the CoarsenRotate hierarchy and the plan-independent reduction.  Includes sigma_device.hpp, so the
// including file is compiled without fp contraction.
//
// A level is (Mt, Mx, rotated): extents of the Cartesian frame of Lattice2D, both even.  Unrotated: Mt Mx vertices, l = Mt j + i.
// Rotated: the vertices with (i + j) even, Mt Mx / 2 of them, in two planes of ht x hx = Mt/2 x Mx/2: the even-even plane E
// first, then the odd-odd plane O; index p q + ht b + a (q = ht hx) is the vertex (2 a + p, 2 b + p) (lattice2d.hh:230-268).
// Neighbours in the reference's order (lattice2d.cc:137-155): unrotated (+1, 0), (-1, 0), (0, +1), (0, -1); rotated (+1, +1),
// (+1, -1), (-1, +1), (-1, -1), i.e. for E(a, b): O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1) and for O(a, b): E(a+1, b+1),
// E(a+1, b), E(a, b+1), E(a, b).
//
// CoarsenRotate (lattice2d.cc:83-108): the coarse partner of an unrotated (Mt, Mx) is the rotated (Mt, Mx), fine vertex (i, j)
// with (i + j) even <-> its rotated index; the coarse partner of a rotated (Mt, Mx) is the unrotated (Mt/2, Mx/2), the E plane
// index for index.  The fine-only vertices ((i + j) odd; the O plane) have coarse neighbours only.
#pragma once
#include "sigma_device.hpp"

namespace mlmcpi {

struct SigmaLevel {
  uint32_t Mt, Mx, ht, hx, q;  // q = ht hx
  int rot;
  double beta;
  __host__ __device__ uint32_t nvert() const { return rot ? 2 * q : 4 * q; }
  __host__ __device__ uint32_t nfineonly() const { return rot ? q : 2 * q; }  // = the number of coarse vertices of the level
};

inline SigmaLevel make_level(const mlmcpi_sigma_level &l) {
  return SigmaLevel{l.Mt, l.Mx, l.Mt / 2, l.Mx / 2, (l.Mt / 2) * (l.Mx / 2), l.rotated != 0 ? 1 : 0, l.beta};
}

// rotated index of the vertex (i, j), (i + j) even, 0 <= i < Mt, 0 <= j < Mx
__device__ __forceinline__ uint32_t rot_index(const SigmaLevel &L, uint32_t i, uint32_t j) { return (i & 1u) * L.q + (j >> 1) * L.ht + (i >> 1); }

// fine-only vertex number x (0 <= x < nfineonly) of the level: its index l and its four neighbours in the reference's order,
// as indices on the level (nf) and on the level's coarse partner (nc)
__device__ __forceinline__ void fineonly_site(const SigmaLevel &L, uint32_t x, uint32_t &l, uint32_t (&nf)[4], uint32_t (&nc)[4]) {
  if (L.rot) {
    const uint32_t a = x % L.ht, b = x / L.ht, ap = a + 1 == L.ht ? 0 : a + 1, bp = b + 1 == L.hx ? 0 : b + 1;
    l = L.q + x;
    nf[0] = bp * L.ht + ap;
    nf[1] = b * L.ht + ap;
    nf[2] = bp * L.ht + a;
    nf[3] = b * L.ht + a;
    for (int k = 0; k < 4; ++k) nc[k] = nf[k];
  } else {
    const uint32_t j = x / L.ht, i = 2 * (x % L.ht) + ((j + 1) & 1u);
    const uint32_t ip = i + 1 == L.Mt ? 0 : i + 1, im = i == 0 ? L.Mt - 1 : i - 1;
    const uint32_t jp = j + 1 == L.Mx ? 0 : j + 1, jm = j == 0 ? L.Mx - 1 : j - 1;
    l = j * L.Mt + i;
    nf[0] = j * L.Mt + ip;
    nf[1] = j * L.Mt + im;
    nf[2] = jp * L.Mt + i;
    nf[3] = jm * L.Mt + i;
    nc[0] = rot_index(L, ip, j);
    nc[1] = rot_index(L, im, j);
    nc[2] = rot_index(L, i, jp);
    nc[3] = rot_index(L, i, jm);
  }
}

// coarse vertex number x (0 <= x < nfineonly) of the level: its index l on the level and c on the coarse partner
__device__ __forceinline__ void coarse_site(const SigmaLevel &L, uint32_t x, uint32_t &l, uint32_t &c) {
  if (L.rot) {
    l = c = x;
  } else {
    const uint32_t j = x / L.ht, i = 2 * (x % L.ht) + (j & 1u);
    l = j * L.Mt + i;
    c = rot_index(L, i, j);
  }
}

// bond term number x of the coarse partner's action, 0 <= x < q: the coarse vertex and the coarse vertices it is summed
// against, as indices on the coarse partner (c0, cn) and on the fine level L (f0, fn).  Fine unrotated -> coarse rotated: E(a, b)
// and its four O neighbours, S_c = -beta_c sum sigma_E . add4(...).  Fine rotated -> coarse unrotated (ht, hx): vertex n with its
// +i and +j neighbours (n_nb = 2), S_c = -beta_c sum sigma_n . (sigma_{n+i} + sigma_{n+j}), the bond sum of sigma2d.hip.
__device__ __forceinline__ void coarse_bond_site(const SigmaLevel &L, uint32_t x, uint32_t &c0, uint32_t &f0, uint32_t (&cn)[4],
                                                 uint32_t (&fn)[4]) {
  const uint32_t a = x % L.ht, b = x / L.ht;
  if (L.rot) {
    const uint32_t ap = a + 1 == L.ht ? 0 : a + 1, bp = b + 1 == L.hx ? 0 : b + 1;
    c0 = f0 = x;
    cn[0] = fn[0] = b * L.ht + ap;
    cn[1] = fn[1] = bp * L.ht + a;
    cn[2] = fn[2] = cn[3] = fn[3] = 0;
  } else {
    const uint32_t am = a == 0 ? L.ht - 1 : a - 1, bm = b == 0 ? L.hx - 1 : b - 1;
    c0 = x;
    f0 = (2 * b) * L.Mt + 2 * a;
    const uint32_t oa[4] = {a, a, am, am}, ob[4] = {b, bm, b, bm};
    for (int k = 0; k < 4; ++k) {
      cn[k] = L.q + ob[k] * L.ht + oa[k];
      fn[k] = (2 * ob[k] + 1) * L.Mt + 2 * oa[k] + 1;
    }
  }
}

// -log p(z; s) of the density p(z) = s exp(s z) / (2 sinh s) on [-1, 1] (distribution/compactexpdistribution.cc) for a spin sig
// under the neighbour sum Dl, s = beta |Dl|, z = sig . Dl / |Dl|:  log p = s (z - 1) + log s - log(1 - exp(-2 s)), which
// neither overflows at large s nor cancels at small s; Dl = 0 gives the uniform density 1/2.
__device__ __forceinline__ double sigma_cfa_term(const V3 &sig, const V3 &Dl, double beta) {
  const double n2 = Dl.x * Dl.x + Dl.y * Dl.y + Dl.z * Dl.z;
  if (!(n2 > 0.0)) return 0.69314718055994531;
  const double nrm = sqrt(n2);
  const V3 d{Dl.x / nrm, Dl.y / nrm, Dl.z / nrm};
  const double s = beta * nrm, z = dot3(sig, d);
  return -((s * (z - 1.0) + log(s)) - log(-expm1(-2.0 * s)));
}

// ---- the plan-independent reduction ---------------------------------------------------------------------------------
// The unit of a per-chain sum is a GROUP of 256 consecutive items, summed by the 256 threads of a workgroup in block_sum's
// fixed order; group g of chain b leaves partial[(b * ngroups + g) * NV + c].  chain_sum adds the groups of a chain: thread t
// takes groups t, t + 256, ... in ascending order, then block_sum.  Neither depends on how many groups a workgroup takes, on
// the grid or on the batch, so a per-chain sum is the same bits under every launch plan.
constexpr uint32_t kGroup = 256;

template <int NV>
__device__ __forceinline__ void chain_sum(const double *__restrict__ partial, uint32_t ngroups, double (&v)[NV], double *red) {
  for (int c = 0; c < NV; ++c) v[c] = 0.0;
  for (uint32_t g = threadIdx.x; g < ngroups; g += kGroup)
    for (int c = 0; c < NV; ++c) v[c] += partial[(size_t)g * NV + c];
  block_sum<NV>(v, red);
}

int check_sigma_level(const mlmcpi_sigma_level *level);  // sigma_levels.hip

}  // namespace mlmcpi
