// sigma_topology_device.hpp -- the face code of the geometric topological charge of the O(3) sigma model, shared by the charge of a
// state of angles (sigma_topology.hip) and the charge of a smoothed field of unit vectors (sigma_field.hip): the tile and its plan,
// the staging geometry, the faces of a staged tile and their sum order.  The two units differ in one thing only:
// where a staged vertex comes from (`fetch`).  Includes sigma_level_device.hpp, so the including file is compiled without fp
// contraction.
#pragma once
#include "sigma_level_device.hpp"

namespace mlmcpi {

constexpr uint32_t kTopoThreads = kGroup;                 // 256: chain_sum's workgroup
constexpr uint32_t kTopoTile = 32;                        // cells along a side of a tile
constexpr uint32_t kTopoLd = kTopoTile + 1;               // staged entries along a side, and the row stride in LDS (doubles)
constexpr uint32_t kTopoPlane = kTopoLd * kTopoLd;        // doubles of one component of one staged plane
constexpr uint32_t kTopoGridX = (1u << 31) / kTopoThreads;  // workgroups along x of a launch; beyond, the grid grows along y
constexpr uint64_t kTopoMaxBlocks = (uint64_t)kTopoGridX * 65535;

struct TopoPlan {
  uint32_t W, H;            // a vertex plane: W columns (the contiguous index), H rows
  uint32_t tiles_a, tiles;  // tiles along W; tiles of a chain
  uint32_t nvert;           // n
};

inline TopoPlan topo_plan(const SigmaLevel &L) {
  TopoPlan G;
  G.W = L.rot ? L.ht : L.Mt;
  G.H = L.rot ? L.hx : L.Mx;
  G.tiles_a = (G.W + kTopoTile - 1) / kTopoTile;
  G.tiles = G.tiles_a * ((G.H + kTopoTile - 1) / kTopoTile);
  G.nvert = L.nvert();
  return G;
}

// workgroups ride one linear index over grid x and, past kTopoGridX, y
inline dim3 topo_grid(uint64_t blocks) {
  const uint32_t gx = blocks < kTopoGridX ? (uint32_t)blocks : kTopoGridX;
  return dim3(gx, (uint32_t)((blocks + gx - 1) / gx));
}

__device__ __forceinline__ uint64_t topo_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__device__ __forceinline__ V3 topo_load(const double *s, uint32_t c) { return V3{s[c], s[kTopoPlane + c], s[2 * kTopoPlane + c]}; }

__device__ __forceinline__ double topo_triple(const V3 &a, const V3 &b, const V3 &c) {
  return dot3(a, V3{b.y * c.z - b.z * c.y, b.z * c.x - b.x * c.z, b.x * c.y - b.y * c.x});
}

// half the signed area of the face (c1, c2, c3, c4): atan2 of the triangle (c1, c2, c3) plus atan2 of (c1, c3, c4)
__device__ __forceinline__ double topo_face(const V3 &c1, const V3 &c2, const V3 &c3, const V3 &c4) {
  const double d13 = dot3(c1, c3);
  const double x1 = ((1.0 + dot3(c1, c2)) + dot3(c2, c3)) + d13, y1 = topo_triple(c1, c2, c3);
  const double x2 = ((1.0 + d13) + dot3(c3, c4)) + dot3(c4, c1), y2 = topo_triple(c1, c3, c4);
  return atan2(y1, x1) + atan2(y2, x2);
}

// the tile of workgroup-in-chain `tile`: origin (a0, b0) in the plane and extents (tw, th), clipped at the plane's upper edges
struct TopoTile {
  uint32_t a0, b0, tw, th;
};

__device__ __forceinline__ TopoTile topo_tile(const TopoPlan &G, uint32_t tile) {
  TopoTile T;
  T.a0 = (tile % G.tiles_a) * kTopoTile;
  T.b0 = (tile / G.tiles_a) * kTopoTile;
  T.tw = G.W - T.a0 < kTopoTile ? G.W - T.a0 : kTopoTile;
  T.th = G.H - T.b0 < kTopoTile ? G.H - T.b0 : kTopoTile;
  return T;
}

// Staging: the tile and the one-vertex halo its faces reach, (tw + 1) x (th + 1) entries per vertex plane, into sig
// [NP][3][kTopoPlane]; fetch(l) is the unit vector of the level's vertex l.  The caller puts the barrier behind it.
template <int ROT, class Fetch>
__device__ __forceinline__ void topo_stage(const TopoPlan &G, const TopoTile &T, double *sig, Fetch fetch) {
  constexpr uint32_t NP = ROT ? 2 : 1;
  const uint32_t sw = T.tw + 1, ns = sw * (T.th + 1);
  for (uint32_t c = threadIdx.x; c < NP * ns; c += kTopoThreads) {
    const uint32_t p = c / ns, r = c - p * ns, la = r % sw, lb = r / sw;
    // plain and E: entry (a0 + la, b0 + lb); O: (a0 - 1 + la, b0 - 1 + lb); a0 + la <= W, so one subtraction wraps either
    uint32_t a = T.a0 + la + (p ? G.W - 1 : 0), bb = T.b0 + lb + (p ? G.H - 1 : 0);
    if (a >= G.W) a -= G.W;
    if (bb >= G.H) bb -= G.H;
    const V3 v = fetch((size_t)p * G.W * G.H + (size_t)bb * G.W + a);
    double *d = sig + p * 3 * kTopoPlane + lb * kTopoLd + la;
    d[0] = v.x;
    d[kTopoPlane] = v.y;
    d[2 * kTopoPlane] = v.z;
  }
}

// this thread's share of the staged tile's faces: the cells t, t + 256, .. in ascending order (cell = tw cb + ca), on a rotated
// level the face of site (2a+1, 2b) before that of (2a, 2b+1)
// NOTE: sigma_topo_tile_kernel (sigma_topology.hip) carries this loop written out, because its instructions are pinned; an edit
// here goes there as well, and the other way round.
template <int ROT>
__device__ __forceinline__ double topo_faces(const TopoTile &T, const double *sig) {
  double acc = 0.0;
  for (uint32_t t = threadIdx.x; t < T.tw * T.th; t += kTopoThreads) {
    const uint32_t c = (t / T.tw) * kTopoLd + t % T.tw;
    if constexpr (ROT) {
      const double *E = sig, *O = sig + 3 * kTopoPlane;
      const V3 e00 = topo_load(E, c), e10 = topo_load(E, c + 1), e01 = topo_load(E, c + kTopoLd);
      const V3 o10 = topo_load(O, c + 1), o01 = topo_load(O, c + kTopoLd), o11 = topo_load(O, c + kTopoLd + 1);
      acc += topo_face(e00, o10, e10, o11);  // site (2a+1, 2b)
      acc += topo_face(o01, e00, o11, e01);  // site (2a, 2b+1)
    } else {
      acc += topo_face(topo_load(sig, c), topo_load(sig, c + 1), topo_load(sig, c + kTopoLd + 1), topo_load(sig, c + kTopoLd));
    }
  }
  return acc;
}

}  // namespace mlmcpi
