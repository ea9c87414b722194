// index_maps.hip -- host-side index maps of the lattices (lattice/lattice2d.hh:230-268,348-375; lattice/lattice1d.cc:11-18;
// lattice/lattice2d.cc:137-155).  Host code only.
#include "internal.hpp"

using namespace mlmcpi;

extern "C" {

uint32_t mlmcpi_vertex_cart2lin(uint32_t Mt, uint32_t Mx, int rotated, int i, int j) {
  const int mt = (int)Mt, mx = (int)Mx;
  if (rotated) {
    const int half_t = mt / 2, half_x = mx / 2;
    const int ii = ((i + mt) - (i & 1)) / 2, jj = ((j + mx) - (j & 1)) / 2;
    return (uint32_t)(half_t * (jj % half_x) + ii % half_t + (mt * mx / 4) * (i & 1));
  }
  return (uint32_t)(mt * ((j + mx) % mx) + (i + mt) % mt);
}

void mlmcpi_vertex_lin2cart(uint32_t Mt, uint32_t Mx, int rotated, uint32_t ell, int *i, int *j) {
  const int mt = (int)Mt, mx = (int)Mx;
  if (rotated) {
    const int quarter = mt * mx / 4, half_t = mt / 2;
    const int parity = (int)ell / quarter;
    const int rest = (int)ell - quarter * parity;
    const int jh = rest / half_t;
    *j = 2 * jh + parity;
    *i = 2 * (rest - half_t * jh) + parity;
  } else {
    *j = (int)(ell / Mt);
    *i = (int)(ell - Mt * (uint32_t)*j);
  }
}

uint32_t mlmcpi_link_cart2lin(uint32_t Mt, uint32_t Mx, int i, int j, int mu) {
  const int mt = (int)Mt, mx = (int)Mx;
  return (uint32_t)(2 * mt * ((j + mx) % mx) + 2 * ((i + mt) % mt) + mu);
}

void mlmcpi_link_lin2cart(uint32_t Mt, uint32_t Mx, uint32_t ell, int *i, int *j, int *mu) {
  (void)Mx;
  const uint32_t row = ell / (2 * Mt), rest = ell - 2 * Mt * row;
  *j = (int)row;
  *i = (int)(rest >> 1);
  *mu = (int)(rest & 1u);
}

int mlmcpi_neighbours_1d(uint32_t M, uint32_t *out) {
  MLMCPI_REQUIRE(out && M > 0, "bad arguments");
  for (uint32_t ell = 0; ell < M; ++ell) {
    out[2 * ell] = (ell + M - 1) % M;
    out[2 * ell + 1] = (ell + 1) % M;
  }
  return MLMCPI_OK;
}

int mlmcpi_neighbours_2d(uint32_t Mt, uint32_t Mx, int rotated, uint32_t *out) {
  MLMCPI_REQUIRE(out && Mt > 0 && Mx > 0, "bad arguments");
  MLMCPI_REQUIRE(!rotated || (Mt % 2 == 0 && Mx % 2 == 0), "rotated lattices need even Mt, Mx");
  // nearest neighbours first, then diagonals (next-nearest on the rotated lattice)
  static const int step_plain[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
  static const int step_rot[8][2] = {{1, 1}, {1, -1}, {-1, 1}, {-1, -1}, {2, 0}, {-2, 0}, {0, 2}, {0, -2}};
  const uint32_t nv = rotated ? Mt * Mx / 2 : Mt * Mx;
  for (uint32_t ell = 0; ell < nv; ++ell) {
    int i, j;
    mlmcpi_vertex_lin2cart(Mt, Mx, rotated, ell, &i, &j);
    for (int k = 0; k < 8; ++k) {
      const int *s = rotated ? step_rot[k] : step_plain[k];
      out[8 * ell + k] = mlmcpi_vertex_cart2lin(Mt, Mx, rotated, i + s[0], j + s[1]);
    }
  }
  return MLMCPI_OK;
}

}  // extern "C"
