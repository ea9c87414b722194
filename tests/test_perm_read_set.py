"""The plane of plaquettes of the closed-form Schwinger sweeps, packed to its read set (sweep_geometry.hpp `PermGeom`,
schwinger_perm.hpp `PermPlane`): the streams of every link are enumerated here from the two sums of the header comment of
schwinger_perm.hpp (quenchedschwingeraction.cc:25-65 is what they sum up), and the constants of `PermGeom` -- taken from
a tiny host program compiled from sweep_geometry.hpp, not restated -- must be exactly their extents per parity, place
every plaquette of the read set at an offset of its own inside the plane, and turn every stream into K equal steps of
kStep.  A plaquette outside the extents would be a read of LDS nobody wrote; two at one offset a silent wrong answer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CONFIGS = [(512, 2, 64), (1024, 2, 64), (512, 0, 64), (512, 0, 32)]   # the instantiations of the kernels
KMAX = 10

PROGRAM = r"""
#include <cstdio>
#include "sweep_geometry.hpp"
using namespace mlmcpi;
template <int NT, int RING, int TH>
static void dump() {
  using PG = PermGeom<NT, RING, TH>;
  static_assert(kPermMaxK == %d, "the depths the test covers");
  for (uint32_t K = 1; K <= kPermMaxK; ++K) {
    std::printf("geom %%d %%d %%d %%u %%d %%d %%d %%d %%u %%zu %%u %%u", NT, RING, TH, K, PG::OW, PG::OH, PG::kPitch, PG::kQRows, PG::kStep,
                PG::plane_bytes, PG::width(K), PG::rows(K));
    for (uint32_t par = 0; par < 2; ++par)
      std::printf(" %%u %%u %%u %%u", PG::col_first(K, par), PG::col_last(K, par), PG::row_first(K, par), PG::row_last(K, par));
    std::printf("\noffsets");
    for (uint32_t rp = 0; rp < 2; ++rp)
      for (uint32_t cp = 0; cp < 2; ++cp)
        for (uint32_t R = PG::row_first(K, rp); R <= PG::row_last(K, rp); R += 2)
          for (uint32_t C = PG::col_first(K, cp); C <= PG::col_last(K, cp); C += 2) std::printf(" %%u", PG::offset(K, C, R));
    std::printf("\n");
  }
}
int main() {
  %s
  return 0;
}
""" % (KMAX, "\n  ".join("dump<%d, %d, %d>();" % c for c in CONFIGS))


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """{(NT, RING, TH, K): (constants, {(C, R): offset})} as PermGeom has them"""
    d = tmp_path_factory.mktemp("perm_read_set")
    src, exe = d / "perm_geom.cc", d / "perm_geom"
    src.write_text(PROGRAM)
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    out = {}
    for g, o in zip(lines[0::2], lines[1::2]):
        g, o = g.split(), o.split()
        assert g[0] == "geom" and o[0] == "offsets"
        v = [int(x) for x in g[1:]]
        NT, RING, TH, K = v[:4]
        c = dict(zip(("OW", "OH", "pitch", "qrows", "step", "plane_bytes", "width", "rows"), v[4:12]))
        c["col"] = {0: (v[12], v[13]), 1: (v[16], v[17])}
        c["row"] = {0: (v[14], v[15]), 1: (v[18], v[19])}
        cells = [(C, R) for rp in (0, 1) for cp in (0, 1) for R in range(c["row"][rp][0], c["row"][rp][1] + 1, 2)
                 for C in range(c["col"][cp][0], c["col"][cp][1] + 1, 2)]
        offs = [int(x) for x in o[1:]]
        assert len(cells) == len(offs)
        out[(NT, RING, TH, K)] = (c, dict(zip(cells, offs)))
    assert set(out) == {c + (K,) for c in CONFIGS for K in range(1, KMAX + 1)}
    return out


def streams(OW, OH, K):
    """The streams of every link of the OW x OH output window, in plane coordinates (output (c, r) = plane (c + 2 K, r + 2 K)):
    lists of K plaquettes (C, R) in the order s = 0, 1, ...; e_x = +1 for even x, -1 for odd x, p_x = x mod 2."""
    e = lambda x: 1 if x % 2 == 0 else -1
    for r in range(OH):
        for c in range(OW):
            i, j = c + 2 * K, r + 2 * K
            pi, pj = i % 2, j % 2
            yield [(i + 2 * s * e(i), j - 1 - pj - 2 * s) for s in range(K)]            # theta_0(i, j): + ...
            yield [(i + 2 * s * e(i), j + pj + 2 * s) for s in range(K)]                # ... - ...
            yield [(i + pi + 2 * s, j + 2 * (s + 1) * e(j)) for s in range(K)]          # theta_1(i, j): + ...
            yield [(i - 1 - pi - 2 * s, j + 2 * (s + 1) * e(j)) for s in range(K)]      # ... - ...


@pytest.mark.parametrize("NT,RING,TH", CONFIGS)
def test_extents_are_the_read_set_and_streams_are_equal_steps(geometry, NT, RING, TH):
    for K in range(1, KMAX + 1):
        c, off = geometry[(NT, RING, TH, K)]
        assert (c["OW"], c["OH"]) == (64 + 2 * RING, TH + 2 * RING)
        cols = {0: set(), 1: set()}
        rows = {0: set(), 1: set()}
        n = 0
        for st in streams(c["OW"], c["OH"], K):
            assert len(st) == K
            o = [off[p] for p in st]                      # (KeyError: a read outside the extents)
            assert all(b - a == c["step"] for a, b in zip(o, o[1:])), (K, st)
            assert len({(C % 2, R % 2) for C, R in st}) == 1
            for C, R in st:
                cols[C % 2].add(C)
                rows[R % 2].add(R)
            n += 1
        assert n == 4 * c["OW"] * c["OH"]
        for par in (0, 1):
            assert (min(cols[par]), max(cols[par])) == c["col"][par], (K, par)
            assert (min(rows[par]), max(rows[par])) == c["row"][par], (K, par)
            # every index of the parity in between is read too: the extents hold nothing but the read set's columns and rows
            assert cols[par] == set(range(c["col"][par][0], c["col"][par][1] + 1, 2))
            assert rows[par] == set(range(c["row"][par][0], c["row"][par][1] + 1, 2))
        # what a build has to cover lies inside what it loads: plaquette (C, R) needs theta columns C, C + 1 and rows R, R + 1
        assert max(c["col"][0][1], c["col"][1][1]) + 1 <= c["width"] and max(c["row"][0][1], c["row"][1][1]) + 1 <= c["rows"]


@pytest.mark.parametrize("NT,RING,TH", CONFIGS)
def test_packed_offsets_are_injective_and_inside_the_plane(geometry, NT, RING, TH):
    for K in range(1, KMAX + 1):
        c, off = geometry[(NT, RING, TH, K)]
        assert len(set(off.values())) == len(off)
        assert min(off.values()) >= 0 and 8 * (max(off.values()) + 1) <= c["plane_bytes"]
        assert c["step"] == c["pitch"] + 1 and c["plane_bytes"] == 4 * c["qrows"] * c["pitch"] * 8
        # a quadrant per (column parity, row parity), rows of one pitch: at most a pitch's padding per quadrant
        for (C, R), o in off.items():
            q, rest = divmod(o, c["qrows"] * c["pitch"])
            assert q == 2 * (R % 2) + C % 2
        held = {par: (c["col"][par][1] - c["col"][par][0]) // 2 + 1 for par in (0, 1)}
        held_r = {par: (c["row"][par][1] - c["row"][par][0]) // 2 + 1 for par in (0, 1)}
        assert held == {0: c["OW"] // 2 + K, 1: c["OW"] // 2 + K} and held_r == {0: c["OH"] // 2 + K, 1: c["OH"] // 2 + K - 1}
        if K == KMAX:   # the deepest launch fills the pitch and all rows but the one of padding
            assert held[0] == c["pitch"] and held_r[0] == c["qrows"] and held_r[1] == c["qrows"] - 1
        # the plane lies in LDS the launch owns anyway: under the image of the fused launch, within 80 KiB of the plain one
        assert c["plane_bytes"] <= (2 * 68 * 68 * 8 if RING == 2 else 80 * 1024)
