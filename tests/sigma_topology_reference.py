"""numpy longdouble restatement of the geometric (Berg-Luescher) topological charge of the O(3) sigma model on a level of its
CoarsenRotate hierarchy (mlmcpathintegral_amd/csrc/sigma_topology.hip; include/mlmcpi_hip.h:
mlmcpi_sigma_level_topological_charge), from the (theta, phi) state in the library's vertex order.

    sigma = (sin theta cos phi, sin theta sin phi, cos theta)
    x = 1 + a.b + b.c + c.a,  y = a.(b x c),  A(a, b, c) = 2 atan2(y, x)
    plain level    one face per vertex (i, j): s1 = (i, j), s2 = (i+1, j), s3 = (i+1, j+1), s4 = (i, j+1);
                   triangles (s1, s2, s3), (s1, s3, s4)
    rotated level  one face per site (i, j), i + j odd: W = (i-1, j), S = (i, j-1), E = (i+1, j), N = (i, j+1);
                   triangles (W, S, E), (W, E, N)
    Q = (1 / 4 pi) sum over faces (A_1 + A_2),  chi = Q^2 / n

The vertex order is that of tests/sigma_level_model.py: `vertex_index` is Level.cart2lin written for arrays (a level of 2^20
vertices is indexed in a blink), and tests/test_sigma_topology_reference.py pins it to Level.cart2lin vertex by vertex.

Besides Q a chain gets its MARGIN, min over triangles of m, m = |y| where x < 0, else hypot(x, y): the distance of (x, y) from the
cut of atan2, across which the charge jumps by one; and its WEIGHT = sum over triangles (1 + 1 / m) / (2 pi), so that

    |Q_computed - Q| <= C eps weight                                                      (error_bound)

for arithmetic of unit roundoff eps.  Where C = 256 comes from, in units of eps, per triangle:
  * a component of sigma is a product of two of sin, cos (each within 2 ulp = 4 eps of the device's libm, the product rounded: 9 eps
    relative; the z component 4 eps).  A product of two components carries 2 x 9 + 1 = 19 eps, a dot product of unit vectors sums three
    of them with sum |terms| <= 1 and two additions: <= 21 eps.  x is 1 plus three dots, three more additions of partial sums <= 4:
    dx <= 3 x 21 + 3 x 4 = 75 eps.
  * y is six triple products a_i b_j c_k, each 3 x 9 + 2 = 29 eps relative, the sum of their moduli <= sqrt 3; the subtractions and
    additions of the cross and dot product add 3 more roundings of partial sums <= sqrt 3: dy <= sqrt 3 x 32 = 56 eps.
  * d atan2 = (x dy - y dx) / (x^2 + y^2), so |dA| <= 2 hypot(dx, dy) / r <= 188 eps / r, r = hypot(x, y) >= m; in units of Q
    (A / 4 pi): 94 eps / (2 pi m).
  * atan2 itself within 2 ulp of a value <= pi: |dA| <= 2 x 4 eps x pi, in units of Q 2 eps = 13 eps / (2 pi).
  * the sums: a triangle's term |A| / 2 <= pi passes through at most D additions on its way into Q (the face, the lane, the wave
    tree, the waves, the tiles of a chain, the last tree), each rounding a partial sum that this term's share bounds by pi: D eps pi
    / (2 pi) = D pi eps / (2 pi) in units of Q.  D <= 2 + 4 + 6 + 4 + T + 6 + 4 with T = ceil(tiles / 256) <= 4 at 2^20 vertices:
    D <= 30, 95 eps / (2 pi).
  Together (94 / m + 13 + 95) eps / (2 pi) <= 256 eps (1 + 1 / m) / (2 pi) / 1.2.  The same C holds for this file's own longdouble
  arithmetic with its eps (its libm is within an ulp, its sums are pairwise).
"""
import functools

import numpy as np

import sigma_level_model as slm

LD = np.longdouble
EPS_DOUBLE = 2.0 ** -53
EPS_LONGDOUBLE = float(np.finfo(LD).eps) / 2
C_BOUND = 256.0
MIN_MARGIN = 1e-6


def vertex_index(Mt, Mx, rotated, i, j):
    """Level(Mt, Mx, rotated).cart2lin(i, j) for integer arrays i, j (periodic; rotated: i + j even)"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    if not rotated:
        return Mt * (j % Mx) + i % Mt
    p = i % 2
    return p * (Mt * Mx // 4) + (Mt // 2) * (((j - p) // 2) % (Mx // 2)) + ((i - p) // 2) % (Mt // 2)


def faces(Mt, Mx, rotated):
    """[n, 4] level indices of the corners c1 .. c4 of every face; the triangles are (c1, c2, c3) and (c1, c3, c4)"""
    i, j = np.meshgrid(np.arange(Mt), np.arange(Mx), indexing="ij")
    i, j = i.ravel(), j.ravel()
    if rotated:
        odd = (i + j) % 2 == 1
        i, j = i[odd], j[odd]
        corners = [(i - 1, j), (i, j - 1), (i + 1, j), (i, j + 1)]
    else:
        corners = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
    return np.stack([vertex_index(Mt, Mx, rotated, ci, cj) for ci, cj in corners], axis=1)


def spins(phi, n):
    """[B, 2 n] angles -> [B, n, 3] longdouble unit vectors"""
    a = np.asarray(phi).reshape(phi.shape[0], n, 2).astype(LD)
    st = np.sin(a[..., 0])
    return np.stack([st * np.cos(a[..., 1]), st * np.sin(a[..., 1]), np.cos(a[..., 0])], axis=-1)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _triangle(a, b, c):
    x = 1 + _dot(a, b) + _dot(b, c) + _dot(c, a)
    y = _dot(a, np.cross(b, c))
    return x, y


class Charge:
    """per chain: Q (longdouble), chi = Q^2 / n (longdouble), margin and weight (float64)"""

    def __init__(self, Q, n, margin, weight):
        self.Q, self.n, self.margin, self.weight = Q, n, margin, weight
        self.chi = Q * Q / n

    def error_bound(self, eps=EPS_DOUBLE):
        """|Q computed in arithmetic of unit roundoff eps - Q| is within this, per chain"""
        return C_BOUND * eps * self.weight

    def chi_bound(self, eps=EPS_DOUBLE):
        """the same for chi = Q^2 / n: (2 |Q| dQ + dQ^2) / n and two roundings of chi itself"""
        dq = self.error_bound(eps)
        return ((2 * np.abs(self.Q) * dq + dq * dq) / self.n + 2 * eps * self.chi).astype(np.float64)


def charge(Mt, Mx, rotated, phi, chunk=64):
    """the definition, for every chain of phi [B, 2 n]"""
    n = Mt * Mx // 2 if rotated else Mt * Mx
    assert phi.ndim == 2 and phi.shape[1] == 2 * n, (phi.shape, n)
    f = faces(Mt, Mx, rotated)
    B = phi.shape[0]
    Q, margin, weight = np.empty(B, dtype=LD), np.empty(B), np.empty(B)
    two_pi = 2 * np.arctan2(LD(0), LD(-1))
    step = max(1, min(chunk, (1 << 21) // n))   # chains per pass: a few million triangles at a time
    for b0 in range(0, B, step):
        s = spins(phi[b0:b0 + step], n)
        c1, c2, c3, c4 = (s[:, f[:, k]] for k in range(4))
        tot, mrg, wgt = 0, np.inf, 0
        for tri in ((c1, c2, c3), (c1, c3, c4)):
            x, y = _triangle(*tri)
            tot = tot + np.arctan2(y, x).sum(axis=1)
            m = np.where(x < 0, np.abs(y), np.hypot(x, y))
            mrg = np.minimum(mrg, m.min(axis=1))
            wgt = wgt + ((1 + 1 / m) / two_pi).sum(axis=1)
        Q[b0:b0 + step] = tot / two_pi
        margin[b0:b0 + step] = mrg
        weight[b0:b0 + step] = wgt
    return Charge(Q, n, margin, weight)


def level_charge(L, phi):
    return charge(L.Mt, L.Mx, L.rotated, phi)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def uniform_spins(Mt, Mx, rotated, B, seed):
    """B chains of independent spins uniform on the sphere (numpy's generator: independent of the library's Philox streams)"""
    n = Mt * Mx // 2 if rotated else Mt * Mx
    rng = np.random.default_rng(seed)
    out = np.empty((B, 2 * n))
    out[:, 0::2] = np.arccos(1.0 - 2.0 * rng.random((B, n)))
    out[:, 1::2] = -np.pi + 2.0 * np.pi * rng.random((B, n))
    return out


def angles_of(sig):
    """[..., 3] unit vectors -> [..., 2] (theta, phi)"""
    sig = np.asarray(sig, dtype=np.float64)
    return np.stack([np.arctan2(np.hypot(sig[..., 0], sig[..., 1]), sig[..., 2]), np.arctan2(sig[..., 1], sig[..., 0])], axis=-1)


def instanton(Mt, Mx, rotated, lam, k, anti=False):
    """the discretised instanton w = ((i + 1j j - c) / lam)^k (anti: its conjugate), c = (M/2 - 1/2)(1 + 1j) + 0.25 + 0.15j, through
    the stereographic projection sigma = (2 Re w, 2 Im w, 1 - |w|^2) / (1 + |w|^2); one chain [1, 2 n] in the level's vertex order"""
    L = slm.Level(Mt, Mx, rotated)
    c = (Mt / 2 - 0.5) * (1 + 1j) + 0.25 + 0.15j
    z = np.array([i + 1j * j for i, j in L.coords])
    w = ((z - c) / lam) ** k
    if anti:
        w = np.conj(w)
    r2 = np.abs(w) ** 2
    sig = np.stack([2 * w.real, 2 * w.imag, 1 - r2], axis=-1) / (1 + r2)[:, None]
    return angles_of(sig).reshape(1, 2 * L.n)


INSTANTONS = [(16, 16, 3.0, 1), (16, 16, 3.0, 2), (8, 8, 1.5, 1), (4, 4, 1.0, 1)]   # (Mt, Mx, lambda, k)

# ---- the inputs of the GPU comparisons (tests/test_sigma_topology_gpu.py) ---------------------------------------------------------
# Near y = 0, x < 0 the charge legitimately jumps by one, so a comparison of Q needs inputs away from the cut: every input below has
# margin >= MIN_MARGIN, by the choice of its seed (the first of seed0, seed0 + 1, .. whose spins the reference itself finds clear
# of the cut; tests/test_sigma_topology_reference.py asserts the condition for every one).  No case is dropped to meet it.
PARITY_SHAPES = [(2, 2), (2, 6), (4, 4), (6, 4), (66, 34), (130, 70)]
PARITY_CHAINS = [3, 300]
BIG_SHAPE, BIG_CHAINS = (1024, 1024), 2
EDGE_SHAPE, EDGE_CHAINS = (4, 4), 65581
SEEDS = {}   # (Mt, Mx, rotated, B) -> seed; filled below


def _seed0(Mt, Mx, rotated, B):
    return 1000 * Mt + 10 * Mx + (5 if rotated else 0) + 100000 * B


def gpu_cases():
    keys = [(Mt, Mx, rot, B) for Mt, Mx in PARITY_SHAPES for rot in (False, True) for B in PARITY_CHAINS]
    keys += [BIG_SHAPE + (rot, BIG_CHAINS) for rot in (False, True)]
    keys += [EDGE_SHAPE + (rot, EDGE_CHAINS) for rot in (False, True)]
    return keys


@functools.lru_cache(maxsize=None)
def gpu_case(Mt, Mx, rotated, B):
    """(phi [B, 2 n] float64, Charge) of a comparison's input; computed once per session and shared, never written to"""
    phi = uniform_spins(Mt, Mx, rotated, B, SEEDS[(Mt, Mx, rotated, B)])
    phi.setflags(write=False)
    return phi, charge(Mt, Mx, rotated, phi)


# `python tests/sigma_topology_reference.py` prints this table
SEEDS.update({
    (2, 2, False, 3): 302020, (2, 2, False, 300): 30002020, (2, 2, True, 3): 302025, (2, 2, True, 300): 30002025,
    (2, 6, False, 3): 302060, (2, 6, False, 300): 30002060, (2, 6, True, 3): 302065, (2, 6, True, 300): 30002065,
    (4, 4, False, 3): 304040, (4, 4, False, 300): 30004040, (4, 4, True, 3): 304045, (4, 4, True, 300): 30004045,
    (6, 4, False, 3): 306040, (6, 4, False, 300): 30006040, (6, 4, True, 3): 306045, (6, 4, True, 300): 30006045,
    (66, 34, False, 3): 366340, (66, 34, False, 300): 30066345, (66, 34, True, 3): 366345, (66, 34, True, 300): 30066345,
    (130, 70, False, 3): 430700, (130, 70, False, 300): 30130708, (130, 70, True, 3): 430705, (130, 70, True, 300): 30130710,
    (1024, 1024, False, 2): 1234245, (1024, 1024, True, 2): 1234248,
    (4, 4, False, 65581): 6558104040, (4, 4, True, 65581): 6558104046,
})


if __name__ == "__main__":
    for key in gpu_cases():
        seed = _seed0(*key)
        while charge(*key[:3], uniform_spins(*key, seed)).margin.min() < MIN_MARGIN:
            seed += 1
        print(f"    {key}: {seed},", flush=True)
