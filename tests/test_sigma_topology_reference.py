"""tests/sigma_topology_reference.py, the longdouble restatement of the geometric topological charge of the O(3) sigma model, pinned on
the CPU: its vertex order is tests/sigma_level_model.py's, Q is an integer, the discretised instantons carry Q = +-k on both layouts,
the symmetries of the charge hold, and every input the GPU comparisons use is clear of the cut of atan2."""
import numpy as np
import pytest

import sigma_level_model as slm
import sigma_topology_reference as ref

SHAPES = [(2, 2), (2, 6), (4, 4), (6, 4), (16, 16)]
LAYOUTS = [False, True]


def _integral(c, eps=ref.EPS_LONGDOUBLE):
    """every chain's Q within its bound of an integer; returns the integers"""
    k = np.rint(c.Q)
    assert np.all(np.abs(c.Q - k) <= c.error_bound(eps)), (np.abs(c.Q - k).max(), c.error_bound(eps).max())
    return k.astype(np.int64)


@pytest.mark.parametrize("Mt,Mx", SHAPES + [(66, 34)])
@pytest.mark.parametrize("rot", LAYOUTS)
def test_vertex_order_is_the_level_models(Mt, Mx, rot):
    L = slm.Level(Mt, Mx, rot)
    i, j = np.meshgrid(np.arange(-2, Mt + 2), np.arange(-2, Mx + 2), indexing="ij")
    if rot:
        keep = (i + j) % 2 == 0
        i, j = i[keep], j[keep]
    got = ref.vertex_index(Mt, Mx, rot, i.ravel(), j.ravel())
    want = [L.cart2lin(int(a), int(b)) for a, b in zip(i.ravel(), j.ravel())]
    assert got.tolist() == want
    f = ref.faces(Mt, Mx, rot)
    assert f.shape == (L.n, 4) and f.min() == 0 and f.max() == L.n - 1    # n faces for n vertices


@pytest.mark.parametrize("Mt,Mx", SHAPES)
@pytest.mark.parametrize("rot", LAYOUTS)
def test_random_spins_give_integers(Mt, Mx, rot):
    phi = ref.uniform_spins(Mt, Mx, rot, 200, seed=11 + Mt + 3 * Mx)
    c = ref.charge(Mt, Mx, rot, phi)
    k = _integral(c)
    print(f"({Mt}, {Mx}, rotated={rot}): |Q - round Q| <= {float(np.abs(c.Q - k).max()):.2e}, charges {k.min()} .. {k.max()}")
    assert np.abs(c.Q - k).max() < 2e-14                  # what float64 arithmetic was seen to give; longdouble does better
    if (Mt, Mx, rot) == (2, 2, True):
        assert np.all(k == 0)                             # W = E: both triangles are degenerate
    elif Mt * Mx >= 16:
        assert k.min() < 0 < k.max()                      # uniform spins wind both ways


@pytest.mark.parametrize("Mt,Mx,lam,k", ref.INSTANTONS)
@pytest.mark.parametrize("rot", LAYOUTS)
def test_instantons(Mt, Mx, lam, k, rot):
    for anti, want in ((False, k), (True, -k)):
        c = ref.charge(Mt, Mx, rot, ref.instanton(Mt, Mx, rot, lam, k, anti))
        assert _integral(c).tolist() == [want], (c.Q, want)
        assert c.margin[0] >= ref.MIN_MARGIN               # the GPU test runs these too


@pytest.mark.parametrize("Mt,Mx,lam,k", ref.INSTANTONS)
@pytest.mark.parametrize("rot", LAYOUTS)
def test_transposed_instantons(Mt, Mx, lam, k, rot):
    """i <-> j reverses the orientation of the lattice: the transposed instanton carries -k on both layouts"""
    L = slm.Level(Mt, Mx, rot)
    a = ref.instanton(Mt, Mx, rot, lam, k).reshape(1, L.n, 2)
    src = np.array([L.cart2lin(j, i) for i, j in L.coords])       # Mt = Mx
    assert _integral(ref.charge(Mt, Mx, rot, a[:, src].reshape(1, -1))).tolist() == [-k]


@pytest.mark.parametrize("rot", LAYOUTS)
def test_trivial_cases(rot):
    for Mt, Mx in SHAPES:
        n = Mt * Mx // 2 if rot else Mt * Mx
        assert ref.charge(Mt, Mx, rot, np.zeros((1, 2 * n))).Q[0] == 0                      # the cold state
        tilted = np.tile([0.7, -2.1], n)[None]
        assert ref.charge(Mt, Mx, rot, tilted).Q[0] == 0                                     # any constant state
    assert np.all(_integral(ref.charge(2, 2, True, ref.uniform_spins(2, 2, True, 50, seed=3))) == 0)


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q      # proper: det +1 (3 x 3: -q flips the sign of the determinant)


@pytest.mark.parametrize("Mt,Mx", [(4, 4), (6, 4), (16, 16)])
@pytest.mark.parametrize("rot", LAYOUTS)
def test_symmetries(Mt, Mx, rot):
    L = slm.Level(Mt, Mx, rot)
    B = 40
    phi = ref.uniform_spins(Mt, Mx, rot, B, seed=101 + Mt)
    base = ref.charge(Mt, Mx, rot, phi)
    keep = base.margin > 1e-4                      # a transformed copy is recomputed in float64: stay clear of the cut
    assert keep.sum() > B // 2
    k0 = _integral(base)
    a = phi.reshape(B, L.n, 2)

    def rounded(x, Mt_=Mt, Mx_=Mx):
        return _integral(ref.charge(Mt_, Mx_, rot, x.reshape(B, -1)))[keep]

    shifted = a.copy()                             # phi -> phi + c: a rotation about the z axis
    shifted[..., 1] += 0.83
    assert np.array_equal(rounded(shifted), k0[keep])
    R = _rotation(np.random.default_rng(5))        # a full O(3) rotation of det +1, on the host
    sig = np.asarray(ref.spins(phi, L.n), dtype=np.float64) @ R.T
    assert np.array_equal(rounded(ref.angles_of(sig)), k0[keep])
    mirrored = a.copy()                            # theta -> pi - theta: the reflection z -> -z flips the charge
    mirrored[..., 0] = np.pi - mirrored[..., 0]
    assert np.array_equal(rounded(mirrored), -k0[keep])
    # the transposed field psi(i, j) = phi(j, i) on the (Mx, Mt) level: an orientation-reversing map of the lattice.  A plain face
    # goes to a face cut along the same diagonal, so every state flips; a rotated face (W, S, E, N) goes to (S, W, N, E), cut along
    # the other diagonal, which a rough state may wind differently: there the smooth states below flip (test_transposed_instantons)
    if not rot:
        Lt = slm.Level(Mx, Mt, rot)
        src = np.array([L.cart2lin(j, i) for i, j in Lt.coords])
        assert np.array_equal(rounded(a[:, src], Mx, Mt), -k0[keep])
    # lattice translations (on a rotated level: those of the level, di + dj even)
    for di, dj in ((2, 0), (0, 2), (1, 1), (1, -1)) + (() if rot else ((1, 0), (0, 1))):
        src = np.array([L.cart2lin(i + di, j + dj) for i, j in L.coords])
        assert np.array_equal(rounded(a[:, src]), k0[keep])


@pytest.mark.parametrize("key", ref.gpu_cases(), ids=lambda k: "%dx%d-%s-%d" % (k[0], k[1], "rot" if k[2] else "plain", k[3]))
def test_gpu_inputs_are_clear_of_the_cut(key):
    """the condition of every GPU comparison of Q, asserted on the reference alone"""
    phi, c = ref.gpu_case(*key)
    print(f"{key}: seed {ref.SEEDS[key]}, margin {c.margin.min():.3e}, largest bound {c.error_bound().max():.3e}")
    assert c.margin.min() >= ref.MIN_MARGIN
    _integral(c)
