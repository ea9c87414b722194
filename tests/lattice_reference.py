"""Plain extended-precision restatement of the 2-D Schwinger and GFF formulas, for the tests only.

numpy in np.longdouble (x87 80-bit: 64-bit mantissa, eps = 2^-63 = 1.08e-19), vectorised with np.roll and written from
the formulas, not from any kernel's order of operations.  It is the "truth" that tests/test_lattice_bands_gpu.py holds
the HIP kernels to at tolerances derived from fp64 rounding alone, which the fp64 oracle (itself a rounded computation
in another order) cannot serve as; tests/test_lattice_reference.py pins it to the oracle and to the reference author's
own Python on the CPU.

Storage (lattice/lattice2d.hh): vertex (i, j) -> j * Mt + i with i the temporal (fastest) index; a Schwinger state
holds two links per vertex, [(j * Mt + i), mu].  Every function takes one state ([n]) or a batch ([B, n]) and returns
long doubles; arrays come back in storage order.

  Schwinger   P(i,j) = t(i,j,0) + t(i+1,j,1) - t(i,j+1,0) - t(i,j,1)           quenchedschwingeraction.cc:14-17
              S = beta sum (1 - cos P)                                           quenchedschwingeraction.cc:7-22
              dS/dt(i,j,0) = beta (sin P(i,j) - sin P(i,j-1))                    quenchedschwingeraction.cc:68-89
              dS/dt(i,j,1) = beta (sin P(i-1,j) - sin P(i,j))
              <cos P>;  Q^2 / (4 pi^2),  Q = sum mod_2pi(P)                      qoiavgplaquette.cc, qoi2dsusceptibility.cc
  GFF         S = 1/2 sum phi (kappa phi - four neighbours),  kappa = 4 + mu2    gffaction.cc:15-23
              dS/dphi = kappa phi - four neighbours                              gffaction.cc:80-94
"""
import numpy as np

LD = np.longdouble
# the derived tolerances of the GPU tests assume a reference at least 2^10 times finer than fp64: no skip, no fall-back
assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble is not extended precision here (eps = {np.finfo(LD).eps})"

# pi to 40 digits, parsed in long double (np.pi is the fp64 value, 1.2e-16 away)
PI = LD("3.141592653589793238462643383279502884197")
TWO_PI = 2 * PI


def _links(theta, Mt, Mx):
    """[..., 2 Mt Mx] -> (t0, t1), each [..., Mx, Mt] (axis -2 = j, axis -1 = i), long double"""
    t = np.asarray(theta, dtype=LD)
    assert t.shape[-1] == 2 * Mt * Mx, (t.shape, Mt, Mx)
    t = t.reshape(t.shape[:-1] + (Mx, Mt, 2))
    return t[..., 0], t[..., 1]


def schwinger_plaquettes(theta, Mt, Mx):
    """P(i,j), unwrapped, [..., Mx * Mt] in vertex order"""
    t0, t1 = _links(theta, Mt, Mx)
    # np.roll(a, -1, axis)[k] = a[k + 1]
    P = t0 + np.roll(t1, -1, axis=-1) - np.roll(t0, -1, axis=-2) - t1
    return P.reshape(P.shape[:-2] + (Mx * Mt,))


def schwinger_action(theta, Mt, Mx, beta):
    P = schwinger_plaquettes(theta, Mt, Mx)
    return LD(beta) * np.sum(1 - np.cos(P), axis=-1)


def schwinger_force(theta, Mt, Mx, beta, plaquettes=None):
    """dS/dtheta in storage order, [..., 2 Mt Mx]; `plaquettes` (unwrapped or wrapped, vertex order) replaces the
    plaquettes computed from theta (to rebuild the force from another source of plaquettes)."""
    P = schwinger_plaquettes(theta, Mt, Mx) if plaquettes is None else np.asarray(plaquettes, dtype=LD)
    s = np.sin(P.reshape(P.shape[:-1] + (Mx, Mt)))
    f0 = LD(beta) * (s - np.roll(s, 1, axis=-2))    # sin P(i,j) - sin P(i,j-1)
    f1 = LD(beta) * (np.roll(s, 1, axis=-1) - s)    # sin P(i-1,j) - sin P(i,j)
    f = np.stack([f0, f1], axis=-1)
    return f.reshape(f.shape[:-3] + (2 * Mt * Mx,))


def schwinger_avg_plaquette(theta, Mt, Mx):
    return np.sum(np.cos(schwinger_plaquettes(theta, Mt, Mx)), axis=-1) / LD(Mt * Mx)


def mod_2pi(x):
    """x - 2 pi round(x / 2 pi): the representative in [-pi, pi] (which end a value at +-pi takes is rounding; callers
    that care keep away from it, see distance_to_branch_cut)"""
    x = np.asarray(x, dtype=LD)
    return x - TWO_PI * np.rint(x / TWO_PI)


def distance_to_branch_cut(theta, Mt, Mx):
    """min over plaquettes of | |mod_2pi(P)| - pi |: how far the field is from a plaquette whose wrap depends on rounding"""
    w = np.abs(mod_2pi(schwinger_plaquettes(theta, Mt, Mx)))
    return np.min(np.abs(w - PI), axis=-1)


def schwinger_charge(theta, Mt, Mx):
    """Q = sum mod_2pi(P) / 2 pi (an integer up to rounding on a periodic lattice)"""
    return np.sum(mod_2pi(schwinger_plaquettes(theta, Mt, Mx)), axis=-1) / TWO_PI


def schwinger_susceptibility(theta, Mt, Mx):
    Q = schwinger_charge(theta, Mt, Mx)
    return Q * Q


def _field(phi, Mt, Mx):
    p = np.asarray(phi, dtype=LD)
    assert p.shape[-1] == Mt * Mx, (p.shape, Mt, Mx)
    return p.reshape(p.shape[:-1] + (Mx, Mt))


def gff_force(phi, Mt, Mx, mu2):
    p = _field(phi, Mt, Mx)
    f = (4 + LD(mu2)) * p - np.roll(p, 1, -1) - np.roll(p, -1, -1) - np.roll(p, 1, -2) - np.roll(p, -1, -2)
    return f.reshape(f.shape[:-2] + (Mt * Mx,))


def gff_action(phi, Mt, Mx, mu2):
    p = np.asarray(phi, dtype=LD)
    return np.sum(p * gff_force(phi, Mt, Mx, mu2), axis=-1) / 2


def phi_squared(phi):
    p = np.asarray(phi, dtype=LD)
    return np.sum(p * p, axis=-1) / LD(p.shape[-1])


def kinetic_energy(p):
    p = np.asarray(p, dtype=LD)
    return np.sum(p * p, axis=-1) / 2
