"""GPU: the 2-D force, the streaming 2-D HMC and the plaquette / energy reductions at the shapes where their index logic
runs: more than one row band and column tile of schwinger_force_band, both stride loops of gff_force_kernel, every
column count NC of schwinger_reduce_band_kernel, the band heights row_blocks() produces over the number of chains B,
both branches of lattice_sum_squares' factoring (the HMC's kinetic energy), and the done flags of repeated HMC trajectories.

Two references.  (i) tests/lattice_reference.py: the formulas in long double (pinned on the CPU by
tests/test_lattice_reference.py), at tolerances DERIVED from fp64 rounding, stated where they are used; the worst
observed error of every case is printed (`pytest -s`, or the captured output of a failing case), so the margin is
visible.  (ii) the oracle (fp64, the reference's order of operations) at the tolerances tests/test_gpu_parity.py uses.

Geometry of the Schwinger force (mlmcpathintegral_amd/csrc/lattice_hmc.hip): a wave walks a band of FORCE_ROWS = 128 rows
and 64 columns of which it owns FORCE_COLS = 62; a failure names (band, row in band, column tile, lane) of the worst
entry.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lattice_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0x1234567812345678
TOL = 1e-12                      # the project's fp64 parity tolerance (tests/test_gpu_parity.py)
FORCE_ROWS, FORCE_COLS = 128, 62
U = 2.0 ** -53                   # unit roundoff of fp64
LD = np.longdouble


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def seq(n):
    return np.sin(np.arange(n) + 1.0)


def assert_close(got, want, tol=TOL, scale=None, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    s = scale if scale is not None else max(1.0, float(np.max(np.abs(want))) if want.size else 1.0)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    assert err <= tol * s, f"{what}: max |diff| = {err:.3e} > {tol:.1e} * {s:.3e}"


def make_lattice(orc, kind, Mt, Mx, **kw):
    from mlmcpathintegral_amd import abi
    if kind == "gff":
        return abi.lattice_action(3, Mt, Mx, mass=kw["mass"]), orc.Action(orc.GFF, Mt=Mt, Mx=Mx, mass=kw["mass"])
    return abi.lattice_action(4, Mt, Mx, beta=kw["beta"]), orc.Action(orc.SCHWINGER, Mt=Mt, Mx=Mx, beta=kw["beta"])


def force_into_nan(gpu_ops, act, xd):
    """mlmcpi_lattice_force into a buffer pre-filled with NaN (ops.lattice_force allocates its own, uninitialised
    output, where an entry that no lane owns could hold anything, the right value of an earlier call included)"""
    from mlmcpathintegral_amd import abi
    f = torch.full_like(xd, float("nan"))
    abi.call("mlmcpi_lattice_force", C.byref(act), gpu_ops._p(xd), gpu_ops._p(f), xd.shape[0], gpu_ops._stream())
    return f


def where_schwinger(l, Mt):
    """flat link index -> the wave geometry of schwinger_force_band that produced it"""
    v, mu = divmod(int(l), 2)
    j, i = divmod(v, Mt)
    return (f"link mu={mu} of vertex (i={i}, j={j}): band {j // FORCE_ROWS}, row {j % FORCE_ROWS} in band, "
            f"column tile {i // FORCE_COLS}, lane {i % FORCE_COLS + 1}")


def check_entries(got, want, bound, tag, where, row_len):
    """every entry of got [B, n] (fp64) against want (long double) at an absolute bound; prints the worst error, and on
    failure names the lattice rows j (row_len entries each) that hold an entry beyond the bound"""
    got = np.asarray(got)
    assert got.shape == want.shape
    bad = ~np.isfinite(got)
    assert not bad.any(), (f"{tag}: {int(bad.sum())} entries were never written (NaN pre-fill), first: chain "
                           f"{np.argwhere(bad)[0][0]}, {where(np.argwhere(bad)[0][1])}")
    err = np.abs(got.astype(LD) - want)
    b, l = np.unravel_index(int(np.argmax(err)), err.shape)
    worst = float(err[b, l])
    print(f"[bands] {tag}: worst |error| vs long double = {worst:.3e} (gate {bound:.3e}, {worst / bound:.3f} of it)")
    if worst > bound:
        beyond = np.argwhere(err > bound)
        rows = sorted({int(k) // row_len for k in beyond[:, 1]})
        raise AssertionError(f"{tag}: |error| = {worst:.3e} > {bound:.3e} in chain {b} at {where(l)}; "
                             f"{len(beyond)} entries beyond the gate, in {len(rows)} rows j = {rows[:12]}{' ...' if len(rows) > 12 else ''}")
    return worst


# ---- 2. Schwinger force across bands and column tiles -------------------------------------------------------------------
# vs long double, per entry.  For |theta| <= pi the fp64 sum of four angles carries at most 3 u * 4 pi = 4.2e-15 (u =
# 2^-53); sin_reduced states an absolute error of ~1e-16; the product by beta and the final difference add 3 u each
# relative to beta: 2 (4.2e-15 + 1e-16 + 1.1e-16) + 3 u = 9.1e-15 beta for a two-term force.  The gate is 4e-14 beta:
# about 4 x, because the 1e-16 of sin_reduced is a comment in device_common.hpp, not a proof.
FORCE_GATE = 4e-14

FORCE_SHAPES = [
    # (Mt, Mx, row j* of the third chain or None, beta)
    (64, 130, None, 1.0),     # 2 bands, ragged last band of 2 rows; 2 column tiles
    (130, 262, 128, 1.0),     # 3 bands, ragged last band of 6 rows; 3 tiles (62 + 62 + 6 columns)
    (256, 300, None, 1.0),    # 3 bands, ragged last band of 44 rows; 5 tiles
    (16, 128, None, 1.0),     # Mx = FORCE_ROWS: exactly one band, the row below it is the wrapped row 127
    (16, 129, 128, 1.0),      # a last band of ONE row, whose four-row look-ahead wraps to rows 0..3
    (16, 127, None, 1.0),     # one row short of a band
    (16, 256, None, 1.0),     # exactly two bands
    (16, 257, None, 2.5),     # two bands and a last band of one row (beta away from 1, where a forgotten coupling could hide)
    (62, 140, None, 1.0),     # Mt = FORCE_COLS: one tile that owns all 62 columns
    (63, 140, None, 1.0),     # last tile owns 1 column
    (124, 140, None, 1.0),    # two full tiles, the last owns 62
    (125, 140, None, 1.0),    # last tile owns 1 column (third tile)
    (61, 140, None, 1.0),     # one tile owning 61 columns: lane 62 holds column 0 again and must not emit
    (2, 2, None, 1.0),        # look-ahead laps the lattice more than once (Mx < 4); a wave holds the same column 32 times
    (2, 130, None, 1.0),      # the same columns many times in a wave, two bands
    (4, 3, None, 1.0),        # odd Mx < 4
    (6, 2, None, 1.0),        # Mx = 2: the row below and the row above are the same row
    (1024, 1024, None, 1.0),  # the timed shape: 8 bands x 17 tiles
    (2050, 136, None, 1.0),   # Mt past the 2048 switch of the reductions: 34 tiles, 2 bands
]


def schwinger_fields(Mt, Mx, jstar=None):
    """[B, 2 Mt Mx]: uniform(-pi, pi) from a seeded generator; the smooth seq(n); and, where jstar is given, a field
    that is constant along j except in row jstar (the first row of a band) -- its plaquettes are the same in every row
    except jstar - 1 and jstar, so its force on the mu = 0 links vanishes outside rows jstar - 1 .. jstar + 1: a kernel
    that takes a wrong row below the seam is O(beta) wrong in row jstar and nowhere else, and the message names it."""
    n = 2 * Mt * Mx
    rng = np.random.default_rng(1000 * Mt + Mx)
    x = [rng.uniform(-np.pi, np.pi, n), seq(n)]
    if jstar is not None:
        row = rng.uniform(-np.pi, np.pi, 2 * Mt)
        f = np.tile(row, Mx).reshape(Mx, 2 * Mt)
        f[jstar] = rng.uniform(-np.pi, np.pi, 2 * Mt)
        x.append(f.reshape(n))
    return np.vstack(x)


@pytest.mark.parametrize("Mt,Mx,jstar,beta", FORCE_SHAPES)
def test_schwinger_force_across_bands_and_tiles(gpu_ops, orc, Mt, Mx, jstar, beta):
    act, A = make_lattice(orc, "schwinger", Mt, Mx, beta=beta)
    x = schwinger_fields(Mt, Mx, jstar)
    assert np.max(np.abs(x)) <= np.pi
    xd = dev(x)
    F = force_into_nan(gpu_ops, act, xd).cpu().numpy()
    where = lambda l: where_schwinger(l, Mt)  # noqa: E731
    tag = f"schwinger force {Mt}x{Mx}"
    check_entries(F, ref.schwinger_force(x, Mt, Mx, beta), FORCE_GATE * beta, tag, where, 2 * Mt)
    # ops.lattice_force (its own output buffer) is the same call
    assert torch.equal(gpu_ops.lattice_force(act, xd), dev(F))
    for b in range(x.shape[0]):
        want = A.force(x[b])
        err = np.abs(F[b] - want)
        l = int(np.argmax(err))
        assert err[l] <= TOL * max(1.0, float(np.max(np.abs(want)))), \
            f"{tag} vs oracle: |diff| = {err[l]:.3e} in chain {b} at {where(l)}"
    if (Mt, Mx) == (1024, 1024):
        # beta (sin P - sin P shifted) rebuilt from the ORACLE's plaquettes (fp64 sums of four angles, each within
        # 4.2e-15 of the exact one: 8.4e-15 beta more on a two-term force, 1.75e-14 beta in all, inside the same gate)
        raw = np.zeros((x.shape[0], Mt * Mx))
        for b in range(x.shape[0]):
            orc.lib().orc_schwinger_plaquettes(A.h, x[b], raw[b])
        check_entries(F, ref.schwinger_force(None, Mt, Mx, beta, plaquettes=raw), FORCE_GATE * beta,
                      tag + " (from the oracle's plaquettes)", where, 2 * Mt)


def test_schwinger_force_of_a_chain_does_not_depend_on_its_batch(gpu_ops):
    """chain b of a batch of 3 equals, bit for bit, the same chain alone (130 x 262: 3 bands x 3 tiles = 9 waves, so the
    workgroups of four waves straddle bands and the last one is ragged)"""
    from mlmcpathintegral_amd import abi
    Mt, Mx = 130, 262
    act = abi.lattice_action(4, Mt, Mx, beta=1.7)
    x = schwinger_fields(Mt, Mx, 128)
    assert x.shape[0] == 3
    xd = dev(x)
    F = force_into_nan(gpu_ops, act, xd)
    assert torch.isfinite(F).all()
    for b in range(3):
        alone = force_into_nan(gpu_ops, act, xd[b:b + 1].contiguous())
        assert torch.equal(alone[0], F[b]), f"chain {b}"


# ---- 4. GFF force with both stride loops running ------------------------------------------------------------------------
# vs long double, per entry: five terms, |phi| <= 3, accumulated one after the other: four roundings of partial sums
# bounded by (kappa + 4) * 3 in magnitude, and the product kappa * phi is one more, inside the same bound when fused:
# 4 u (kappa + 4) 3.  Gate at 4 x that; FMA contraction only makes the error smaller.
def gff_force_gate(mu2):
    return 4 * (4 * U * (4 + mu2 + 4) * 3)


def gff_fields(M, B, seed):
    n = M * M
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, (B, n))
    x[0] = seq(n)
    return x


GFF_FORCE_SHAPES = [
    (257, 2),     # Mt = 256 + 1: the thread stride loop runs twice for exactly one column
    (512, 2),     # thread stride twice for every column (row_blocks = 512: one row per block)
    (128, 40),    # row_blocks = ceil(2048 / 40) = 52 < 128: the row stride loop runs two and three times
    (70, 2049),   # row_blocks = 1: one block walks every row
]


@pytest.mark.parametrize("mass", [10.0, 0.3])
@pytest.mark.parametrize("M,B", GFF_FORCE_SHAPES)
def test_gff_force_with_both_stride_loops(gpu_ops, orc, M, B, mass):
    act, A = make_lattice(orc, "gff", M, M, mass=mass)
    mu2 = orc.lib().orc_action_gff_mu2(A.h)
    x = gff_fields(M, B, 7 * M + B)
    assert np.max(np.abs(x)) <= 3
    F = force_into_nan(gpu_ops, act, dev(x)).cpu().numpy()
    where = lambda l: f"vertex (i={l % M}, j={l // M}): thread {l % M % 256}, pass {l % M // 256} of the thread stride"  # noqa: E731
    check_entries(F, ref.gff_force(x, M, M, mu2), gff_force_gate(mu2), f"gff force {M}^2 B={B} mass={mass}", where, M)
    for b in range(B):
        assert_close(F[b], A.force(x[b]), what=f"gff force vs oracle, chain {b}")


# ---- 5. reductions across NC and across B -------------------------------------------------------------------------------
# vs long double.  A sum of N terms accumulated per thread, then by a tree over the 256 threads and over the bands:
# (N / 256 + 12) u sum|term| for the additions (per-thread serial part, the trees), plus the error of the terms
# themselves: N * 3e-16 for 1 - cos P and cos P (cos_reduced states |x| 2e-16 + 1e-16 with |x| <= 4 pi).
def cos_sum_bound(N, sum_abs):
    return (N / 256 + 12) * U * sum_abs + N * 3e-16


def check_schwinger_reductions(gpu_ops, orc, Mt, Mx, beta, x, tag, n_oracle):
    """evaluate, qoi_avg_plaquette, qoi_2d_susceptibility of every chain of x against long double, and of the first
    n_oracle chains against the oracle; returns the device values"""
    act, A = make_lattice(orc, "schwinger", Mt, Mx, beta=beta)
    B, N = x.shape[0], Mt * Mx
    xd = dev(x)
    got = {"evaluate": gpu_ops.lattice_evaluate(act, xd).cpu().numpy(),
           "plaq": gpu_ops.qoi_avg_plaquette(xd, Mt, Mx).cpu().numpy(),
           "chi": gpu_ops.qoi_2d_susceptibility(xd, Mt, Mx).cpu().numpy()}
    worst = {"evaluate": 0.0, "plaq": 0.0, "chi": 0.0}
    for c0 in range(0, B, 128):   # (chunks of chains: the long-double temporaries of 2049 chains would take gigabytes)
        xs = x[c0:c0 + 128]
        P = ref.schwinger_plaquettes(xs, Mt, Mx)
        w = ref.mod_2pi(P)
        # mod_2pi is discontinuous at +-pi, where one ulp in P would change Q by one: the inputs keep away from it
        cut = np.min(np.abs(np.abs(w) - ref.PI), axis=-1)
        assert np.all(cut > 1e-9), f"{tag}: a plaquette within {float(np.min(cut)):.1e} of +-pi: choose another seed"
        cosP = np.cos(P)
        S = LD(beta) * np.sum(1 - cosP, axis=-1)
        plaq = np.sum(cosP, axis=-1) / LD(N)
        s = np.sum(w, axis=-1)
        chi = s * s / (4 * ref.PI * ref.PI)
        for k in range(xs.shape[0]):
            b = c0 + k
            bound_S = beta * (cos_sum_bound(N, float(np.sum(1 - cosP[k]))) + U * float(S[k]) / beta)
            bound_p = cos_sum_bound(N, float(np.sum(np.abs(cosP[k])))) / N + U
            # Q: the terms mod_2pi(P) carry the 4.2e-15 of the fp64 angle sum and 2 u 4 pi of the reduction: 5.6e-15;
            # chi = s^2 / 4 pi^2, so d chi = (2 |s| ds + ds^2) / 4 pi^2, and three more roundings
            ds = (N / 256 + 12) * U * float(np.sum(np.abs(w[k]))) + N * 5.6e-15
            bound_c = (2 * abs(float(s[k])) * ds + ds * ds) / (4 * np.pi ** 2) + 3 * U * float(chi[k])
            for name, want, bound in (("evaluate", S[k], bound_S), ("plaq", plaq[k], bound_p), ("chi", chi[k], bound_c)):
                err = abs(float(LD(got[name][b]) - want))
                worst[name] = max(worst[name], err / bound)
                assert err <= bound, f"{tag} {name}, chain {b}: |error| = {err:.3e} > {bound:.3e} (value {float(want):.6g})"
    print(f"[bands] {tag}: worst error / derived bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    L = orc.lib()
    for b in range(min(n_oracle, B)):
        assert_close(got["evaluate"][b], A.evaluate(x[b]), what=f"{tag} evaluate vs oracle")
        assert_close(got["plaq"][b], L.orc_qoi_avg_plaquette(x[b], Mt, Mx), what=f"{tag} plaquette vs oracle")
        assert_close(got["chi"][b], L.orc_qoi_2d_susceptibility(x[b], Mt, Mx), tol=1e-10, what=f"{tag} chi vs oracle")
    return got


def reduction_fields(Mt, Mx, B, seed):
    n = 2 * Mt * Mx
    x = np.random.default_rng(seed).uniform(-np.pi, np.pi, (B, n))
    if B > 1:
        x[1] = seq(n)
    return x


# NC = ceil(Mt / 256) columns per thread of schwinger_reduce_band_kernel; Mt < 64 or Mt > 2048 take lattice_reduce_kernel
REDUCE_MT = [63,      # generic kernel, just below the switch
             64,      # NC = 1, the smallest lattice of the band kernel: three of four waves idle
             65, 256,  # NC = 1; 256: every thread exactly one column
             257,     # NC = 2 with one column in the second pass
             512,     # NC = 2
             600,     # NC = 3
             1030,    # NC = 5
             1300,    # NC = 6
             1600,    # NC = 7
             1800,    # NC = 8
             2048,    # NC = 8, the largest lattice of the band kernel
             2050]    # generic kernel, just above the switch


@pytest.mark.parametrize("Mt", REDUCE_MT)
def test_schwinger_reductions_for_every_column_count(gpu_ops, orc, Mt):
    Mx, B, beta = 24, 2, 1.3
    x = reduction_fields(Mt, Mx, B, seed=Mt)
    check_schwinger_reductions(gpu_ops, orc, Mt, Mx, beta, x, f"reduce {Mt}x{Mx} B={B}", n_oracle=B)


def test_schwinger_reductions_cover_nc_4(gpu_ops, orc):
    """NC = 4 (the timed 1024 columns) at a height the long-double reference affords; with REDUCE_MT: NC = 1..8"""
    x = reduction_fields(1000, 24, 2, seed=1000)
    check_schwinger_reductions(gpu_ops, orc, 1000, 24, 1.3, x, "reduce 1000x24 B=2", n_oracle=2)


# (128, 100): row_blocks(100, B) = min(100, ceil(2048 / B)) bands are asked for, bands shorter than 8 rows are made 8
REDUCE_B = [1,       # 100 bands of 1 row asked: clamped to 8 rows, 13 bands, the last of 4 rows
            33,      # ceil(2048 / 33) = 63 bands of 2 rows asked: clamped to 8 rows again
            200,     # 11 bands asked: 10 rows per band, 10 bands
            300,     # 7 bands asked: 15 rows per band, 7 bands, the last of 10 rows
            2049]    # one band of all 100 rows: nsplit = 1


@pytest.mark.parametrize("B", REDUCE_B)
def test_schwinger_reductions_for_every_band_height(gpu_ops, orc, B):
    Mt, Mx, beta = 128, 100, 0.9
    x = reduction_fields(Mt, Mx, B, seed=100 + B)
    got = check_schwinger_reductions(gpu_ops, orc, Mt, Mx, beta, x, f"reduce {Mt}x{Mx} B={B}", n_oracle=3)
    # The value of a chain must not depend on its batch beyond the order of the sum: alone (B = 1) the bands are 8 rows,
    # in the batch they are whatever B made them, and lattice_finish_kernel adds the band sums in an order fixed by
    # their number -- so 1e-13 relative (the project's scale: max(1, |value|)), not bit for bit.
    act, _ = make_lattice(orc, "schwinger", Mt, Mx, beta=beta)
    for b in sorted({0, 1, B // 2, B - 1} & set(range(B))):
        xb = dev(x[b:b + 1])
        assert_close(gpu_ops.lattice_evaluate(act, xb).cpu().numpy()[0], got["evaluate"][b], tol=1e-13, what=f"evaluate alone, chain {b}")
        assert_close(gpu_ops.qoi_avg_plaquette(xb, Mt, Mx).cpu().numpy()[0], got["plaq"][b], tol=1e-13, what=f"plaquette alone, chain {b}")
        assert_close(gpu_ops.qoi_2d_susceptibility(xb, Mt, Mx).cpu().numpy()[0], got["chi"][b], tol=1e-13, what=f"chi alone, chain {b}")


@pytest.mark.parametrize("M,B", [(257, 2), (128, 40)])
@pytest.mark.parametrize("mass", [10.0, 0.3])
def test_gff_reductions_with_both_stride_loops(gpu_ops, orc, M, B, mass):
    """evaluate and qoi_phi_squared through lattice_reduce_kernel: 257 columns (thread stride), 52 blocks for 128 rows
    (row stride).  Bounds vs long double, |phi| <= 3, N = M^2 terms: the additions (N / 256 + 12) u sum|term| as for the
    plaquette sums; the terms: phi^2 is one rounding, u phi^2; phi * (kappa phi - four neighbours) is the force's
    4 u (kappa + 4) 3 times |phi|, and one rounding of the product."""
    act, A = make_lattice(orc, "gff", M, M, mass=mass)
    L = orc.lib()
    mu2 = L.orc_action_gff_mu2(A.h)
    N = M * M
    x = gff_fields(M, B, 11 * M + B)
    xd = dev(x)
    S = gpu_ops.lattice_evaluate(act, xd).cpu().numpy()
    q = gpu_ops.qoi_phi_squared(xd).cpu().numpy()
    xl = x.astype(LD)
    term = xl * ref.gff_force(x, M, M, mu2)
    S_ref, q_ref = ref.gff_action(x, M, M, mu2), ref.phi_squared(x)
    worst_S = worst_q = 0.0
    for b in range(B):
        sa = float(np.sum(np.abs(term[b])))
        bound_S = 0.5 * ((N / 256 + 12) * U * sa + float(np.sum(np.abs(xl[b]))) * 4 * U * (8 + mu2) * 3 + U * sa) + U * abs(float(S_ref[b]))
        bound_q = ((N / 256 + 12) * U + 2 * U) * float(q_ref[b])
        eS, eq = abs(float(LD(S[b]) - S_ref[b])), abs(float(LD(q[b]) - q_ref[b]))
        worst_S, worst_q = max(worst_S, eS / bound_S), max(worst_q, eq / bound_q)
        assert eS <= bound_S, f"gff evaluate {M}^2 chain {b}: |error| = {eS:.3e} > {bound_S:.3e}"
        assert eq <= bound_q, f"phi^2 {M}^2 chain {b}: |error| = {eq:.3e} > {bound_q:.3e}"
        assert_close(S[b], A.evaluate(x[b]), what="gff evaluate vs oracle")
        assert_close(q[b], L.orc_qoi_2d_phi_squared(x[b], N), what="phi^2 vs oracle")
    print(f"[bands] gff reduce {M}^2 B={B} mass={mass}: worst error / derived bound: evaluate {worst_S:.3f}, phi^2 {worst_q:.3f}")


# ---- 3. 2-D HMC on lattices the step kernel has to work for -------------------------------------------------------------
def oracle_momenta(orc, n, chain, step):
    """the momenta of dev_hmc_trajectory: the cosine branch of one Box-Muller pair per entry (purpose P_MOMENTUM)"""
    L, out, p = orc.lib(), np.zeros(4), np.empty(n)
    for l in range(n):
        L.orc_dev_random(SEED, chain, step, l, orc.P_MOMENTUM, 0, out)
        p[l] = out[2]
    return p


def oracle_hmc(orc, A, x0, nt, dt, n_rep, chain0, n_draws):
    """HMCSampler::draw with n_rep repetitions (hmcsampler.cc:10-12: `accept = accept or single_step()`), n_draws times
    per chain, by the oracle alone.  Returns per draw the states, the accept flags, the energies of the last repetition
    that ran, the repetition that accepted (-1: none), and the smallest |u - exp(-dH)| over the Metropolis tests."""
    B = x0.shape[0]
    x = x0.copy()
    states, flags, energies, first = [], np.zeros((n_draws, B), dtype=int), np.zeros((n_draws, B, 4)), np.full((n_draws, B), -1)
    margin, out = np.inf, np.zeros(4)
    for d in range(n_draws):
        for b in range(B):
            a = 0
            for r in range(n_rep):
                if a:
                    break
                a, en, dH = A.dev_hmc_trajectory(x[b], nt, dt, SEED, chain0 + b, d * n_rep + r)
                if dH >= 0:
                    orc.lib().orc_dev_random(SEED, chain0 + b, d * n_rep + r, 0, orc.P_ACCEPT, 0, out)
                    margin = min(margin, abs(out[0] - np.exp(-dH)))
                if a:
                    first[d, b] = r
            flags[d, b], energies[d, b] = a, en
        states.append(x.copy())
    return states, flags, energies, first, margin


def hmc_start(kind, n, B, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (B, n))


def kinetic_bound(p):
    """T = 1/2 sum p^2 vs long double of the ORACLE's momenta: the additions (n / 256 + 12) u sum p^2 and one rounding
    per square, u sum p^2; and the device's momenta are not the oracle's bit for bit: Box-Muller sqrt(-2 ln u) cos(2 pi v)
    with |sqrt| <= 9.5 takes the rounding of 2 pi v (4 u 2 pi on the cosine's argument) and a few ulp of log, sqrt
    and cos between libm and the device library, <= 1.5e-14 per momentum in all, so 1.5e-14 sum|p| on sum p^2 / 2."""
    n, s2 = p.size, float(np.sum(p.astype(LD) ** 2))
    return 0.5 * ((n / 256 + 13) * U * s2) + 1.5e-14 * float(np.sum(np.abs(p)))


HMC_CASES = [
    # kind, Mt, Mx, kw, B: the kinetic energy (lattice_sum_squares) sums n = w * h momenta as h rows of w, w the largest power of two in
    # [64, 4096] that divides n, or as one row of n where there is none
    ("schwinger", 192, 260, dict(beta=1.0), 3),   # 3 bands x 4 tiles; n = 99840 = 2^9 * 195: w = 512
    ("schwinger", 130, 70, dict(beta=2.0), 3),    # n = 18200 = 2^3 * 5^2 * 7 * 13: the one-row fall-back
    ("schwinger", 64, 256, dict(beta=1.0), 3),    # two bands; n = 32768: w = 4096
    ("gff", 300, 300, dict(mass=10.0), 3),        # thread stride of the step kernel; n = 90000 = 2^4 * 5625: fall-back
    ("gff", 128, 128, dict(mass=10.0), 40),       # row_blocks = 52 < 128: row stride in the step kernel and the reductions
]


@pytest.mark.parametrize("kind,Mt,Mx,kw,B", HMC_CASES)
def test_lattice_hmc_on_many_bands_matches_oracle(gpu_ops, orc, kind, Mt, Mx, kw, B):
    """tolerances of test_lattice_hmc_matches_oracle: energies 1e-11, state 1e-10, accept flags equal.  The HMC's kinetic
    energy cannot be called on its own: it is pinned through T0 = energies[:, 1] of the first trajectory against 1/2 sum p^2 in
    long double, with p rebuilt by the oracle's momentum draw (orc_dev_random, purpose P_MOMENTUM), for three chains."""
    act, A = make_lattice(orc, kind, Mt, Mx, **kw)
    n, nt, dt, chain0 = A.size, 8, 0.05, 2
    x0 = hmc_start(kind, n, B, 3)
    xd = dev(x0)
    hmc = gpu_ops.LatticeHMC(act, B, nt, dt, seed=SEED, chain0=chain0)
    xo = x0.copy()
    for t in range(3):
        acc = hmc.draw(xd).cpu().numpy()
        en = hmc.energies.cpu().numpy()
        for b in range(B):
            a, e, _ = A.dev_hmc_trajectory(xo[b], nt, dt, SEED, chain0 + b, t)
            assert_close(en[b], e, tol=1e-11, what=f"energies, trajectory {t}, chain {b}")
            assert acc[b] == a, (t, b)
        assert_close(xd.cpu().numpy(), xo, tol=1e-10, what=f"state after trajectory {t}")
        if t == 0:
            for b in range(min(B, 3)):
                p = oracle_momenta(orc, n, chain0 + b, 0)
                T0, bound = ref.kinetic_energy(p), kinetic_bound(p)
                err = abs(float(LD(en[b, 1]) - T0))
                print(f"[bands] hmc {kind} {Mt}x{Mx} chain {b}: |T0 - sum p^2 / 2| = {err:.3e} (bound {bound:.3e}), T0 = {float(T0):.6f}")
                assert err <= bound, f"T0 of chain {b}: |error| = {err:.3e} > {bound:.3e}"


# n_rep = 3.  dt was chosen on the CPU with the oracle alone (scanning dt at these seeds) so that over the chains and
# draws of the case some chains accept at the first repetition, some later and at least one never; no Metropolis test of
# the case has u within 1e-9 of exp(-dH) (asserted below: were one closer, another dt or seed would be the remedy, not
# a looser comparison of the flags).
HMC_REP_CASES = [
    ("schwinger", 64, 130, dict(beta=1.0), 4, 6, 0.10),   # 2 bands x 2 tiles; accepting repetition 0 / later / none: 5 / 3 / 4 of 12
    ("gff", 128, 128, dict(mass=10.0), 40, 6, 0.10),      # row stride with chains that are done and chains that are not; 93 / 20 / 7 of 120
]


@pytest.mark.parametrize("kind,Mt,Mx,kw,B,nt,dt", HMC_REP_CASES)
def test_lattice_hmc_repeats_until_accepted(gpu_ops, orc, kind, Mt, Mx, kw, B, nt, dt):
    act, A = make_lattice(orc, kind, Mt, Mx, **kw)
    n, n_rep, chain0, n_draws = A.size, 3, 2, 3
    x0 = hmc_start(kind, n, B, 5)
    states, flags, energies, first, margin = oracle_hmc(orc, A, x0, nt, dt, n_rep, chain0, n_draws)
    # the mix, from the oracle's own flags, before the device is looked at
    assert (first == 0).any() and (first > 0).any() and (first < 0).any(), f"accepting repetitions: {first.tolist()}"
    assert margin > 1e-9, f"a Metropolis test within {margin:.1e} of its threshold"
    xd = dev(x0)
    hmc = gpu_ops.LatticeHMC(act, B, nt, dt, n_rep=n_rep, seed=SEED, chain0=chain0)
    for d in range(n_draws):
        acc = hmc.draw(xd).cpu().numpy()
        en = hmc.energies.cpu().numpy()
        assert acc.tolist() == flags[d].tolist(), f"draw {d}: accepting repetitions {first[d].tolist()}"
        for b in range(B):
            assert_close(en[b], energies[d, b], tol=1e-11, what=f"energies of the last repetition, draw {d}, chain {b}")
        assert_close(xd.cpu().numpy(), states[d], tol=1e-10, what=f"state after draw {d}")
