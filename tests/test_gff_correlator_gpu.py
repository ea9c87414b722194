"""GPU: mlmcpi_gff_correlator against the long-double definition (tests/gff_correlator_reference.py) on both layouts, spikes on
both sides of every tile, band and chunk boundary, the identities, its determinism contract bit for bit, the accumulator, the
65535-chain edge of the launch grid, guard bands and refusals, and the law of <C(tau; q)> and E_q of the GFF action at (16, 16),
mass 4 (exact sampler and overrelaxed heat bath).

Bound of the parity test, absolute and per entry: k eps (1/N) sum_i A_i A_{i + tau}, A_i = sum over the slice of |phi|, with
k = 2 sqrt(2) (n + 3) + 2 + ceil(M_d / 64) + 6 + 2 and n = min(rows, 256) + bands (direction t) or min(columns, 64) + chunks
(direction x) of the route built; the derivation stands beside gff_correlator_reference.rounding_count.  Largest observed
|error| / bound per shape: DESIGN.md 4.1e.  The records of one run are profiles/gff_correlator_zscores.json (this module writes the
z-scores and the parity ratios into the directory MLMCPI_GFF_CORRELATOR_RECORDS names, if the variable is set)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gff_correlator_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
RECORDS = os.environ.get("MLMCPI_GFF_CORRELATOR_RECORDS")
B_BIG = 70

# (Mt, Mx, P, rotated, largest batch); (130, 514) is there because (66, 34) and (130, 70) fit one band of 256 rows
SMALL = [(2, 2, 2), (2, 6, 2), (6, 2, 2), (16, 16, 8), (66, 34, 8), (130, 70, 5), (130, 514, 5)]
FIELDS = [(Mt, Mx, P, rot, B_BIG) for Mt, Mx, P in SMALL for rot in (0, 1)] + [(1024, 1024, 8, 0, 2), (1024, 1024, 1, 1, 2)]
CASES = [f[:4] + (B,) for f in FIELDS for B in ((3, B_BIG) if f[4] == B_BIG else (f[4],))]

REFERENCE = {}


def _reference(Mt, Mx, P, rot):
    """the spiked field of a shape at its largest batch, its long-double correlators and their bound, computed once and shared; a
    smaller batch is the first chains of the same field"""
    key = (Mt, Mx, P, rot)
    if key not in REFERENCE:
        B = [f[4] for f in FIELDS if f[:4] == key][0]
        phi = ref.spiked_field(977 * Mt + 31 * Mx + 2 * P + rot, B, Mt, Mx, rot)
        want, bound = ref.correlator(phi, Mt, Mx, P, rot), ref.bound(phi, Mt, Mx, P, rot)
        for a in (phi, want, bound):
            a.setflags(write=False)
        REFERENCE[key] = (phi, want, bound)
    return REFERENCE[key]


def _record(name, payload):
    if RECORDS:
        os.makedirs(RECORDS, exist_ok=True)
        path = os.path.join(RECORDS, "gff_correlator_zscores.json")
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = payload
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


RATIOS = {}


@pytest.mark.parametrize("case", CASES, ids=lambda v: "x".join(map(str, v)))
def test_parity_with_the_long_double_reference(gpu_ops, case):
    import torch
    from mlmcpathintegral_amd import ops
    Mt, Mx, P, rot, B = case
    p = ref.plan(Mt, Mx, rot, P, B)
    assert ops.gff_correlator_plan(Mt, Mx, P, rot, B) == p
    if (Mt, Mx) in ((130, 514), (1024, 1024)):
        assert p["bands"] > 1 and p["chunks"] > 1
    phi, want, bound = _reference(Mt, Mx, P, rot)
    got = ops.gff_correlator(torch.tensor(phi[:B]).cuda(), Mt, Mx, P, bool(rot)).cpu().numpy()
    assert got.shape == (B, ref.n_out(Mt, Mx, P)) and np.isfinite(got).all()
    err = np.abs((got - want[:B]).astype(np.float64))
    ratio = float(np.max(err / bound[:B]))
    print(f"[gff correlator] {Mt} x {Mx} rotated {rot} P {P} B {B}: bands {p['bands']} chunks {p['chunks']} k_t "
          f"{ref.rounding_count(Mt, Mx, rot, 0):.0f} k_x {ref.rounding_count(Mt, Mx, rot, 1):.0f}: max |err| {err.max():.3e}, max err / bound {ratio:.4f}")
    RATIOS["x".join(map(str, case))] = ratio
    _record("parity", {"max_ratio_to_bound": max(RATIOS.values()), "cases": dict(RATIOS)})
    assert ratio <= 1.0, ratio


def test_the_case_list_reaches_every_geometry():
    plans = [ref.plan(c[0], c[1], c[3], c[2], c[4]) for c in CASES]
    assert {(p["bands"] > 1, p["chunks"] > 1) for p in plans} >= {(False, False), (False, True), (True, True)}
    assert {p["vector_loads"] for p in plans} == {0, 1} and {p["planes"] for p in plans} == {1, 2}
    assert any(p["chunks"] >= 3 for p in plans) and any(p["bands"] >= 3 for p in plans)
    assert {c[2] for c in CASES} >= {1, 2, 5, 8} and max(c[4] for c in CASES) > 64
    # the spikes sit on both sides of every boundary of the plan, in the first and last row and column and at the corners
    sites = set(ref.boundary_sites(130, 514, 0).tolist())
    for r in (0, 63, 64, 255, 256, 511, 512, 513):
        for c in (0, 63, 64, 127, 128, 129):
            assert r * 130 + c in sites


def test_zero_momentum_sums_to_the_square_of_the_total(gpu_ops):
    """N sum_tau w(tau) C_t(tau; 0) = (sum phi)^2, and along x, within the same bound"""
    import torch
    from mlmcpathintegral_amd import ops
    for Mt, Mx, P, rot in [(66, 34, 8, 0), (66, 34, 8, 1), (2, 6, 2, 0)]:
        phi, _, bound = _reference(Mt, Mx, P, rot)
        got = ops.gff_correlator(torch.tensor(phi).cuda(), Mt, Mx, P, bool(rot)).cpu().numpy()
        n, total = ref.n_vertices(Mt, Mx, rot), phi.astype(ref.LD).sum(axis=1) ** 2
        for d, M in ((0, Mt), (1, Mx)):
            w = np.array([1 if t == 0 or 2 * t == M else 2 for t in range(M // 2 + 1)])
            C0, b0 = ref.split(got, Mt, Mx, P)[d][:, 0], ref.split(bound, Mt, Mx, P)[d][:, 0]
            assert np.all(np.abs((n * (w * C0.astype(ref.LD)).sum(axis=1) - total).astype(np.float64)) <= n * (w * b0).sum(axis=1)), (Mt, Mx, rot, d)


def test_parseval_against_phi_squared(gpu_ops):
    """every momentum of the projected direction fits P = 3 at extent 4: sum_q w_q C_x(0; q) = Mt phi^2 on (4, 6), sum_q w_q C_t(0; q)
    = Mx phi^2 on (6, 4), phi^2 = mlmcpi_qoi_phi_squared (itself N roundings of a sum of squares)"""
    import torch
    from mlmcpathintegral_amd import ops
    rng = np.random.default_rng(11)
    w = np.array([1.0, 2.0, 1.0])
    for Mt, Mx, d in [(4, 6, 1), (6, 4, 0)]:
        phi = rng.standard_normal((5, Mt * Mx))
        dev = torch.tensor(phi).cuda()
        got, phi2 = ops.gff_correlator(dev, Mt, Mx, 3).cpu().numpy(), ops.qoi_phi_squared(dev).cpu().numpy()
        C0, b0 = ref.split(got, Mt, Mx, 3)[d][:, :, 0], ref.split(ref.bound(phi, Mt, Mx, 3), Mt, Mx, 3)[d][:, :, 0]
        M = Mt if d else Mx
        assert np.all(np.abs((w * C0).sum(axis=1) - M * phi2) <= (w * b0).sum(axis=1) + (Mt * Mx + 4) * ref.EPS * M * phi2), (Mt, Mx)


def test_plane_wave_on_the_device(gpu_ops):
    """cos(2 pi (k i / Mt + q0 j / Mx)): momentum q0 alone along t with C_t = (Mx/4) cos(2 pi k tau / Mt), momentum k alone along x; the
    field is rounded to double once (1/2 ulp per vertex: twice the bound covers it)"""
    import torch
    from mlmcpathintegral_amd import ops
    Mt, Mx, k, q0, P = 8, 8, 1, 2, 5
    i, j = ref.coordinates(Mt, Mx, 0)
    phi = np.cos(2 * ref.PI * (k * i.astype(ref.LD) / Mt + q0 * j.astype(ref.LD) / Mx)).astype(np.float64)[None, :]
    got = ops.gff_correlator(torch.tensor(phi).cuda(), Mt, Mx, P).cpu().numpy()
    bound = 2 * ref.bound(phi, Mt, Mx, P)
    Ct, Cx = ref.split(got, Mt, Mx, P)
    bt, bx = ref.split(bound, Mt, Mx, P)
    tau = np.arange(Mt // 2 + 1)
    for q in range(P):
        assert np.all(np.abs(Ct[0, q] - (Mx / 4 * np.cos(2 * np.pi * k * tau / Mt) if q == q0 else 0)) <= bt[0, q]), q
        assert np.all(np.abs(Cx[0, q] - (Mt / 4 * np.cos(2 * np.pi * q0 * tau / Mx) if q == k else 0)) <= bx[0, q]), q


@pytest.mark.parametrize("Mt,Mx,P,rot", [(66, 34, 8, 0), (66, 34, 8, 1), (130, 514, 5, 1)])
def test_a_chain_is_the_same_bits_however_it_is_batched(gpu_ops, Mt, Mx, P, rot):
    import torch
    from mlmcpathintegral_amd import ops
    phi = torch.tensor(_reference(Mt, Mx, P, rot)[0]).cuda()
    whole = ops.gff_correlator(phi, Mt, Mx, P, bool(rot))
    for b in (0, 32, 33, B_BIG - 1):
        assert torch.equal(ops.gff_correlator(phi[b:b + 1].contiguous(), Mt, Mx, P, bool(rot))[0], whole[b]), b
    parts = torch.cat([ops.gff_correlator(phi[:33].contiguous(), Mt, Mx, P, bool(rot)), ops.gff_correlator(phi[33:].contiguous(), Mt, Mx, P, bool(rot))])
    assert torch.equal(parts, whole)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = ops.gff_correlator(phi, Mt, Mx, P, bool(rot))
    side.synchronize()
    assert torch.equal(other, whole)
    # with d_acc: the same output; after two calls the sums of C and C^2
    acc = torch.zeros((B_BIG, whole.shape[1], 2), dtype=torch.float64, device="cuda")
    assert torch.equal(ops.gff_correlator(phi, Mt, Mx, P, bool(rot), acc=acc), whole)
    flipped = phi.flip(0).contiguous()
    second = ops.gff_correlator(flipped, Mt, Mx, P, bool(rot), acc=acc)
    assert torch.equal(second, whole.flip(0))
    assert torch.equal(acc[..., 0], whole + second) and torch.equal(acc[..., 1], whole * whole + second * second)


@pytest.mark.parametrize("Mt,Mx,P", [(2, 2, 1), (4, 4, 2)])
@pytest.mark.parametrize("n_chains", [65535, 65581])
def test_the_grid_edge(gpu_ops, Mt, Mx, P, n_chains):
    """what the chain-count table gives the exports with a `uint32_t B`: every chain against the same call split at 40000, and the
    chains at both ends and around 65535 against the reference (they carry spikes) and against a call of one chain"""
    import torch
    from mlmcpathintegral_amd import ops
    rng = np.random.default_rng(Mt + n_chains)
    phi = rng.standard_normal((n_chains, Mt * Mx))
    pins = [b for b in (0, 1, 65534, 65535, 65536, n_chains - 1) if b < n_chains]
    phi[pins] += rng.uniform(20, 100, (len(pins), Mt * Mx))
    dev = torch.tensor(phi).cuda()
    acc = torch.zeros((n_chains, ref.n_out(Mt, Mx, P), 2), dtype=torch.float64, device="cuda")
    whole = ops.gff_correlator(dev, Mt, Mx, P, acc=acc)
    parts = torch.cat([ops.gff_correlator(dev[:40000].contiguous(), Mt, Mx, P), ops.gff_correlator(dev[40000:].contiguous(), Mt, Mx, P)])
    assert torch.equal(parts, whole) and torch.equal(acc[..., 0], whole) and torch.equal(acc[..., 1], whole * whole)
    got = whole[pins].cpu().numpy()
    want, bound = ref.correlator(phi[pins], Mt, Mx, P), ref.bound(phi[pins], Mt, Mx, P)
    assert np.all(np.abs((got - want).astype(np.float64)) <= bound)
    for b in pins:
        assert torch.equal(ops.gff_correlator(dev[b:b + 1].contiguous(), Mt, Mx, P)[0], whole[b]), b


def _raw(lib, Mt, Mx, rot, P, phi, n, out, acc, work, nbytes):
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    import torch
    return lib.mlmcpi_gff_correlator(Mt, Mx, rot, P, ptr(phi), n, ptr(out), ptr(acc), ptr(work), nbytes,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_guard_bands_and_refusals(gpu_ops):
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    Mt, Mx, P, B, G = 66, 34, 8, 3, 512
    for rot in (0, 1):
        phi = torch.tensor(_reference(Mt, Mx, P, rot)[0][:B]).cuda()
        n_out, nbytes = ref.n_out(Mt, Mx, P), ref.plan(Mt, Mx, rot, P, B)["work_bytes"]
        out = torch.full((G + B * n_out + G,), SENTINEL, dtype=torch.float64, device="cuda")
        acc = torch.full((G + 2 * B * n_out + G,), SENTINEL, dtype=torch.float64, device="cuda")
        work = torch.full((256 * 8 + nbytes + 256 * 8,), 0x5A, dtype=torch.uint8, device="cuda")
        o, a, w = out[G:G + B * n_out], acc[G:G + 2 * B * n_out], work[2048:2048 + nbytes]
        assert w.data_ptr() % 256 == 0
        refusals = [((Mt + 1, Mx, rot, P, phi, B, o, a, w, nbytes), -1), ((Mt, 0, rot, P, phi, B, o, a, w, nbytes), -1),
                    ((1 << 16, 1 << 15, rot, P, phi, B, o, a, w, nbytes), -1), ((Mt, Mx, rot, 0, phi, B, o, a, w, nbytes), -1),
                    ((Mt, Mx, rot, 9, phi, B, o, a, w, nbytes), -3), ((16, 4, rot, 4, phi, B, o, a, w, nbytes), -1),
                    ((4, 16, rot, 4, phi, B, o, a, w, nbytes), -1), ((Mt, Mx, rot, P, None, B, o, a, w, nbytes), -1),
                    ((Mt, Mx, rot, P, phi, B, None, a, w, nbytes), -1), ((Mt, Mx, rot, P, phi, B, o, a, None, nbytes), -1),
                    ((Mt, Mx, rot, P, phi, 0, o, a, w, nbytes), -1), ((Mt, Mx, rot, P, phi, B, o, a, w, nbytes - 1), -1)]
        for args, status in refusals:
            assert _raw(lib, *args) == status, args[:4]
            assert lib.mlmcpi_last_error()
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((acc == SENTINEL).all()) and bool((work == 0x5A).all())
        a.zero_()
        assert _raw(lib, Mt, Mx, rot, P, phi, B, o, a, w, nbytes) == 0
        torch.cuda.synchronize()
        for buf, lo, hi, s in ((out, G, G + B * n_out, SENTINEL), (acc, G, G + 2 * B * n_out, SENTINEL), (work, 2048, 2048 + nbytes, 0x5A)):
            assert bool((buf[:lo] == s).all()) and bool((buf[hi:] == s).all())
        want, bound = _reference(Mt, Mx, P, rot)[1:]
        got = o.reshape(B, n_out).cpu().numpy()
        assert np.all(np.abs((got - want[:B]).astype(np.float64)) <= bound[:B])
        assert torch.equal(a.reshape(B, n_out, 2)[..., 0], o.reshape(B, n_out))


# ---- the law: GFF action on (16, 16), mass 4, P = 4 ----
LAW = dict(M=16, mass=4.0, P=4, chains=1024)


def _exact_table():
    M, P = LAW["M"], LAW["P"]
    one = np.array([[float(ref.correlator_exact(M, M, LAW["mass"], q, tau)) for tau in range(M // 2 + 1)] for q in range(P)]).reshape(-1)
    return np.concatenate([one, one])       # the square lattice: C_x has the law of C_t


EXACT_RUN = {}


def _exact_run():
    """1024 chains x 50 exact draws (a fresh step each: independent), C and C^2 accumulated per chain; run once and shared"""
    if not EXACT_RUN:
        import torch
        from mlmcpathintegral_amd import abi, ops
        M, P, B = LAW["M"], LAW["P"], LAW["chains"]
        act = abi.lattice_action(abi.GFF, M, M, mass=LAW["mass"])
        sampler = ops.GFFExactSampler(act, B, seed=20261020)
        acc = torch.zeros((B, ref.n_out(M, M, P), 2), dtype=torch.float64, device="cuda")
        work = ops.gff_correlator_workspace(M, M, P, B)
        for _ in range(50):
            ops.gff_correlator(sampler.draw(), M, M, P, acc=acc, work=work)
        EXACT_RUN["acc"] = acc.cpu().numpy()
    return EXACT_RUN["acc"]


def test_law_with_the_exact_sampler(gpu_ops):
    acc = _exact_run()
    n = LAW["chains"] * 50
    mean, sq = acc[..., 0].sum(axis=0) / n, acc[..., 1].sum(axis=0) / n
    err = np.sqrt((sq - mean * mean) * n / (n - 1.0) / n)
    z = (mean - _exact_table()) / err
    print(f"[gff correlator] exact sampler, {n} samples: max |z| {np.abs(z).max():.3f} over {z.size} entries")
    _record("law_exact_sampler", {"samples": n, "max_abs_z": float(np.abs(z).max()), "z": z.tolist()})
    assert z.size == 72 and np.abs(z).max() < 4.5, z


def test_law_with_the_overrelaxed_heat_bath(gpu_ops):
    """chains start from mlmcpi_lattice_initialise, for the GFF an exact draw: in equilibrium without a warm-up; 40 draws of 10 + 1
    sweeps; the error is the spread of the per-chain means"""
    import torch
    from mlmcpathintegral_amd import abi, ops
    M, P, B, draws = LAW["M"], LAW["P"], LAW["chains"], 40
    act = abi.lattice_action(abi.GFF, M, M, mass=LAW["mass"])
    phi = ops.lattice_initialise(act, B, 4711)
    scratch = torch.empty_like(phi)
    acc = torch.zeros((B, ref.n_out(M, M, P), 2), dtype=torch.float64, device="cuda")
    for d in range(draws):
        ops.lattice_sweep_draw(act, phi, scratch, 10, 1, 4711, 0, 11 * d)
        ops.gff_correlator(phi, M, M, P, acc=acc)
    per_chain = acc[..., 0].cpu().numpy() / draws
    mean, err = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(B)
    z = (mean - _exact_table()) / err
    print(f"[gff correlator] heat bath, {B} chains x {draws} draws: max |z| {np.abs(z).max():.3f} over {z.size} entries")
    _record("law_heatbath", {"chains": B, "draws": draws, "max_abs_z": float(np.abs(z).max()), "z": z.tolist()})
    assert z.size == 72 and np.abs(z).max() < 4.5, z


def test_energies_follow_the_dispersion_relation(gpu_ops):
    """E_q from the effective mass of C_t at tau = 2, q = 0 .. 3, with the jackknife over the 1024 chains of the exact-sampler run"""
    acc = _exact_run()
    M, P, B = LAW["M"], LAW["P"], LAW["chains"]
    m = ref.split(acc[..., 0] / 50, M, M, P)[0]                         # per-chain means of C_t [B, P, 9]
    mass_of = lambda c: np.arccosh((c[..., 1] + c[..., 3]) / (2 * c[..., 2]))
    total, rows = m.sum(axis=0), []
    for q in range(P):
        value = mass_of(total[q] / B)
        leave = mass_of((total[q][None, :] - m[:, q]) / (B - 1.0))
        error = np.sqrt((B - 1.0) / B * np.sum((leave - leave.mean()) ** 2))
        want = float(ref.dispersion_exact(M, M, LAW["mass"], q))
        rows.append({"q": q, "E": float(value), "error": float(error), "exact": want, "z": float((value - want) / error)})
        print(f"[gff correlator] E_{q} = {value:.5f} +/- {error:.5f}, exact {want:.5f}")
        assert error > 0 and abs(value - want) < 4.5 * error, rows[-1]
    _record("energies", rows)
