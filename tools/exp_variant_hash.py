#!/usr/bin/env python3
"""Bit-for-bit comparison of two library builds (MLMCPI_LIB_VARIANT): SHA-256 of the states a set of draws leaves behind --
Schwinger closed-form launches of every depth, 64 x 64 and 64 x 32 tiles, GFF register-block launches on 64 x 64 and 32 x 32
tiles, with and without the heat bath and the QoI -- and, under MLMCPI_OR_KERNEL=block, the Schwinger sweep-by-sweep plan
(lines starting "block": state hashes, and the QoI values themselves, which two builds may sum in different tile orders).
Behind them the 1-D paths: HMC draws and whole-chain runs on every launch geometry, rotor sweeps with both heat-bath samplers,
the two-level step of the three actions and the exact harmonic-oscillator draw.  First of all the sigma-model cluster samplers
(lines starting "sigma"): Wolff and Swendsen-Wang, unrotated and rotated, under every forced plan, with and without their
optional outputs; `--sigma-cluster` stops after that section.
   MLMCPI_LIB_VARIANT=r04 python tools/exp_variant_hash.py > a.txt; python tools/exp_variant_hash.py > b.txt
   python tools/exp_variant_hash.py [--sigma-cluster]
   python tools/exp_variant_hash.py --compare a.txt b.txt   (other lines equal; block lines: states equal, QoI to 1e-13)"""
import hashlib, sys
import torch


def compare(fa, fb):
    la, lb = open(fa).read().splitlines(), open(fb).read().splitlines()
    bad = 0 if len(la) == len(lb) else 1
    for a, b in zip(la, lb):
        if not a.startswith("block "):
            ok = a == b
        else:   # "block <case>: <state hash> qoi <values>"
            (ka, _, qa), (kb, _, qb) = a.partition(" qoi "), b.partition(" qoi ")
            ok = ka == kb and len(qa.split()) == len(qb.split()) and all(
                abs(float(u) - float(v)) <= 1e-13 for u, v in zip(qa.split(), qb.split()))
        if not ok:
            bad += 1
            print(f"DIFFERS\n  {a}\n  {b}")
    print(f"{len(la)} lines, {bad} differ")
    return bad


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
sys.path.insert(0, ".")
from mlmcpathintegral_amd import abi, ops
abi.load()
SEED = 11


def h(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


# ---- the O(3) sigma-model cluster samplers: 10 updates of each draw on the lattice and on its rotated level, every forced plan
def sigma_cluster_section():
    wolff_plans = [(("MLMCPI_SIGMA_CLUSTER_TEAM", t), ("MLMCPI_SIGMA_CLUSTER_BITMAP", m)) for t in ("wave", "block") for m in ("global", "lds")]
    sw_plans = [(("MLMCPI_SIGMA_SW_PLAN", "chain"),), (("MLMCPI_SIGMA_SW_PLAN", "tiled"),),
                (("MLMCPI_SIGMA_SW_PLAN", "tiled"), ("MLMCPI_SIGMA_SW_TILE", "16x8"))]
    for Mt, Mx, B in ((16, 16, 3), (130, 70, 3), (512, 300, 2)):
        for rotated in (0, 1):
            lv = abi.sigma_level(Mt, Mx, rotated, 1.2)
            x0 = ops.sigma_level_initialise(lv, B, SEED)
            for name, plans, draw in (("wolff", wolff_plans, lambda x, out: ops.sigma_level_cluster_draw(lv, x, 10, SEED, 2, 7, count=out)),
                                      ("sw", sw_plans, lambda x, out: ops.sigma_level_sw_draw(lv, x, 10, SEED, 2, 7, outputs=out))):
                for plan in plans:
                    for k, v in plan:
                        abi.set_option(k, v)
                    try:
                        for out in (False, True):
                            x = x0.clone()
                            try:
                                r = draw(x, out)
                                r = () if r is None else r if isinstance(r, tuple) else (r,)
                                res = " ".join([h(x)] + [h(t) for t in r])
                            except RuntimeError as e:   # the chain plan forced beyond its bound, and nothing else
                                if "MLMCPI_SIGMA_SW_PLAN=chain holds a chain of at most" not in str(e):
                                    raise
                                res = "refused"
                            print(f"sigma {name} {Mt}x{Mx} rotated={rotated} {' '.join(v for _, v in plan)} outputs={out}: {res}", flush=True)
                    finally:
                        for k, _ in plan:
                            abi.set_option(k, "")


if "--sigma-cluster" in sys.argv[1:]:   # this section alone
    sigma_cluster_section()
    sys.exit(0)


for Mt, Mx, B, beta in ((128, 128, 3, 1.0), (192, 128, 2, 1.0), (256, 192, 2, 0.7), (192, 96, 2, 1.0), (64, 64, 2, 1.0), (128, 128, 2, 3.0), (1024, 1024, 2, 1.0)):
    act = abi.lattice_action(abi.SCHWINGER, Mt, Mx, beta=beta)
    x0 = ops.lattice_initialise(act, B, SEED, 0)
    for n_or, n_hb in ((1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (13, 0), (23, 0), (1, 1), (4, 1), (6, 1), (7, 1), (9, 1), (10, 1), (10, 2)):
        x = x0.clone()
        ops.lattice_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, 0, 5)
        line = f"{Mt}x{Mx} B={B} beta={beta} ({n_or},{n_hb}): {h(x)}"
        if n_hb:
            a, w, q = ops.lattice_sweep_draw_qoi(act, x0.clone(), torch.empty_like(x0), torch.empty_like(x0), n_or, n_hb, SEED, 0, 5, 1)
            line += f" qoi {h(a)} {h(q)}"
        print(line, flush=True)

for M, B in ((64, 2), (96, 2), (128, 3), (130, 2), (160, 2), (512, 2)):
    act = abi.lattice_action(abi.GFF, M, M, mass=3.0)
    x0 = ops.lattice_initialise(act, B, SEED, 0)
    for n_or, n_hb in ((1, 0), (3, 0), (5, 0), (6, 0), (10, 0), (13, 0), (1, 1), (4, 1), (5, 1), (6, 1), (10, 1), (10, 2)):
        x = x0.clone()
        ops.lattice_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, 0, 5)
        line = f"gff {M}x{M} B={B} ({n_or},{n_hb}): {h(x)}"
        if n_hb:
            a, w, q = ops.lattice_sweep_draw_qoi(act, x0.clone(), torch.empty_like(x0), torch.empty_like(x0), n_or, n_hb, SEED, 0, 5, 3)
            line += f" qoi {h(a)} {h(q)}"
        print(line, flush=True)

abi.set_option("MLMCPI_OR_KERNEL", "block")
try:
    for Mt, Mx, B, beta in ((128, 128, 1, 1.0), (128, 128, 2, 1.0), (256, 192, 2, 0.7), (192, 96, 2, 1.0), (128, 128, 2, 10.0), (1024, 1024, 1, 1.0)):
        act = abi.lattice_action(abi.SCHWINGER, Mt, Mx, beta=beta)
        x0 = ops.lattice_initialise(act, B, SEED, 0)
        for n_or, n_hb in ((3, 0), (13, 0), (1, 1), (4, 1), (5, 1), (6, 1), (8, 1), (10, 1), (10, 2)):
            x = x0.clone()
            ops.lattice_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, 0, 5)
            line = f"block {Mt}x{Mx} B={B} beta={beta} ({n_or},{n_hb}): {h(x)}"
            if n_hb:
                a, w, q = ops.lattice_sweep_draw_qoi(act, x0.clone(), torch.empty_like(x0), torch.empty_like(x0), n_or, n_hb, SEED, 0, 5, 1)
                line += f" {h(a)} qoi " + " ".join(f"{v:.17g}" for v in q.cpu().numpy())
            print(line, flush=True)
finally:
    abi.set_option("MLMCPI_OR_KERNEL", "")

# ---- the 1-D paths: HMC draws and whole-chain runs, rotor sweeps, the two-level step, the exact HO draw
def path_act(name, M, m0=None):
    if name == "rotor":
        return abi.path_action(2, M, M / 8.0, 0.25 if m0 is None else m0)
    return abi.path_action(0 if name == "harmonic" else 1, M, M / 8.0, 1.0, 1.0, 0.0 if name == "harmonic" else 1.0,
                           0.0 if name == "harmonic" else 1.0)


def path_start(M, B):
    g = torch.Generator().manual_seed(M + B)
    return (torch.rand((B, M), generator=g, dtype=torch.float64) * 2 - 1).cuda()


for name, M, B, nt, dt in (("harmonic", 128, 4, 20, 0.05), ("quartic", 1000, 2, 12, 0.08), ("quartic", 1024, 2100, 6, 0.34),
                           ("rotor", 512, 2100, 6, 0.45), ("rotor", 65536, 2, 6, 0.05)):
    act, x = path_act(name, M), path_start(M, B)
    hmc = ops.PathHMC(act, B, nt, dt, n_rep=2, seed=SEED, chain0=3)
    for d in range(3):
        acc = hmc.draw(x)
        print(f"hmc_draw {name} M={M} B={B} draw {d}: {h(x)} {h(acc)} {h(hmc.energies)}", flush=True)
    for qoi_kind in (1, 2):
        x = path_start(M, B)
        run = ops.PathHMC(act, B, nt, dt, n_rep=2, seed=SEED, chain0=3)
        q, cnt = ops.path_hmc_run(run, x, 3, qoi_kind)
        print(f"hmc_run {name} M={M} B={B} qoi {qoi_kind}: {h(x)} {h(q)} {h(cnt)}", flush=True)

for m0 in (0.25, 2.0):   # 2 m0 / a = 4 and 32: step envelope and wrapped Cauchy (kVsKappaMax = 16)
    for M in (64, 4096, 10000):
        act, x0 = path_act("rotor", M, m0), path_start(M, 3) * 3.0
        for n_or, n_hb in ((10, 1), (3, 0), (0, 2)):
            x = x0.clone()
            ops.path_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, 0, 5)
            a, w, q = ops.path_sweep_draw_qoi(act, x0.clone(), torch.empty_like(x0), torch.empty_like(x0), n_or, n_hb, SEED, 0, 5)
            print(f"rotor_sweep M={M} m0={m0} ({n_or},{n_hb}): {h(x)} qoi {h(a)} {h(q)}", flush=True)

for name in ("harmonic", "quartic", "rotor"):
    for M in (64, 4096):
        fine, coarse = path_act(name, M), path_act(name, M // 2)
        coarse.T_final = fine.T_final
        step = ops.PathTwoLevelStep(fine, coarse, 3, seed=SEED, chain0=1)
        step.set_state(path_start(M, 3))
        xc = path_start(M // 2, 3)
        for d in range(2):
            acc = step.draw(xc)
            print(f"twolevel {name} M={M} step {d}: {h(step.theta)} {h(acc)} {h(step.terms)}", flush=True)

print(f"ho_exact M=128 B=32: {h(ops.HOExactSampler(path_act('harmonic', 128), 32, seed=SEED, chain0=2).draw())}", flush=True)

sigma_cluster_section()
