#!/usr/bin/env python3
"""Bit-for-bit comparison of two library builds (MLMCPI_LIB_VARIANT): SHA-256 of the states a set of draws leaves behind --
Schwinger closed-form launches of every depth, 64 x 64 and 64 x 32 tiles, GFF register-block launches on 64 x 64 and 32 x 32
tiles, with and without the heat bath and the QoI -- and, under MLMCPI_OR_KERNEL=block, the Schwinger sweep-by-sweep plan
(lines starting "block": state hashes, and the QoI values themselves, which two builds may sum in different tile orders).
   MLMCPI_LIB_VARIANT=r04 python tools/exp_variant_hash.py > a.txt; python tools/exp_variant_hash.py > b.txt
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
