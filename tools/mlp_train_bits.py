"""Bit-level fixtures of the NerfNetwork training pass (k_nerf_mlp_train, mlp.hip): one forward_backward at seeded
inputs per (config, n); the fp16 MLP gradient bits are kept whole, the network output and dL/d(encoding) as a SHA-256
of their bytes. A change to the kernel that keeps every product and every accumulation order leaves all three
unchanged bit for bit (tests/test_gpu_mlp_train_bits.py).

    python tools/mlp_train_bits.py --write --commit $(git rev-parse HEAD)     # regenerate tests/golden/mlp_train_bits/
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_train_bits")
LOG2T = 14
# n = 100: one block, a partial tile and empty tiles; 4,133: several blocks, ragged; 36,901: on a 256-CU part some
# blocks run two iterations and some one
CASES = [(cfg, n) for cfg in ("C2", "C2p") for n in (100, 4133, 36901)]
GRID = {"C2": (4, 4), "C2p": (16, 2)}  # levels, features per level


def case_name(cfg, n):
    return f"{cfg}_n{n}"


def inputs(n):
    g = np.random.default_rng(1000 + n)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = g.random((n, 3))
    c[:, 3] = 0.01
    d = g.standard_normal((n, 3))
    c[:, 4:] = (d / np.linalg.norm(d, axis=1, keepdims=True) + 1) / 2
    dL = np.zeros((n, 16), np.float16)
    dL[:, :4] = g.uniform(-1, 1, (n, 4))
    return c, dL


def run_case(pkg, cfg_name, n):
    """-> (MLP gradient bits uint16 [n_matrix], output bits uint16 [n, 16], dL/d(encoding) bits uint16 [n, L F])"""
    import torch

    cfg = pkg.nerf_config(cfg_name)
    cfg["encoding"]["log2_hashmap_size"] = LOG2T
    net = pkg.create_nerf_network(cfg)
    tr = pkg.Trainer(net, cfg["optimizer"])
    nm = net.n_matrix_params
    p = net.initialize_params(1337)
    p[nm:] = np.random.default_rng(3).uniform(-0.5, 0.5, p.size - nm).astype(np.float32)
    tr.set_params_full_precision(p)
    c, dL = inputs(n)
    out = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    net.forward_backward(torch.from_numpy(c).cuda(), torch.from_numpy(dL).cuda(), output=out)
    torch.cuda.synchronize()
    L, F = GRID[cfg_name]
    grad = tr.gradients[:nm].cpu().numpy().view(np.uint16).copy()
    denc = np.ascontiguousarray(net.workspace("dL_dencoding", n).cpu().numpy().view(np.uint16)[:, :L * F])
    return grad, out.cpu().numpy().view(np.uint16).copy(), denc


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--write", action="store_true", help="write the fixtures (default: compare against them)")
    ap.add_argument("--commit", default="unknown", help="commit the fixtures are recorded from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package

    pkg = load_package()
    manifest = {"commit": args.commit, "log2_hashmap_size": LOG2T, "cases": {}}
    old = None
    if not args.write:
        old = json.load(open(os.path.join(args.out, "manifest.json")))
    else:
        os.makedirs(args.out, exist_ok=True)
    bad = 0
    for cfg, n in CASES:
        grad, out, denc = run_case(pkg, cfg, n)
        name = case_name(cfg, n)
        rec = {"n_matrix": int(grad.size), "grad_sha256": sha(grad), "out_sha256": sha(out), "denc_sha256": sha(denc)}
        manifest["cases"][name] = rec
        if args.write:
            np.save(os.path.join(args.out, name + "_grad.npy"), grad)
            print(name, rec)
        else:
            same = rec == old["cases"][name] and np.array_equal(grad, np.load(os.path.join(args.out, name + "_grad.npy")))
            bad += not same
            print(name, "identical" if same else "DIFFERENT")
    if args.write:
        with open(os.path.join(args.out, "manifest.json"), "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
