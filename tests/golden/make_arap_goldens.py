"""Generate tests/golden/arap.npz by running the REFERENCE's own ARAP code on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_arap_goldens.py <path to the reference tree>

``cal_connectivity_from_points``, ``produce_edge_matrix_nfmt``, ``estimate_rotation`` and ``cal_arap_error``
(custom/threestudio-animate3d/systems/util.py) are compiled from the reference file as it lies; the module imports pytorch3d and scipy at
its top, so only these definitions are executed.  pytorch3d is not installed: ``pytorch3d.ops.knn_points`` / ``knn_gather`` are STUBBED by a
brute-force search (tests/arap_ref.knn_bruteforce in float32, the query itself first at distance 0, as knn_points returns it) and plain
indexing.  The ``.cuda()`` calls are removed and the ``device="cuda"`` default becomes "cpu" in the syntax tree; the autocast decorator of
``estimate_rotation`` is dropped.  ``np.random.choice`` is seeded, and the draw is recorded by making it from the same seed beforehand; the points
are drawn until every drawn vertex has a well-conditioned rotation in every frame (tests/arap_ref.COND, through ``make_points``).
Only data is written: inputs, ii / jj / nn / weight, sample_idx, rotations, the error and its autograd gradient."""
import ast
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import arap_ref  # noqa: E402

NV, SAMPLE_NUM, SEED, NP_SEED = 3000, 512, 7, 0
CASES = {"k3": dict(K=3, radius=0.01, wobble=False), "k8": dict(K=8, radius=0.085, wobble=True)}   # wobble: a second frame for util.py:80-84


class Neutralise(ast.NodeTransformer):
    def visit_Call(self, node):
        self.generic_visit(node)
        if isinstance(node.func, ast.Attribute) and node.func.attr == "cuda" and not node.args and not node.keywords:
            return node.func.value
        return node

    def visit_FunctionDef(self, node):
        self.generic_visit(node)
        node.decorator_list = []
        node.args.defaults = [ast.Constant("cpu") if isinstance(d, ast.Constant) and d.value == "cuda" else d for d in node.args.defaults]
        return node


def extract(path, names):
    tree = ast.parse(open(path).read())
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names}
    assert not set(names) - set(found), set(names) - set(found)
    mod = ast.Module(body=[Neutralise().visit(found[n]) for n in names], type_ignores=[])
    return ast.fix_missing_locations(mod)


def knn_points(p1, p2, lengths1, lengths2, K):
    assert p1.shape[0] == 1 and p1 is not None and torch.equal(p1, p2)
    idx, dist = arap_ref.knn_bruteforce(p1[0], K - 1)
    n = p1.shape[1]
    idx = torch.cat([torch.arange(n)[:, None], idx], dim=1)
    dist = torch.cat([torch.zeros(n, 1, dtype=dist.dtype), dist], dim=1)
    return types.SimpleNamespace(dists=dist[None], idx=idx[None])


def knn_gather(x, idx):
    return torch.stack([x[b][idx[b]] for b in range(x.shape[0])])


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    p3d = types.SimpleNamespace(ops=types.SimpleNamespace(knn_points=knn_points, knn_gather=knn_gather))
    ns = {"torch": torch, "np": np, "F": F, "svd": torch.svd, "pytorch3d": p3d}
    names = ("produce_edge_matrix_nfmt", "cal_connectivity_from_points", "estimate_rotation", "cal_arap_error")
    exec(compile(extract(os.path.join(ref, "custom", "threestudio-animate3d", "systems", "util.py"), names), "util.py", "exec"), ns)

    np.random.seed(NP_SEED)
    sample_idx = torch.from_numpy(np.random.choice(NV, SAMPLE_NUM)).long()             # the draw cal_arap_error will make from this seed

    def scene(source):
        frames = [source, source.clone(), arap_ref.deform(source, SEED + 1), arap_ref.deform(source, SEED + 2, mirror=True),
                  arap_ref.deform(source, SEED + 3, amplitude=0.05)]
        frames[4][:, 1] = source[:, 1]                                                # one axis copied from the source
        nodes = torch.stack(frames).float()                                          # frame 0: the source; frame 1: bitwise equal to it
        graphs = {}
        for tag, c in CASES.items():
            points = nodes[0:1].clone()
            if c["wobble"]:                                                           # a slightly moved copy: the multi-frame radius test cuts some edges
                moved = arap_ref.deform(source, SEED + 9, amplitude=0.02) - arap_ref.deform(source, SEED + 9, amplitude=0.0)
                points = torch.cat([points, (source + 0.3 * moved).float()[None]])
            ii, jj, nn, weight = ns["cal_connectivity_from_points"](points.clone(), radius=c["radius"], K=c["K"])
            dense = torch.full((NV, c["K"]), -1, dtype=torch.long)
            dense[ii, nn] = jj
            variants = [("unit", None)] + ([("weighted", weight)] if bool(torch.isfinite(weight).all()) else [])
            graphs[tag] = (points, ii, jj, nn, weight, dense, variants)
        return nodes, graphs

    def ill_conditioned(source):                                                      # drawn vertices whose rotation is ill-conditioned in some frame
        nodes, graphs = scene(source)
        bad = torch.zeros(NV, dtype=torch.bool)
        for points, ii, jj, nn, weight, dense, variants in graphs.values():
            for _, w in variants:
                w64 = arap_ref.default_weight(dense, torch.float64) if w is None else w.double()
                cond = arap_ref.conditioning(nodes[0].double(), nodes[1:].double(), dense, w64, sample_idx)
                bad[sample_idx[(cond < arap_ref.COND).any(0)]] = True
        return bad

    source, rounds, _, _ = arap_ref.make_points(NV, 10, SEED, radius=CASES["k8"]["radius"], duplicates=0,
                                                extra_bad=ill_conditioned)
    nodes, graphs = scene(source)
    out = {"nodes": nodes.numpy(), "sample_num": np.array(SAMPLE_NUM), "np_seed": np.array(NP_SEED),
           "sample_idx": sample_idx.numpy().astype(np.int32)}
    zero = ns["estimate_rotation"](nodes[0], nodes[1], *[torch.zeros(1, dtype=torch.long)] * 3, K=1, weight=torch.ones(4, 1),
                                   sample_idx=torch.arange(4))
    out["rotation_of_zero_S"] = zero.numpy()                                          # what the reference's SVD gives for S = 0
    for tag, (points, ii, jj, nn, weight, dense, variants) in graphs.items():
        K = CASES[tag]["K"]
        out[f"{tag}_points"] = points.numpy()
        out[f"{tag}_K"], out[f"{tag}_radius"] = np.array(K), np.array(CASES[tag]["radius"])
        out[f"{tag}_ii"], out[f"{tag}_jj"], out[f"{tag}_nn"] = (t.numpy().astype(np.int32) for t in (ii, jj, nn))
        out[f"{tag}_weight"] = weight.numpy()
        for vname, w in variants:
            leaf = nodes.clone().requires_grad_(True)
            np.random.seed(NP_SEED)
            err = ns["cal_arap_error"](leaf, ii, jj, nn, K=K, weight=w, sample_num=SAMPLE_NUM)
            (grad,) = torch.autograd.grad(err, leaf)
            w_full = torch.zeros(NV, K)
            w_full[ii, nn] = 1
            w_s = (w_full if w is None else w)[sample_idx]
            with torch.no_grad():
                rots = torch.stack([ns["estimate_rotation"](nodes[0], nodes[f], ii, jj, nn, K=K, weight=w_s, sample_idx=sample_idx)
                                    for f in range(1, nodes.shape[0])])
            out[f"{tag}_{vname}_error"], out[f"{tag}_{vname}_grad"], out[f"{tag}_{vname}_rotations"] = (err.detach().numpy(), grad.numpy(),
                                                                                                       rots.numpy())
            print(tag, vname, "error", float(err.detach()), "absent edges", int((dense < 0).sum()), "rounds", rounds)
    path = os.path.join(HERE, "arap.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes; zero-S rotation:\n", out["rotation_of_zero_S"][0])


if __name__ == "__main__":
    main()
