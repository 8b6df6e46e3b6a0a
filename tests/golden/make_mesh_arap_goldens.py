"""Generate tests/golden/mesh_arap.npz by running the REFERENCE's own mesh-connectivity ARAP code on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_mesh_arap_goldens.py <path to the reference tree>

``prepare_arap_from_mesh_vertices``, ``sample_matrix_vectorized``, ``produce_edge_matrix_nfmt``, ``estimate_rotation`` and
``cal_arap_error`` (custom/threestudio-animate3d/systems/util.py) are compiled from the reference file as it lies, with the syntax-tree
neutralisation of tests/golden/make_arap_goldens.py (``.cuda()`` removed, decorators dropped).  Only data is written.

The connectivity: a triangulated 24 x 25 vertex grid (600 vertices, valence 2 to 6) whose rows are shuffled so that no row is ascending
on purpose, with hand-made rows over it: three of degree 1 and three of degree 2 (below ``arap_K`` = 3) and one hub of degree 24.  It is
stored as CSR arrays in dict order, not as a JSON file.  Recorded: the reference's padded ``nn_idx`` / ``max_idx``, one
``sample_matrix_vectorized`` draw under ``torch.manual_seed``, the (ii, jj, nn) edge list built as animate3d.py:227-234 builds it, a
5-frame trajectory on a curved sheet (frame 0 the source, frame 1 bitwise equal to it, frame 3 mirrored), the ``sample_idx`` that
``cal_arap_error`` draws from the recorded numpy seed, the reference's rotations, error and autograd gradient.  The drawn neighbours of
a drawn vertex whose rotation is ill-conditioned in some frame (tests/arap_ref.COND) are moved again until none is left, as
make_arap_goldens.py redraws its points.  Before that the numpy seed is advanced until ``sample_idx`` holds the hub and a degree-2 row
and no degree-1 row (one edge: the rotation is not unique, nothing to compare)."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import arap_ref, mesh_ref  # noqa: E402
from tests.golden.make_arap_goldens import extract  # noqa: E402

NX, NY, K, SAMPLE_NUM, SEED, TORCH_SEED, JITTER = 24, 25, 3, 256, 11, 3, 0.03
DEGREE_1, DEGREE_2, HUB, HUB_DEGREE = (37, 290, 511), (64, 333, 580), 301, 24


def connectivity():
    rng = np.random.default_rng(SEED)
    Nv = NX * NY
    rows = mesh_ref.adjacency_from_faces(mesh_ref.grid_faces(NX, NY), Nv)
    for r in rows:
        rng.shuffle(r)
        if len(r) > 1 and r == sorted(r):
            r.reverse()
    for v in DEGREE_1:
        rows[v] = rows[v][:1]
    for v in DEGREE_2:
        rows[v] = rows[v][:2]
    far = [u for u in rng.permutation(Nv).tolist() if u != HUB][:HUB_DEGREE]
    rows[HUB] = far
    return rows


def sheet(Nv, g):
    """A curved sheet with jitter in every coordinate: the neighbourhoods are not planar."""
    y, x = torch.meshgrid(torch.linspace(-0.5, 0.5, NY, dtype=torch.float64), torch.linspace(-0.5, 0.5, NX, dtype=torch.float64), indexing="ij")
    z = 0.15 * torch.sin(3.0 * x) * torch.cos(2.0 * y)
    p = torch.stack([x, y, z], -1).reshape(Nv, 3)
    return p + JITTER * torch.randn(Nv, 3, generator=g, dtype=torch.float64)


def trajectory(source):
    frames = [source, source.clone(), arap_ref.deform(source, SEED + 1), arap_ref.deform(source, SEED + 2, mirror=True),
              arap_ref.deform(source, SEED + 3, amplitude=0.05)]
    return torch.stack(frames).float()                                                   # frame 0: the source; frame 1: bitwise equal to it


def well_conditioned_sheet(draw, judged, max_rounds=200):
    """The sheet, with the drawn neighbours of every vertex of ``judged`` whose rotation is ill-conditioned in some frame moved again,
    until none is left."""
    Nv = draw.shape[0]
    g = torch.Generator().manual_seed(SEED)
    source = sheet(Nv, g)
    w64 = arap_ref.default_weight(draw, torch.float64)
    for rounds in range(1, max_rounds + 1):
        source = source.float().double()
        nodes = trajectory(source)
        cond = arap_ref.conditioning(nodes[0].double(), nodes[1:].double(), draw, w64, judged)
        bad = judged[(cond < arap_ref.COND).any(0)]
        if len(bad) == 0:
            return source, nodes, rounds, float(cond.min())
        move = torch.unique(draw[bad][draw[bad] >= 0])
        source[move] += JITTER * torch.randn(len(move), 3, generator=g, dtype=torch.float64)
    raise RuntimeError(f"{len(bad)} ill-conditioned vertices after {max_rounds} rounds")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = {"torch": torch, "np": np, "F": F, "svd": torch.svd}
    names = ("prepare_arap_from_mesh_vertices", "sample_matrix_vectorized", "produce_edge_matrix_nfmt", "estimate_rotation", "cal_arap_error")
    exec(compile(extract(os.path.join(ref, "custom", "threestudio-animate3d", "systems", "util.py"), names), "util.py", "exec"), ns)

    rows = connectivity()
    Nv = len(rows)
    info = {str(v): {str(u): 1.0 for u in r} for v, r in enumerate(rows)}
    nn_idx, max_idx = ns["prepare_arap_from_mesh_vertices"](info)
    torch.manual_seed(TORCH_SEED)
    draw = ns["sample_matrix_vectorized"](nn_idx, K, max_idx)
    ii = torch.arange(Nv)[:, None].long().expand(Nv, K).reshape([-1])                     # animate3d.py:227-234
    jj = draw.reshape([-1])
    nn = torch.arange(K)[None].long().expand(Nv, K).reshape([-1])
    mask = jj != -1
    ii, jj, nn = ii[mask], jj[mask], nn[mask]

    for np_seed in range(1000):
        np.random.seed(np_seed)
        sample_idx = torch.from_numpy(np.random.choice(Nv, SAMPLE_NUM)).long()             # the draw cal_arap_error will make from this seed
        drawn = set(sample_idx.tolist())
        if not drawn & set(DEGREE_1) and HUB in drawn and drawn & set(DEGREE_2):
            break
    else:
        raise RuntimeError("no numpy seed draws the hub and a degree-2 row without a degree-1 row")
    source, nodes, rounds, worst = well_conditioned_sheet(draw, torch.unique(sample_idx))

    leaf = nodes.clone().requires_grad_(True)
    np.random.seed(np_seed)
    err = ns["cal_arap_error"](leaf, ii, jj, nn, K=K, sample_num=SAMPLE_NUM)
    (grad,) = torch.autograd.grad(err, leaf)
    w_full = torch.zeros(Nv, K)
    w_full[ii, nn] = 1
    with torch.no_grad():
        rots = torch.stack([ns["estimate_rotation"](nodes[0], nodes[f], ii, jj, nn, K=K, weight=w_full[sample_idx], sample_idx=sample_idx)
                            for f in range(1, nodes.shape[0])])
    row_start, col = mesh_ref.csr_of(rows)
    out = {"row_start": row_start.astype(np.int32), "col": col.astype(np.int32), "nn_idx": nn_idx.numpy().astype(np.int32),
           "max_idx": max_idx.numpy(), "K": np.array(K), "torch_seed": np.array(TORCH_SEED), "draw": draw.numpy().astype(np.int32),
           "ii": ii.numpy().astype(np.int32), "jj": jj.numpy().astype(np.int32), "nn": nn.numpy().astype(np.int32), "nodes": nodes.numpy(),
           "sample_num": np.array(SAMPLE_NUM), "np_seed": np.array(np_seed), "sample_idx": sample_idx.numpy().astype(np.int32),
           "rotations": rots.numpy(), "error": err.detach().numpy(), "grad": grad.numpy()}
    path = os.path.join(HERE, "mesh_arap.npz")
    np.savez_compressed(path, **out)
    deg = np.diff(row_start)
    print(f"{Nv} vertices, degrees {deg.min()} .. {deg.max()}, {int((draw < 0).sum())} absent edges in the draw, numpy seed {np_seed}, "
          f"{rounds} rounds of moving points, worst conditioning {worst:.3f}, error {float(err.detach()):.6f}; {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
