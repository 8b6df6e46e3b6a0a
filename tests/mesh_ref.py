"""Host restatement of the mesh branch's neighbour sampler (csrc/arap.hip, mesh_sample_kernel; specified in include/animate3d_hip.h), in
numpy: the same generator (Philox4x32-10, key = the seed's two 32-bit halves, counter (v, p / 4, 0, 0), word p % 4) and the same integer
acceptance rule, so the kernel's output is reproduced bit for bit.  Vectorised over the vertices, one pass per row position.  Beside it:
brute-force vertex adjacency from faces with Python sets, the subset index the uniformity tests count over, and the graphs the CPU and
GPU tests share."""
from itertools import combinations

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed, c0, c1):
    """The four 32-bit words (uint64 arrays holding 32-bit values) of the block with key (seed lo, seed hi) and counter (c0, c1, 0, 0)."""
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c = [np.asarray(c0, dtype=np.uint64) & MASK, np.asarray(c1, dtype=np.uint64) & MASK]
    c += [np.zeros_like(c[0]), np.zeros_like(c[0])]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def sample(row_start, col, K, seed):
    """nn_idx [Nv, K] int32: position p of row v is kept iff mulhi32(r_p, d - p) < K - kept; the row ends at kept = K; then -1."""
    row_start, col = np.asarray(row_start, dtype=np.int64), np.asarray(col, dtype=np.int64)
    Nv = len(row_start) - 1
    deg = row_start[1:] - row_start[:-1]
    v = np.arange(Nv, dtype=np.uint64)
    out = np.full((Nv, K), -1, dtype=np.int32)
    kept = np.zeros(Nv, dtype=np.int64)
    for p in range(int(deg.max()) if Nv else 0):
        if p % 4 == 0:
            block = philox4x32_10(seed, v, np.full(Nv, p // 4, dtype=np.uint64))
        left = np.maximum(deg - p, 0).astype(np.uint64)
        hi = ((block[p % 4] * left) >> np.uint64(32)).astype(np.int64)
        take = (p < deg) & (kept < K) & (hi < K - kept)
        rows = np.nonzero(take)[0]
        out[rows, kept[rows]] = col[row_start[rows] + p]
        kept[rows] += 1
    return out


def positions(row_start, col, nn_idx):
    """[Nv, K]: the row position of every sampled entry (-1 for -1), for rows without duplicates; -2 where an entry is no neighbour."""
    row_start, col, nn_idx = (np.asarray(a, dtype=np.int64) for a in (row_start, col, nn_idx))
    pos = np.full(nn_idx.shape, -2, dtype=np.int64)
    pos[nn_idx == -1] = -1
    deg = row_start[1:] - row_start[:-1]
    for p in range(int(deg.max())):
        live = p < deg
        here = np.full(len(deg), -3, dtype=np.int64)
        here[live] = col[row_start[:-1][live] + p]
        pos[(nn_idx == here[:, None]) & (pos == -2)] = p
    return pos


def check_invariants(row_start, col, nn_idx, K):
    """The sampling contract, from the output alone (rows without duplicates): every entry is a neighbour of its row, entries are
    distinct, there are min(K, d) of them, -1 comes only at the tail, and the entries are in ascending row position."""
    row_start = np.asarray(row_start, dtype=np.int64)
    deg = row_start[1:] - row_start[:-1]
    nn_idx = np.asarray(nn_idx)
    assert nn_idx.shape == (len(deg), K)
    pos = positions(row_start, col, nn_idx)
    assert (pos != -2).all(), "an entry that is no neighbour of its row"
    count = (pos >= 0).sum(1)
    assert np.array_equal(count, np.minimum(K, deg)), "a row does not hold min(K, d) entries"
    slot = np.arange(K)[None]
    assert ((pos >= 0) == (slot < count[:, None])).all(), "-1 before the tail"
    asc = (pos[:, 1:] > pos[:, :-1]) | (pos[:, 1:] < 0)
    assert asc.all(), "entries not distinct or not in ascending row position"


def adjacency_from_faces(faces, Nv):
    """[sorted neighbour list per vertex] by brute force: sets, both directions, no self-edge."""
    nbr = [set() for _ in range(Nv)]
    for tri in np.asarray(faces).tolist():
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if a != b:
                nbr[a].add(b)
                nbr[b].add(a)
    return [sorted(s) for s in nbr]


def grid_faces(nx, ny):
    """The triangles of an nx x ny vertex grid, each quad cut along one diagonal: [2 (nx - 1)(ny - 1), 3], vertex = y * nx + x."""
    y, x = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    a = (y * nx + x).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)]).astype(np.int64)


def csr_of(rows):
    """(row_start [Nv + 1], col [E]) int64 of a list of neighbour lists."""
    deg = np.array([len(r) for r in rows], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), np.array([u for r in rows for u in r], dtype=np.int64)


def padded_of(rows):
    """The reference's dense form of a list of neighbour lists: [Nv, Dmax] int64, -1 padded at the tail."""
    D = max(len(r) for r in rows)
    return np.array([list(r) + [-1] * (D - len(r)) for r in rows], dtype=np.int64).reshape(len(rows), D)


def ring_rows(Nv, d):
    """Every vertex v has the d neighbours v + 1 .. v + d (mod Nv): one seed gives Nv independent draws from equal rows."""
    return [[(v + 1 + j) % Nv for j in range(d)] for v in range(Nv)]


ZOO_DEGREES = (0, 1, 2, 3, 4, 7, 16, 17, 40)


def zoo_rows(Nv=1000, seed=5):
    """Nv rows whose degrees cycle through ZOO_DEGREES in shuffled order, each a random set of other vertices in random (not ascending) order."""
    rng = np.random.default_rng(seed)
    deg = np.array([ZOO_DEGREES[i % len(ZOO_DEGREES)] for i in range(Nv)])
    rng.shuffle(deg)
    rows = []
    for v in range(Nv):
        r = rng.choice(Nv - 1, size=int(deg[v]), replace=False)
        rows.append([int(u) + (int(u) >= v) for u in r])                       # never v itself; rng.choice's order is random
    return rows


def subset_index(d, K):
    """{K-tuple of ascending positions: its index among the C(d, K) subsets}."""
    return {c: i for i, c in enumerate(combinations(range(d), K))}
