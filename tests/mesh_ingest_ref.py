"""Host restatement of the mesh ingest (animate3d_amd/mesh.py, csrc/mesh_ingest.hip) in float64 numpy, the meshes the CPU and GPU tests
share, and the derived error bars of the kernel's outputs against that restatement.

The restatement evaluates the contract's formulas in float64 on the fp32 inputs as they are: adjacency by brute force with Python sets
(tests/mesh_ref.py), its own bilinear sampler (checked against ``F.grid_sample`` in float64 by tests/test_mesh_ingest_host.py), plain
means.  Nothing here imports the code under test.

Bars, with u = 2^-24 (the unit roundoff of fp32), d a row's degree and c a vertex's corner count; each is against float64 on the same
fp32 inputs:

* ``edge_length``: 6 u relative (three subtractions, three squares, two additions, one square root, all correctly rounded).
* ``mean_edge``: (d + 4) u relative (d non-negative terms with one rounding each, d - 1 additions, one division).
* ``xyz``: 8 u scale_factor (|x| + |y| + |z|).
* ``scaling``: the relative bar of the logarithm's argument, (d + 4) u, taken as absolute (d log a = d a / a), plus 4 ulp of the result.
* ``colors``: (c + 1) u absolute for colours in [0, 1]; with a texture plus 4 e32, where e32 is the error of torch's float32
  ``grid_sample`` against its float64 one on the same inputs.
* ``shs``: the colour bar / C0 + 2 u |value|.
* against the reference's golden the same plus u relative: its values went through a float32 file."""
import numpy as np

from tests import mesh_ref

U = 2.0 ** -24
C0 = 0.28209479177387814
NX, NY, FAN, SEED, JITTER = 24, 25, 70, 23, 0.03
TEX_H, TEX_W = 5, 3
SEAM_VERTEX = 301
ROT_X, ROT_Z, SCALE, SHRINK, OPACITY = 90.0, 90.0, 0.76, 1.1, 1 - 1e-5          # the released mesh-animation config's load_ply_cfg


def frame(rot_x_degree, rot_z_degree):
    tx, tz = np.deg2rad(rot_x_degree), np.deg2rad(rot_z_degree)
    rx = np.array([[1, 0, 0], [0, np.cos(tx), -np.sin(tx)], [0, np.sin(tx), np.cos(tx)]])
    rz = np.array([[np.cos(tz), -np.sin(tz), 0], [np.sin(tz), np.cos(tz), 0], [0, 0, 1]])
    return rz @ rx


def golden_mesh():
    """The golden's mesh: the 24 x 25 jittered curved sheet (valence 2 to 6), a closed fan whose hub (vertex 600) has degree 70 over the
    rim 601 .. 670, one duplicated face, and a UV seam: vertex 301 has a second UV in every other face it is in.  The sheet's UVs are
    its grid coordinates (0 and 1 exactly on the border), the fan's reach outside [0, 1].  Returns float32 / int64 arrays."""
    rng = np.random.default_rng(SEED)
    y, x = np.meshgrid(np.linspace(-0.5, 0.5, NY), np.linspace(-0.5, 0.5, NX), indexing="ij")
    z = 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y)
    sheet = np.stack([x, y, z], -1).reshape(-1, 3) + JITTER * rng.standard_normal((NX * NY, 3))
    n0 = NX * NY
    ang = 2 * np.pi * np.arange(FAN) / FAN
    rim = np.stack([2.0 + 0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.05 * np.sin(5 * ang)], -1) + 0.01 * rng.standard_normal((FAN, 3))
    verts = np.concatenate([sheet, [[2.0, 0.0, 0.2]], rim]).astype(np.float32)
    fan = np.stack([np.full(FAN, n0), n0 + 1 + np.arange(FAN), n0 + 1 + (np.arange(FAN) + 1) % FAN], 1)
    faces = np.concatenate([mesh_ref.grid_faces(NX, NY), fan]).astype(np.int64)
    faces = np.concatenate([faces, faces[10:11]])                                              # a duplicated face
    uv_sheet = np.stack([np.tile(np.arange(NX) / (NX - 1), NY), np.repeat(np.arange(NY) / (NY - 1), NX)], -1)
    uv_fan = np.concatenate([[[0.5, 0.5]], np.stack([0.5 + 0.7 * np.cos(ang), 0.5 + 0.7 * np.sin(ang)], -1)])
    uvs = np.concatenate([uv_sheet, uv_fan, [[0.83, 0.21]]]).astype(np.float32)                 # the last: the seam's second UV
    faces_uvs = faces.copy()
    seam = np.nonzero((faces == SEAM_VERTEX).any(1))[0][::2]
    for f in seam:
        faces_uvs[f][faces[f] == SEAM_VERTEX] = len(uvs) - 1
    texture = rng.random((TEX_H, TEX_W, 3)).astype(np.float32)
    return dict(verts=verts, faces=faces, uvs=uvs, faces_uvs=faces_uvs, texture=texture)


def tetrahedron():
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.3, 0.2, 0.8]], dtype=np.float32)
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int64)
    return verts, faces


def flat_grid():
    """An axis-aligned 3 x 3 grid in the plane z = 0.25 with power-of-two spacings: every quantity is exact in fp32, and every vertex's
    neighbours coincide with it in z (a zero mean edge and a -inf log-scale on that axis)."""
    y, x = np.meshgrid(np.arange(3) * 0.5, np.arange(3) * 0.25, indexing="ij")
    verts = np.stack([x, y, np.full_like(x, 0.25)], -1).reshape(-1, 3).astype(np.float32)
    return verts, mesh_ref.grid_faces(3, 3)


def sample_texture(texture, uv):
    """``F.grid_sample(flip(texture, rows), uv * 2 - 1, bilinear, border, align_corners=True)`` at ``uv [..., 2]``, in float64."""
    tex = np.asarray(texture, dtype=np.float64)[::-1]
    H, W = tex.shape[:2]
    uv = np.asarray(uv, dtype=np.float64)
    x, y = np.clip(uv[..., 0] * (W - 1), 0, W - 1), np.clip(uv[..., 1] * (H - 1), 0, H - 1)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = (x - x0)[..., None], (y - y0)[..., None]
    return (tex[y0, x0] * (1 - wx) + tex[y0, x1] * wx) * (1 - wy) + (tex[y1, x0] * (1 - wx) + tex[y1, x1] * wx) * wy


def restate(verts, faces, *, vertex_colors=None, corner_colors=None, texture=None, uvs=None, faces_uvs=None, rot_x_degree=0.0,
            rot_z_degree=0.0, scale_factor=1.0, shrink=1.1):
    """Every output of ``gaussians_from_mesh`` in float64, plus ``rows`` (sorted neighbour lists), ``row_start``, ``col``, ``degree [Nv]``
    and ``corners [Nv]`` (corner counts)."""
    x = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    Nv = x.shape[0]
    rows = mesh_ref.adjacency_from_faces(faces, Nv)
    row_start, col = mesh_ref.csr_of(rows)
    src = np.repeat(np.arange(Nv), np.diff(row_start))
    delta = x[col] - x[src]
    edge_length = np.sqrt((delta ** 2).sum(1))
    degree = np.diff(row_start)
    mean_edge = np.zeros((Nv, 3))
    np.add.at(mean_edge, src, np.abs(delta))
    mean_edge /= np.maximum(degree, 1)[:, None]
    corners = np.bincount(faces.reshape(-1), minlength=Nv)
    if vertex_colors is not None:
        colors = np.asarray(vertex_colors, dtype=np.float64)
    else:
        per_corner = (np.asarray(corner_colors, dtype=np.float64) if corner_colors is not None
                      else sample_texture(texture, np.asarray(uvs, dtype=np.float64)[np.asarray(faces_uvs)])).reshape(-1, 3)
        colors = np.zeros((Nv, 3))
        np.add.at(colors, faces.reshape(-1), per_corner)
        colors /= np.maximum(corners, 1)[:, None]
    R = frame(rot_x_degree, rot_z_degree)
    with np.errstate(divide="ignore"):
        scaling = np.log(mean_edge / shrink * scale_factor)
    return dict(rows=rows, row_start=row_start, col=col, degree=degree, corners=corners, edge_length=edge_length, mean_edge=mean_edge,
                colors=colors, xyz=scale_factor * (x @ R.T), scaling=scaling, shs=(colors - 0.5) / C0, R=R)


def ulp32(values):
    """The spacing of fp32 numbers at |values| (of the normal range)."""
    a = np.abs(np.asarray(values, dtype=np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 23)


def bars(ref, verts, *, scale_factor, textured_e32=None, golden=False):
    """{quantity: the absolute bar per element} from the module docstring, for the restatement ``ref`` of the fp32 inputs ``verts``."""
    extra = U if golden else 0.0
    src = np.repeat(np.arange(len(ref["degree"])), ref["degree"])
    d, c = ref["degree"][:, None].astype(np.float64), ref["corners"][:, None].astype(np.float64)
    finite = np.isfinite(ref["scaling"])
    color = (c + 1) * U + (0.0 if textured_e32 is None else 4.0 * textured_e32) + extra * np.abs(ref["colors"])
    return {"edge_length": (6 * U + extra) * ref["edge_length"],
            "mean_edge": ((d + 4) * U + extra) * ref["mean_edge"],
            "xyz": 8 * U * scale_factor * np.abs(np.asarray(verts, dtype=np.float64)).sum(1, keepdims=True) + extra * np.abs(ref["xyz"]),
            "scaling": np.where(finite, (d + 4) * U + 4 * ulp32(np.where(finite, ref["scaling"], 1.0)) + extra * np.abs(np.where(finite, ref["scaling"], 0.0)), 0.0),
            "colors": color * np.ones_like(ref["colors"]),
            "shs": color / C0 + (2 * U + extra) * np.abs(ref["shs"]),
            "_src": src}


def worst(got, want, bar):
    """(largest error / bar over the elements with a non-zero bar, whether every element with a zero bar is equal)."""
    got, want, bar = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.broadcast_to(bar, np.shape(want))
    with np.errstate(invalid="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want))                                   # equal infinities: no error
    live = bar > 0
    ratio = float((err[live] / bar[live]).max()) if live.any() else 0.0
    return ratio, bool(np.array_equal(got[~live], want[~live]))


def write_ply(path, names, table, ascii=False):
    """A PLY with one ``vertex`` element of float properties ``names`` and the rows of ``table [N, len(names)]``."""
    table = np.asarray(table)
    header = f"ply\nformat {'ascii' if ascii else 'binary_little_endian'} 1.0\ncomment a test file\nelement vertex {len(table)}\n"
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        if ascii:
            f.write("".join(" ".join(repr(float(np.float32(v))) for v in row) + "\n" for row in table).encode("ascii"))
        else:
            f.write(table.astype("<f4").tobytes())


def rotation_matrices(q):
    """[N, 3, 3] of quaternions [N, 4] (w first), normalised, in float64."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
