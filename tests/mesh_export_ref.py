"""Host side of the mesh-export tests (animate3d_amd/mesh_export.py, csrc/mesh_export.hip): the float64 numpy restatement of the vertex
normals, the conditioning number q of a vertex's sum, a minimal GLB reader, and the meshes the CPU and GPU tests share.  Nothing here
imports the code under test.

The restatement walks every vertex's corners in ascending corner order (descending on request), adds ``u x w`` of the two edges leaving
the corner in float64 on the fp32 positions as they are, normalises in float64, and writes ``(0, 0, 1)`` where the squared length of the
sum is not > 0 or not finite: the contract of a3d_mesh_vertex_normals_f32.

``q(v) = |sum u x w| / sum |u| |w|`` measures how much of the summed magnitude survives the sum.  Every term is computed in float64 from
exact fp32 differences with a relative error of a few 2^-53, so the direction of the sum carries a relative error of at most about
``c 2^-52 / q`` for c corners: with ``q >= 1/64`` and c <= 64 that is below 1e-11, two float64 evaluations (another summation order,
a contracted product) then round to equal or adjacent fp32 values, and adjacent fp32 values of magnitude <= 1 are at most 2^-24 apart.
That is the GPU tests' bar; a mesh that misses the precondition is changed, never the bar."""
import json
import struct

import numpy as np

from tests import mesh_ref

U = 2.0 ** -24
Q_MIN = 1.0 / 64.0
COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}
DTYPES = {5126: "<f4", 5125: "<u4", 5123: "<u2", 5121: "u1"}


# ---- the restatement

def normals_f64(positions, faces, descending=False):
    """positions [T, Nv, 3] (any float dtype, read as they are), faces [F, 3] -> (normals [T, Nv, 3] float64, q [T, Nv])."""
    P = np.asarray(positions).astype(np.float64)
    flat = np.asarray(faces).reshape(-1).astype(np.int64)
    T, Nv = P.shape[:2]
    corners = [[] for _ in range(Nv)]
    for c, v in enumerate(flat.tolist()):
        corners[v].append(c)
    out, q = np.zeros((T, Nv, 3)), np.zeros((T, Nv))
    for v in range(Nv):
        s, mag = np.zeros((T, 3)), np.zeros(T)
        for c in (reversed(corners[v]) if descending else corners[v]):
            f, k = divmod(c, 3)
            a, b, d = flat[c], flat[3 * f + (k + 1) % 3], flat[3 * f + (k + 2) % 3]
            u, w = P[:, b] - P[:, a], P[:, d] - P[:, a]
            s[:, 0] += u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
            s[:, 1] += u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
            s[:, 2] += u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
            mag += np.sqrt((u * u).sum(1)) * np.sqrt((w * w).sum(1))
        len2 = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]
        sound = (len2 > 0) & np.isfinite(len2)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, v] = np.where(sound[:, None], s / np.sqrt(len2)[:, None], np.array([0.0, 0.0, 1.0]))
            q[:, v] = np.where(mag > 0, np.sqrt(len2) / mag, 0.0)
    return out, q


# ---- meshes (float64 positions / int64 faces; the tests cast)

def regular_tetrahedron():
    """Centred at the origin, faces wound outwards: by symmetry every vertex normal is the normalised vertex position."""
    verts = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)
    return verts, faces


def sphere(bands=9, meridians=64):
    """A latitude / longitude unit sphere: vertex 0 the north pole, ``bands - 1`` rings of ``meridians`` vertices, the south pole last;
    2 meridians triangles at the poles (each of degree ``meridians``) and 2 per quad between rings, wound outwards.  9 x 64: 514 vertices
    (2 x 256 + 2: every block size up to 256 is crossed) and 1 024 faces."""
    rings = bands - 1
    theta = np.pi * np.arange(1, bands) / bands
    phi = 2 * np.pi * np.arange(meridians) / meridians
    ring = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None], np.sin(theta)[:, None] * np.sin(phi)[None],
                     np.repeat(np.cos(theta)[:, None], meridians, 1)], -1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    south = 1 + rings * meridians
    j = np.arange(meridians)
    jn = (j + 1) % meridians
    faces = [np.stack([np.zeros_like(j), 1 + j, 1 + jn], 1)]
    for r in range(rings - 1):
        a, b = 1 + r * meridians, 1 + (r + 1) * meridians
        faces += [np.stack([a + j, b + j, b + jn], 1), np.stack([a + j, b + jn, a + jn], 1)]
    last = 1 + (rings - 1) * meridians
    faces.append(np.stack([np.full_like(j, south), last + jn, last + j], 1))
    return verts, np.concatenate(faces).astype(np.int64)


def sphere_trajectory(frames=4):
    """The sphere, deformed and jittered: ``v (1 + 0.15 sin(3 v[:, (1, 2, 0)] + t)) + 0.02 N(0, 1)`` for t = 0 .. frames - 1 from
    ``default_rng(0)``, cast to fp32.  Returns (positions [frames, 514, 3] float32, faces)."""
    v, faces = sphere()
    rng = np.random.default_rng(0)
    pos = np.stack([v * (1 + 0.15 * np.sin(3 * v[:, (1, 2, 0)] + t)) + 0.02 * rng.standard_normal(v.shape) for t in range(frames)])
    return pos.astype(np.float32), faces


def strip(frames=2):
    """An open 3 x 40 vertex strip, bent and jittered: boundary vertices with one and with two corners, interior ones with six."""
    faces = mesh_ref.grid_faces(3, 40)
    y, x = np.meshgrid(np.arange(40) * 0.1, np.arange(3) * 0.1, indexing="ij")
    rng = np.random.default_rng(3)
    base = np.stack([x, y, 0.2 * np.sin(2.0 * y)], -1).reshape(-1, 3)
    pos = np.stack([base + [0.0, 0.0, 0.05 * t] * np.cos(3.0 * base[:, 1:2]) + 0.01 * rng.standard_normal(base.shape) for t in range(frames)])
    return pos.astype(np.float32), faces


def with_tetrahedron_first(positions, faces):
    """The regular tetrahedron (scaled to 0.3, moved aside) as a first component: every vertex of ``positions`` moves 4 rows down."""
    tv, tf = regular_tetrahedron()
    tet = np.broadcast_to((0.3 * tv + [3.0, 0.0, 0.0]).astype(positions.dtype), (positions.shape[0], 4, 3))
    return np.concatenate([tet, positions], 1), np.concatenate([tf, np.asarray(faces) + 4])


def seamed_cube():
    """A cube as 12 triangles over 8 positions, with 14 UVs laid out as a cross with seams: 16 distinct (position, UV) pairs; positions
    carry one, two or three UVs, and two UVs are shared by two positions, so neither index alone identifies a glTF vertex.  The chart
    is a test pattern, not a faithful unfolding.  Returns (verts [8, 3], faces [12, 3], uvs [14, 2], faces_uvs [12, 3])."""
    verts = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    cross = [(0, 1, 2, 3), (4, 5, 6, 7), (8, 9, 5, 4), (1, 10, 11, 2), (12, 4, 7, 13), (0, 3, 6, 5)]
    uvs = np.array([[0.25, 0.0], [0.5, 0.0], [0.5, 0.25], [0.25, 0.25], [0.25, 0.5], [0.5, 0.5], [0.5, 0.75], [0.25, 0.75], [0.25, 1.0],
                    [0.5, 1.0], [0.75, 0.0], [0.75, 0.25], [0.0, 0.5], [0.0, 0.75]])
    tri = lambda q: [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    faces = np.array([t for q in quads for t in tri(q)], dtype=np.int64)
    faces_uvs = np.array([t for q in cross for t in tri(q)], dtype=np.int64)
    return verts, faces, uvs, faces_uvs


# ---- a minimal GLB reader

class Glb:
    """``json``: the JSON chunk parsed; ``bin``: the BIN chunk; ``raw``: the layout facts the tests assert (lengths, paddings, types)."""

    def __init__(self, path):
        data = open(path, "rb").read()
        magic, version, length = struct.unpack_from("<III", data, 0)
        n_json, t_json = struct.unpack_from("<II", data, 12)
        text = data[20:20 + n_json]
        n_bin, t_bin = struct.unpack_from("<II", data, 20 + n_json)
        self.bin = data[28 + n_json:28 + n_json + n_bin]
        self.json = json.loads(text.decode("utf-8"))
        self.raw = dict(magic=magic, version=version, length=length, size=len(data), json_length=n_json, json_type=t_json, bin_length=n_bin,
                        bin_type=t_bin, json_text=text, end=28 + n_json + n_bin)

    def view(self, i):
        v = self.json["bufferViews"][i]
        off = v.get("byteOffset", 0)
        return self.bin[off:off + v["byteLength"]]

    def accessor(self, i):
        a = self.json["accessors"][i]
        width = COMPONENTS[a["type"]]
        arr = np.frombuffer(self.view(a["bufferView"]), dtype=DTYPES[a["componentType"]], count=a["count"] * width, offset=a.get("byteOffset", 0))
        return arr.reshape(a["count"], width) if width > 1 else arr
