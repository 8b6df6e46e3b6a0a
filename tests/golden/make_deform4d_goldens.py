"""Generate tests/golden/deform4d.npz by running the REFERENCE's own deformation-field code on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_deform4d_goldens.py <path to the reference tree>

``grid_sample_wrapper`` and the ``Gaussian4DModel`` methods ``init_grid_param``, ``interpolate_ms_features``, ``get_xyz``, ``get_rotation``,
``get_scaling`` (custom/threestudio-animate3d/geometry/gaussian_4d.py), ``VanillaMLP`` (threestudio/models/networks.py) and
``build_rotation``, ``extract_rotation_torch``, ``euler_angles_to_rotation_matrix`` (geometry/utils.py) are compiled from the reference
files as they lie (the modules import threestudio, plyfile and a CUDA extension, so only these definitions are executed) and run on a
stub ``self``.  The per-frame glue below restates diff_gaussian_rasterizer_advanced_4d.py:77-135.  ``scaling_activation`` /
``rotation_activation`` belong to the threestudio-3dgs plugin, absent from the reference tree: torch.exp and F.normalize, the 3DGS standard.
Only data is written: seeded inputs, weights, the reference's outputs and its state-dict key names and shapes."""
import ast
import itertools
import math
import os
import sys
import types
from typing import Collection, Iterable, Optional, Sequence

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import deform_ref  # noqa: E402

N, GRID_SIZE, TIMESTAMPS, SEED = deform_ref.SCENES["golden"]
MLP_CONFIG = {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 32, "n_hidden_layers": 1}


def extract(path, names):
    """Module-level functions / classes and methods of any class called ``names``, as top-level definitions."""
    tree = ast.parse(open(path).read())
    found = {}
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            found[node.name] = node
        if isinstance(node, ast.ClassDef):
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name in names:
                    found[sub.name] = sub
    missing = set(names) - set(found)
    assert not missing, missing
    return ast.Module(body=[found[n] for n in names], type_ignores=[])


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = {"torch": torch, "nn": nn, "F": F, "math": math, "itertools": itertools, "np": np, "Sequence": Sequence, "Collection": Collection,
          "Iterable": Iterable, "Optional": Optional, "get_activation": lambda name: (lambda x: x)}
    geo = os.path.join(ref, "custom", "threestudio-animate3d", "geometry")
    for path, names in ((os.path.join(geo, "utils.py"), ("build_rotation", "extract_rotation_torch", "euler_angles_to_rotation_matrix")),
                        (os.path.join(ref, "threestudio", "models", "networks.py"), ("VanillaMLP",)),
                        (os.path.join(geo, "gaussian_4d.py"), ("grid_sample_wrapper", "init_grid_param", "interpolate_ms_features", "get_xyz",
                                                               "get_rotation", "get_scaling"))):
        exec(compile(extract(path, names), os.path.basename(path), "exec"), ns)

    class Stub(nn.Module):
        pass

    for name in ("interpolate_ms_features", "get_xyz", "get_rotation", "get_scaling"):
        setattr(Stub, name, ns[name])
    scene = deform_ref.make_scene(N, GRID_SIZE, TIMESTAMPS, seed=SEED, use_global_trans=True)
    out = {"grid_size": np.array(GRID_SIZE), "timestamps": scene["timestamps"].numpy(), "xyz": scene["xyz"].numpy(),
           "scaling": scene["scaling"].numpy(), "rotation": scene["rotation"].numpy()}
    for s, planes in enumerate(scene["grids"]):
        for p, plane in enumerate(planes):
            out[f"grids.{s}.{p}"] = plane.numpy()
    for name, (w0, w2) in scene["nets"].items():
        out[f"{name}.layers.0.weight"], out[f"{name}.layers.2.weight"] = w0.numpy(), w2.numpy()

    for use_global in (False, True):
        torch.manual_seed(1)
        st = Stub()
        st.cfg = types.SimpleNamespace(use_global_trans=use_global)
        st.grids = nn.ModuleList([ns["init_grid_param"](st, grid_nd=2, in_dim=4, out_dim=16, reso=reso) for reso in GRID_SIZE])
        names = deform_ref.LOCAL + (deform_ref.GLOBAL if use_global else ())
        for name in names:
            setattr(st, name, ns["VanillaMLP"](32, deform_ref.OUT[name], MLP_CONFIG))
        tag = "global" if use_global else "local"
        sd = st.state_dict()
        out[f"keys_{tag}"] = np.array(list(sd.keys()))
        out[f"shapes_{tag}"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        if use_global:                       # the reference's initial values of the planes: min / max per plane
            out["init_min"] = np.array([float(p.min()) for g in st.grids for p in g], dtype=np.float32)
            out["init_max"] = np.array([float(p.max()) for g in st.grids for p in g], dtype=np.float32)
        state = {k: torch.from_numpy(out[k]) for k in sd}
        st.load_state_dict(state, strict=True)
        st.register_buffer("_xyz", scene["xyz"].clone())
        st._scaling, st._rotation = scene["scaling"].clone(), scene["rotation"].clone()
        st.scaling_activation, st.rotation_activation = torch.exp, F.normalize
        st.global_rot_trans_activation = nn.Sigmoid()
        for deform_scales in (False, True):
            for fft in (False, True):
                means, scales, rots = [], [], []
                with torch.no_grad():
                    for t in scene["timestamps"]:
                        hidden = None
                        if fft or not bool((t == -1).all()):
                            pts = torch.cat([st._xyz, torch.ones_like(st._xyz[..., 0:1]) * t], dim=-1)
                            hidden = st.interpolate_ms_features(pts, st.grids)
                        means.append(st.get_xyz(hidden))
                        scales.append(st.get_scaling(hidden) if deform_scales else st.get_scaling())
                        rots.append(st.get_rotation(hidden))
                key = f"{tag}_ds{int(deform_scales)}_fft{int(fft)}"
                out[f"means_{key}"], out[f"scales_{key}"], out[f"rotations_{key}"] = (torch.stack(v).numpy() for v in (means, scales, rots))
    path = os.path.join(HERE, "deform4d.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
