"""Generate tests/golden/cameras.npz by running the REFERENCE's own data modules on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_camera_goldens.py <path to the reference tree>

The three dataset classes and the two config dataclasses of custom/threestudio-animate3d/data/uncond_hybrid.py and
``SimpleMultiImageDataBase`` of data/simple_multi_image.py are taken out of the reference files through the syntax tree and executed as
they lie (``collate``, ``progressive_view``, ``update_step``, the eval datasets' ``__init__`` / ``__getitem__``, the camera part of
``setup``); the modules import threestudio, pytorch_lightning and cv2 at their top, so only these definitions are executed, against
stubs.  ``get_ray_directions``, ``get_rays``, ``get_projection_matrix`` and ``get_mvp_matrix`` return placeholders of one element per
camera (the reference indexes and unpacks what they return), ``set_rays`` and ``load_images`` do nothing, ``threestudio`` only logs;
``torch`` in the executed namespace is a proxy that records every ``rand`` / ``randn`` result and otherwise delegates; ``random`` is
seeded per case.  Only data is written: per case the config, the recorded draws in the reference's order (the five per-object uniforms
as ``obj [R, 5]``, the position draw as ``pert_u [B, 3]``, the centre and up draws as ``pert_n [B, 6]``; the light draws that follow are
dropped), the coin, the reference's ``elevation``, ``azimuth``, ``camera_distances``, ``camera_positions``, ``c2w``, ``fovy``,
``timestamps``, ``height``, ``width``, and ``ref_err``: per field the largest absolute deviation of the reference's fp32 value from
tests/cameras_ref.py's float64 restatement on the same draws."""
import ast
import dataclasses
import json
import os
import random
import sys
import types
import typing

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import cameras_ref as R  # noqa: E402

FIELDS = R.RANDOM_FIELDS


class AttrDict(dict):
    __getattr__ = dict.__getitem__


class TorchProxy:
    """``torch`` with every ``rand`` / ``randn`` result recorded, in order."""

    def __init__(self):
        self.draws = []

    def rand(self, *a, **k):
        self.draws.append(("rand", torch.rand(*a, **k)))
        return self.draws[-1][1]

    def randn(self, *a, **k):
        self.draws.append(("randn", torch.randn(*a, **k)))
        return self.draws[-1][1]

    def __getattr__(self, name):
        return getattr(torch, name)


def per_camera(c2w):
    return torch.zeros(c2w.shape[0], 1)


def extract(path, names):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    return ast.fix_missing_locations(ast.Module(body=body, type_ignores=[]))


def namespace(proxy):
    ns = {k: getattr(typing, k) for k in typing.__all__}
    ns.update(torch=proxy, F=F, math=__import__("math"), random=random, bisect=__import__("bisect"), np=np, dataclass=dataclasses.dataclass,
              field=dataclasses.field, IterableDataset=type("IterableDataset", (), {}), Dataset=type("Dataset", (), {}),
              Updateable=type("Updateable", (), {}),
              threestudio=types.SimpleNamespace(warn=lambda *a: None, debug=lambda *a: None, info=lambda *a: None),
              get_ray_directions=lambda H, W, focal: torch.zeros(1, 1, 3), get_rays=lambda d, c2w, **k: (per_camera(c2w), per_camera(c2w)),
              get_projection_matrix=lambda fovy, *a: torch.zeros(fovy.shape[0], 1), get_mvp_matrix=lambda c2w, proj: per_camera(c2w),
              get_rank=lambda: 0, parse_structured=lambda cls, cfg: AttrDict(cfg))
    return ns


def with_defaults(cls, overrides):
    """The reference dataclass's own defaults, overridden; tuples become lists where the reference indexes them."""
    cfg = AttrDict(dataclasses.asdict(cls()))
    cfg.update({k: (list(v) if isinstance(v, tuple) else v) for k, v in overrides.items()})
    return cfg


def ref_err(reference, exact):
    return {f: float(np.abs(reference[f].astype(np.float64) - exact[f]).max()) for f in FIELDS}


def np32(t):
    return t.detach().numpy().astype(np.float32)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    data_dir = os.path.join(ref, "custom", "threestudio-animate3d", "data")
    proxy = TorchProxy()
    ns = namespace(proxy)
    hybrid = ("HybridRandomCameraDataModuleConfig", "HybridRandomCameraTestDataModuleConfig", "HybridRandomCameraIterableDataset",
              "HybridRandomCameraDataset", "HybridRandomCameraTestDataset")
    exec(compile(extract(os.path.join(data_dir, "uncond_hybrid.py"), hybrid), "uncond_hybrid.py", "exec"), ns)
    exec(compile(extract(os.path.join(data_dir, "simple_multi_image.py"), ("SimpleMultiImageDataBase",)), "simple_multi_image.py", "exec"), ns)
    out, meta = {}, {"random": [], "orbit": []}

    # the guidance sampler: update_step, then collate
    for i, case in enumerate(R.RANDOM_CASES):
        cfg = with_defaults(ns["HybridRandomCameraDataModuleConfig"], case["cfg"])
        for key in ("height", "width", "batch_size"):
            cfg[key] = cfg[key] if isinstance(cfg[key], int) else list(cfg[key])
        ds = ns["HybridRandomCameraIterableDataset"](cfg)
        ds.update_step(0, case["step"])
        random.seed(case["seed"])
        state = random.getstate()
        coin = random.random() < 0.5
        random.setstate(state)
        torch.manual_seed(1000 + case["seed"])
        proxy.draws.clear()
        batch = ds.collate(None)
        kinds = [k for k, _ in proxy.draws[:8]]
        assert kinds == ["rand"] * 6 + ["randn"] * 2, kinds
        draws = [t for _, t in proxy.draws[:8]]
        obj, pert_u, pert_n = torch.stack(draws[:5], dim=1), draws[5], torch.cat(draws[6:8], dim=1)
        assert (0 if coin else 1) == case["elev_mode"], (case["name"], coin)
        reference = {f: np32(batch[f]) for f in FIELDS}
        exact = R.random_from_draws(case["cfg"], case["step"], np32(obj), np32(pert_u), np32(pert_n), case["elev_mode"])
        err = ref_err(reference, exact)
        for f in FIELDS:
            out[f"random{i}_{f}"] = reference[f]
            out[f"random{i}_ref_err_{f}"] = np.array(err[f])
        out[f"random{i}_obj"], out[f"random{i}_pert_u"], out[f"random{i}_pert_n"] = np32(obj), np32(pert_u), np32(pert_n)
        out[f"random{i}_timestamps"] = np32(batch["timestamps"])
        meta["random"].append(dict(name=case["name"], coin=bool(coin), height=int(batch["height"]), width=int(batch["width"]),
                                   batch_size=int(ds.batch_size), elevation_range=list(map(float, ds.elevation_range)),
                                   azimuth_range=list(map(float, ds.azimuth_range)), ref_err=err))

    # the data views: the camera part of SimpleMultiImageDataBase.setup
    class DataBase(ns["SimpleMultiImageDataBase"]):
        def set_rays(self):
            pass

        def load_images(self):
            pass

    dv = R.DATA_VIEW_CASE
    cfg = AttrDict(dv, default_azimuth_deg=list(dv["default_azimuth_deg"]), use_random_camera=False, resolution_milestones=[])
    base = DataBase()
    base.setup(cfg, "train")
    reference = dict(elevation=np32(base.elevation_deg), azimuth=np32(base.azimuth_deg), camera_distances=np32(base.camera_distance),
                     camera_positions=np32(base.camera_position), c2w=np32(base.c2w4x4), fovy=np32(base.fovy))
    exact = R.spherical(reference["elevation"], reference["azimuth"], reference["camera_distances"], [dv["default_fovy_deg"]] * 12)
    err = ref_err(reference, exact)
    for f in FIELDS:
        out[f"data_{f}"] = reference[f]
        out[f"data_ref_err_{f}"] = np.array(err[f])
    out["data_timestamps"] = np32(base.timestamps)
    meta["data"] = dict(ref_err=err, height=int(base.height), width=int(base.width))

    # the evaluation sets, item by item
    def items_of(ds, n, fovy_deg):
        items = [ds[i] for i in range(n)]
        reference = dict(elevation=np32(torch.stack([it["elevation"] for it in items])), azimuth=np32(torch.stack([it["azimuth"] for it in items])),
                         camera_distances=np32(torch.stack([it["camera_distances"] for it in items])),
                         camera_positions=np32(torch.stack([it["camera_positions"] for it in items])),
                         c2w=np32(torch.stack([it["c2w"] for it in items])), fovy=np32(torch.stack([it["fovy"] for it in items])))
        exact = R.spherical(reference["elevation"], reference["azimuth"], reference["camera_distances"], [fovy_deg] * n)
        stamps = np32(torch.stack([it["timestamps"] for it in items]))
        sizes = sorted({(it["height"], it["width"]) for it in items})
        assert len(sizes) == 1 and [it["index"] for it in items] == list(range(n))
        return reference, stamps, ref_err(reference, exact), sizes[0]

    for i, case in enumerate(R.ORBIT_CASES):
        cfg = with_defaults(ns["HybridRandomCameraDataModuleConfig"], dict(R.ORBIT_CFG, n_val_views=case["n_val_views"],
                                                                           n_test_views=case["n_test_views"]))
        ds = ns["HybridRandomCameraDataset"](cfg, case["split"])
        reference, stamps, err, size = items_of(ds, len(ds), R.ORBIT_CFG["eval_fovy_deg"])
        for f in FIELDS:
            out[f"orbit{i}_{f}"] = reference[f]
            out[f"orbit{i}_ref_err_{f}"] = np.array(err[f])
        out[f"orbit{i}_timestamps"] = stamps
        out[f"orbit{i}_cameras_c2w"] = np32(ds.c2w)              # before the item map: which camera every item holds
        meta["orbit"].append(dict(case, n_items=len(ds), ref_err=err, height=size[0], width=size[1]))

    cfg = with_defaults(ns["HybridRandomCameraTestDataModuleConfig"], {k: ([list(r) for r in v] if k == "eval_azimuth_deg" else v)
                                                                       for k, v in R.TESTSET_CFG.items()})
    ds = ns["HybridRandomCameraTestDataset"](cfg, "test")
    reference, stamps, err, size = items_of(ds, len(ds), R.TESTSET_CFG["eval_fovy_deg"])
    for f in FIELDS:
        out[f"testset_{f}"] = reference[f]
        out[f"testset_ref_err_{f}"] = np.array(err[f])
    out["testset_timestamps"] = stamps
    out["testset_cameras_c2w"] = np32(ds.c2w)
    meta["testset"] = dict(n_items=len(ds), ref_err=err, height=size[0], width=size[1])

    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "cameras.npz")
    np.savez_compressed(path, **out)
    print(len(R.RANDOM_CASES), "random cases,", len(R.ORBIT_CASES), "orbit cases,", os.path.getsize(path), "bytes")
    for name, entry in [(c["name"], c) for c in meta["random"]] + [("data", meta["data"]), ("testset", meta["testset"])]:
        print(name, {k: f"{v:.2e}" for k, v in entry["ref_err"].items()})


if __name__ == "__main__":
    main()
