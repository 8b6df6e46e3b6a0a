"""Generate tests/golden/stage_frames.npz by running the REFERENCE's own ``Animate3DSystem.test_step`` on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_stage_frames_goldens.py <path to the reference tree>

``test_step`` (custom/threestudio-animate3d/systems/animate3d.py:427-471) is taken out of the reference file through the syntax tree and
executed as it lies, as tests/golden/make_stage4d_goldens.py does with ``training_step``, against a stub ``self``: ``cfg`` is an attribute
dictionary, ``_save_dir`` a temporary directory, and the system is callable (the renderer): it returns the seeded render of
tests/frames_ref.py for ``batch["index"]`` as ``comp_rgb`` (the clamp and permute of the raw image, as advanced_4d.py:180 and
batch_renderer:73 make it), ``comp_mask`` and ``means3D``.  Both ``test_option``s run, ``n_frame = 3``, all 36 test-set indices and 12
four-view indices, ``save_gaussian_trajectory`` on.  Only data is written: per option the relative path of every file the reference wrote,
in index order, the decoded PNGs and the ``.npy`` arrays."""
import ast
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import frames_ref as R  # noqa: E402


def extract(path):
    tree = ast.parse(open(path).read())
    (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Animate3DSystem"]
    (fn,) = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "test_step"]
    return ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))


class System:
    """What ``test_step`` touches of ``self``."""

    def __init__(self, test_option, save_dir):
        self.cfg = types.SimpleNamespace(load_guidance=False, test_option=test_option, n_frame=R.N_FRAME, save_gaussian_trajectory=True)
        self._save_dir = save_dir
        self.seen = []

    def __call__(self, batch):
        i = int(batch["index"][0])
        self.seen.append((i, batch["do_guidance"], batch["do_reconstruction"]))
        image, alpha = R.make_render(R.render_key(self.cfg.test_option, i))
        return {"comp_rgb": image[None].clamp(0, 1).permute(0, 2, 3, 1), "comp_mask": alpha[None].permute(0, 2, 3, 1),
                "means3D": [R.make_means(R.render_key(self.cfg.test_option, i))]}


def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = {"torch": torch, "np": np, "os": os, "Image": Image}
    exec(compile(extract(os.path.join(ref, "custom", "threestudio-animate3d", "systems", "animate3d.py")), "animate3d.py", "exec"), ns)
    out = {}
    for option, count in R.COUNTS.items():
        with tempfile.TemporaryDirectory() as tmp:
            system = System(option, tmp)
            png_paths, npy_paths = [], []
            for i in range(count):
                before = set(files_under(tmp))
                ns["test_step"](system, {"index": torch.tensor([i])}, i)
                new = sorted(set(files_under(tmp)) - before)
                png_paths += [p for p in new if p.endswith(".png")]
                npy_paths += [p for p in new if p.endswith(".npy")]
                assert len(new) == (2 if i < R.N_FRAME else 1), (option, i, new)
            assert [s[0] for s in system.seen] == list(range(count)) and all(s[1:] == (False, True) for s in system.seen)
            assert files_under(tmp) == sorted(png_paths + npy_paths)
            images = []
            for p in png_paths:
                with Image.open(os.path.join(tmp, p)) as im:
                    assert im.mode == "RGBA"
                    images.append(np.asarray(im).copy())
            out[f"{option}_png_paths"] = np.array([p.replace(os.sep, "/") for p in png_paths])
            out[f"{option}_rgba"] = np.stack(images)
            out[f"{option}_npy_paths"] = np.array([p.replace(os.sep, "/") for p in npy_paths])
            out[f"{option}_npy"] = np.stack([np.load(os.path.join(tmp, p)) for p in npy_paths])
    path = os.path.join(HERE, "stage_frames.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
