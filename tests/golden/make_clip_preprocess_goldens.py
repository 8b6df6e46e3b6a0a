"""Generate tests/golden/clip_preprocess.npz by running the REFERENCE's own image pre-processing path on the CPU.

Run in the build container only (needs the reference tree, Pillow and transformers):

    python -B tests/golden/make_clip_preprocess_goldens.py <path to the reference tree>

``IPAdapterImageProcessor`` (animatediff/utils/util.py:268-287) is compiled from the reference file as it lies (the module imports much
else at its top, so only this class is executed) and given ``transformers.CLIPImageProcessor()`` as its feature extractor and, as its
image encoder, a module that hands the pixel values it receives back as ``image_embeds``.  The images are built the way the guidance
builds them (custom/threestudio-animate3d/guidance/animatemv_guidance.py:553-554): ``Image.fromarray((image * 255).astype(np.uint8))``.
Only data is written: the small frame itself, the seed and a CRC of the large one, and the processor's ``pixel_values``."""
import ast
import os
import sys
import types
import zlib

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import clip_pre_ref  # noqa: E402

CASES = {"small": dict(h=37, w=29, seed=5, size=28), "big": dict(h=256, w=256, seed=6, size=224)}


class Echo(nn.Module):
    def __init__(self):
        super().__init__()
        self.p = nn.Parameter(torch.zeros(1))

    def forward(self, pixel_values):
        return types.SimpleNamespace(image_embeds=pixel_values)


def main():
    import transformers
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    tree = ast.parse(open(os.path.join(ref, "animatediff", "utils", "util.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "IPAdapterImageProcessor"]
    ns = {"nn": nn, "torch": torch}
    exec(compile(ast.fix_missing_locations(ast.Module(body=cls, type_ignores=[])), "util.py", "exec"), ns)
    out = {}
    for tag, c in CASES.items():
        fe = transformers.CLIPImageProcessor(size={"shortest_edge": c["size"]}, crop_size={"height": c["size"], "width": c["size"]})
        proc = ns["IPAdapterImageProcessor"](fe, Echo())
        frame = clip_pre_ref.golden_frame(c["h"], c["w"], c["seed"])
        image = Image.fromarray((frame * 255).astype(np.uint8))
        pv = proc.encode_image([image]).detach().numpy().astype(np.float32)
        out[f"{tag}_hw"], out[f"{tag}_seed"], out[f"{tag}_size"] = np.array([c["h"], c["w"]]), np.array(c["seed"]), np.array(c["size"])
        out[f"{tag}_crc"] = np.array(zlib.crc32(frame.tobytes()), dtype=np.uint32)
        out[f"{tag}_pixel_values"] = pv[0]
        mine = clip_pre_ref.preprocess(frame[None], c["size"], c["size"])[1][0]
        print(tag, pv.shape, "restatement max abs diff", float(np.abs(mine - pv[0]).max()))
    out["small_rgb"] = clip_pre_ref.golden_frame(**{k: CASES["small"][k] for k in ("h", "w", "seed")})
    path = os.path.join(HERE, "clip_preprocess.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
