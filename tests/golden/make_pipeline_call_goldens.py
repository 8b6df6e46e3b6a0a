"""Generate tests/golden/pipeline_call.npz by running the REFERENCE's own statements of ``AnimateDiffMVI2VPipeline.__call__`` around its loop.

Run where the reference tree is available:

    python -B tests/golden/make_pipeline_call_goldens.py [path to the reference tree]

Taken from the syntax tree of animatediff/pipelines/pipeline.py as they lie, and compiled into functions whose parameters are the names they
read (the module itself imports diffusers / torchvision, absent here): the methods ``encode_image`` (:527-538), ``encode_latents`` (:540-562),
``prepare_latents`` (:677-733, run with ``i2v_similarity_init`` = None) and ``decode_latents`` (:565-577), the functions ``tensor2vid``
(:237-255) and ``get_camera`` (:127-190), the two statements of ``__call__`` that put the unconditional halves in front (:931-937), and, through
tests/golden/make_pipeline_loop_goldens.py, the FreeInit / denoising loop statement (:988-1045).  They run in ``__call__``'s order with
stand-ins: the VAE, text and image encoders of tests/pipeline_ref.py, the UNet of tests/sds_stub.py, ``transforms.Resize`` as the identity
at the images' own size, torchvision's ``Normalize`` and diffusers' ``VaeImageProcessor.postprocess`` / ``randn_tensor`` / scheduler /
FreeInit restated (third-party; oracle/denoise_ref.py).  One generator serves the whole call; the stand-in VAE draws its posterior sample
from it, so the vectors pin the order of the draws: posterior sample, noise of frames 1.., FreeInit's fresh noise.

Only data (seeded inputs and the reference's outputs) is written; no reference source is copied."""
import ast
import contextlib
import math
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.denoise_ref import FreeInitRef  # noqa: E402
from tests import pipeline_ref as R  # noqa: E402
from tests.golden import make_pipeline_loop_goldens as L  # noqa: E402
from tests.sds_stub import stub_unet  # noqa: E402

N, F, SIDE, STEPS, SCALE, FREE_INIT_ITERS, SEED = 2, 4, 32, 3, 3.0, 2, 77


def _function(nodes, name, params, returns):
    """``nodes`` (statements of the reference) as the body of ``name(*params)`` that returns the names ``returns``."""
    ret = ast.Return(value=ast.Tuple(elts=[ast.Name(id=r, ctx=ast.Load()) for r in returns], ctx=ast.Load()))
    fn = ast.FunctionDef(name=name, args=ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in params], kwonlyargs=[], kw_defaults=[],
                                                       defaults=[]), body=list(nodes) + [ret], decorator_list=[])
    return ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))


def reference_pieces(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "animatediff/pipelines/pipeline.py")).read())
    cls = next(nd for nd in tree.body if isinstance(nd, ast.ClassDef) and nd.name == "AnimateDiffMVI2VPipeline")
    method = lambda name: next(nd for nd in cls.body if isinstance(nd, ast.FunctionDef) and nd.name == name)
    call = method("__call__")
    is_cfg = lambda t: isinstance(t, ast.Attribute) and t.attr == "do_classifier_free_guidance"
    cat_prompt = next(nd for nd in call.body if isinstance(nd, ast.If) and is_cfg(nd.test))
    cat_image = next(nd for nd in call.body if isinstance(nd, ast.If) and isinstance(nd.test, ast.Compare)
                     and getattr(nd.test.left, "id", None) == "ip_adapter_image" and any(is_cfg(s.test) for s in nd.body if isinstance(s, ast.If)))
    tensor2vid = next(nd for nd in tree.body if isinstance(nd, ast.FunctionDef) and nd.name == "tensor2vid")
    tensor2vid.returns = None
    for a in tensor2vid.args.args:
        a.annotation = None

    class Compose:
        def __init__(self, steps):
            self.steps = steps

        def __call__(self, x):
            for s in self.steps:
                x = s(x)
            return x

    def resize(size):                                  # the identity at the images' own size; anything else is not restated
        def run(x):
            assert min(x.shape[-2:]) == size, (x.shape, size)
            return x
        return run

    def normalize(mean, std, inplace=False):           # torchvision.transforms.functional.normalize
        def run(x):
            x = x if inplace else x.clone()
            m, s = torch.as_tensor(mean, dtype=x.dtype), torch.as_tensor(std, dtype=x.dtype)
            return x.sub_(m[:, None, None]).div_(s[:, None, None])
        return run

    top = lambda name: next(nd for nd in tree.body if isinstance(nd, ast.FunctionDef) and nd.name == name)
    ns = {"torch": torch, "np": np, "math": math, "F": torch.nn.functional, "transforms": SimpleNamespace(Compose=Compose, Resize=resize, Normalize=normalize),
          "randn_tensor": lambda shape, generator=None, device=None, dtype=None: torch.randn(shape, generator=generator, dtype=dtype)}
    mod = ast.fix_missing_locations(ast.Module(body=[method("encode_image"), method("encode_latents"), method("prepare_latents"),
                                                     method("decode_latents"), tensor2vid, top("get_camera"), top("generate_c2w"), top("normalize_camera")],
                                               type_ignores=[]))
    exec(compile(mod, "pipeline_pieces", "exec"), ns)
    exec(compile(_function([cat_prompt, cat_image], "front_halves", ["self", "prompt_embeds", "negative_prompt_embeds", "ip_adapter_image", "device"],
                           ["prompt_embeds", "image_embeds"]), "pipeline_front", "exec"), ns)
    return ns


def postprocess(image, output_type):                   # VaeImageProcessor.postprocess (do_normalize), diffusers 0.28.0
    image = (image / 2 + 0.5).clamp(0, 1)
    if output_type == "pt":
        return image
    image = image.cpu().permute(0, 2, 3, 1).float().numpy()
    if output_type == "np":
        return image
    return [Image.fromarray(i) for i in (image * 255).round().astype("uint8")]


def main(ref_root):
    ns = reference_pieces(ref_root)
    ref_loop = L.reference_loop()
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (N, SIDE, SIDE, 3), generator=g, dtype=torch.uint8).numpy()
    ids, neg_ids = torch.randint(1, 100, (1, 9), generator=g), torch.randint(1, 100, (1, 9), generator=g)
    pil = [Image.fromarray(i) for i in images]
    gen = torch.Generator().manual_seed(SEED)
    sched = L.Scheduler()
    sched.init_noise_sigma = 1.0                     # DDIMScheduler
    sched.set_timesteps(STEPS)
    fi = FreeInitRef(sched)
    calls = []

    def unet(sample, t, **kw):
        calls.append(sample.clone())
        kw.pop("cross_attention_kwargs")
        return stub_unet(sample, t, **kw)

    class ImageEncoder:
        def parameters(self):
            return iter([torch.zeros(1)])

        def __call__(self, x):
            return SimpleNamespace(image_embeds=R.stub_image_embeds(x))

    me = SimpleNamespace(
        vae=R.StubVAE(gen), vae_scale_factor=8, scheduler=sched, unet=unet, do_classifier_free_guidance=True, free_init_enabled=True,
        feature_extractor=lambda image, return_tensors: SimpleNamespace(pixel_values=R.unit_ref(np.stack([np.asarray(i) for i in image]))),
        image_encoder=ImageEncoder(),
        progress_bar=lambda total: contextlib.nullcontext(SimpleNamespace(update=lambda: None)),
        _apply_free_init=lambda lat, it, nsteps, device, dtype, generator: (fi.apply(lat, it, generator), sched.timesteps))
    me.encode_image = lambda image, device: ns["encode_image"](me, image, device)
    # step 3 (encode_prompt's per-view repeat restated: bs_embed = 1), then the reference's own two cat statements
    pe, ne = R.stub_text_encoder(ids)[0], R.stub_text_encoder(neg_ids)[0]
    pe, ne = pe.repeat(1, N, 1).view(N, pe.shape[1], -1), ne.repeat(1, N, 1).view(N, ne.shape[1], -1)
    prompt_embeds, image_embeds = ns["front_halves"](me, pe, ne, pil, "cpu")
    # step 5
    first = ns["encode_latents"](me, (SIDE, SIDE), pil).unsqueeze(2)
    rest = ns["prepare_latents"](me, N, 4, F - 1, SIDE, SIDE, torch.float32, "cpu", gen, None, None, latent_timestep=None, latent_cond_image=first)
    latents = torch.cat([first, rest], dim=2)
    camera = ns["get_camera"](N).to(prompt_embeds)      # :984
    final = ref_loop(me, latents.clone(), first, sched.timesteps, STEPS, "cpu", gen, None, 1.0, prompt_embeds, None, camera, None,
                     {"image_embeds": image_embeds}, False, SCALE, {}, None, [], None, 1, FREE_INIT_ITERS)
    video = ns["decode_latents"](me, final)
    frames = ns["tensor2vid"](video, SimpleNamespace(postprocess=postprocess), "pil")
    out = dict(images=images, ids=ids.numpy(), neg_ids=neg_ids.numpy(), camera=camera.numpy(), prompt_embeds=prompt_embeds.numpy(),
               image_embeds=image_embeds.numpy(), first=first.numpy(), latents=latents.numpy(), final=final.numpy(), video=video.numpy(),
               frames_u8=np.stack([np.stack([np.asarray(im) for im in view]) for view in frames]),
               frames_np=ns["tensor2vid"](video, SimpleNamespace(postprocess=postprocess), "np"),
               first_unet_sample=calls[0].numpy(), second_pass_unet_sample=calls[STEPS].numpy(),
               cfg=np.array([N, F, SIDE, STEPS, SCALE, FREE_INIT_ITERS, SEED, len(calls)], dtype=np.float64))
    path = os.path.join(HERE, "pipeline_call.npz")
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print("wrote", path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else L.REF)
