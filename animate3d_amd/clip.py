"""The condition towers in front of the denoising loop — SURVEY.md §8(f) item 3, first half.

``animatediff/pipelines/pipeline.py:345-524`` (``encode_prompt``: ``text_encoder(ids)[0]``) and ``:527-538`` /
``animatediff/utils/util.py:268-287`` (``encode_image``: ``image_encoder(pixels).image_embeds`` and a zero tensor for the
unconditional half) call two third-party transformers models once per sample:

* the SD1.5 text encoder, ``transformers.CLIPTextModel`` (ViT-L/14 text tower: 12 layers x 768, 12 heads of 64, QuickGELU,
  causal attention over 77 tokens, final LayerNorm) -> ``prompt_embeds [B, 77, 768]``;
* the IP-Adapter image encoder, ``transformers.CLIPVisionModelWithProjection`` (ViT-H/14: 32 layers x 1280, 16 heads of 80,
  GELU, 257 tokens, post-LayerNorm of the class token, 1280 -> 1024 projection) -> ``image_embeds [B, 1024]``.

Both run here on the kernels of the denoise step (LayerNorm, fused-QKV GEMMs with bias, flash attention — head dim 64 with the
causal flag, head dim 80 —, activation, residual GEMM epilogues) under transformers' parameter names, so
``load_state_dict(hf_model.state_dict())`` works key for key.  Tokenisation (CLIPTokenizer) stays with the caller: the text tower's
input is token ids.  The image tower takes normalised pixel values (``forward``) or rendered frames (``encode_frames``): for those,
``preprocess_frames`` is ``CLIPImageProcessor`` on the GPU, bit-equal to the PIL path and without a host synchronisation (below).  No
CPU fallback.
Parity: the oracle is transformers' own implementation (installed here; architecture unchanged since the reference's pin
4.25.1), tests/test_clip.py.

Image pre-processing of rendered frames — the 4D-SDS step encodes frame 0 of every (b, view) video on every optimisation step
(custom/threestudio-animate3d/guidance/animatemv_guidance.py:546-555): device -> host, ``(image * 255).astype(np.uint8)``, PIL images,
``CLIPImageProcessor`` (shortest edge to 224 with PIL's antialiased bicubic filter, centre crop 224, ``/255``, mean / std), host -> device.
PIL's 8-bit resampler is integer arithmetic on fixed-point coefficients, so the whole chain is reproduced exactly:

* ``resize_plan`` computes, on the host and once per input shape, what PIL computes per call: the coefficients in double precision
  (``precompute_coeffs``, bicubic a = -0.5), their fixed-point form at 22 precision bits with PIL's rounding (``normalize_coeffs_8bpc``), the
  output size, the crop offsets, and the table ``((v / 255) - mean) / std`` of the 256 byte values per channel (float64, rounded once);
* ``preprocess_frames`` is one launch of csrc/clip_preprocess.hip: quantisation, the horizontal and the vertical pass with a clip to a byte
  after each, crop, table look-up; it writes ``pixel_values`` or directly the zero-padded patch rows the tower's first GEMM reads.

Values: ``rgb`` in [0, 1] gives the reference's bytes; NaN and values below 0 become byte 0, values above 1 byte 255 (numpy's cast is
undefined there).  An ``image_index`` entry outside the batch gives a frame of zero bytes (nothing is read; no host check, no
synchronisation).  No gradient: the reference runs this under ``no_grad`` on detached frames.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn

from .f32_stage import launch, require_f32_cuda, require_index_cuda
from .hip_ops import _DTYPE_CODE, RowMap, _p, load_library, on_model_device
from .modules import Holder


@dataclass
class CLIPTowerConfig:
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    # text
    vocab_size: int = 49408
    max_position_embeddings: int = 77
    # vision
    image_size: int = 224
    patch_size: int = 14
    num_channels: int = 3
    projection_dim: int = 1024


TEXT_SD15 = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, hidden_act="quick_gelu")
VISION_VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, hidden_act="gelu",
                    image_size=224, patch_size=14, projection_dim=1024)


class _Attn(Holder):
    def __init__(self, c):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)


class _MLP(Holder):
    def __init__(self, c, i):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, i), nn.Linear(i, c)


class _Layer(Holder):
    def __init__(self, cfg):
        super().__init__()
        c = cfg.hidden_size
        self.self_attn = _Attn(c)
        self.layer_norm1 = nn.LayerNorm(c, eps=cfg.layer_norm_eps)
        self.mlp = _MLP(c, cfg.intermediate_size)
        self.layer_norm2 = nn.LayerNorm(c, eps=cfg.layer_norm_eps)


class _Encoder(Holder):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])


class _TextEmbeddings(Holder):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class _TextTransformer(Holder):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _TextEmbeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _VisionEmbeddings(Holder):
    def __init__(self, cfg):
        super().__init__()
        c = cfg.hidden_size
        self.class_embedding = nn.Parameter(torch.randn(c))
        self.patch_embedding = nn.Conv2d(cfg.num_channels, c, cfg.patch_size, stride=cfg.patch_size, bias=False)
        self.position_embedding = nn.Embedding((cfg.image_size // cfg.patch_size) ** 2 + 1, c)


class _VisionTransformer(Holder):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _VisionEmbeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)          # (sic: transformers' spelling)
        self.encoder = _Encoder(cfg)
        self.post_layernorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _Tower(nn.Module):
    """Shared machinery: op set following the model dtype, packed weights, one pre-LN transformer layer."""

    def __init__(self, config: CLIPTowerConfig, ops=None):
        super().__init__()
        self.config = config
        self._ops, self._ops_auto, self._packed = ops, False, None

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def ops(self):
        if self._ops is None:
            from .hip_ops import HipOps          # raises without an MI355X or without the built library
            self._ops = HipOps(self.device, torch.float16 if self.dtype == torch.float16 else torch.bfloat16)
            self._ops_auto = True
        return self._ops

    def _apply(self, fn, *a, **k):
        self._packed = None
        if self._ops_auto:
            self._ops, self._ops_auto = None, False
        return super()._apply(fn, *a, **k)

    _PREFIX = ""          # "text_model." / "vision_model.": transformers <= 4.x key prefix (the reference's checkpoints have it)

    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}        # buffer of older transformers versions
        fam = ("embeddings.", "encoder.", "final_layer_norm.", "pre_layrnorm.", "post_layernorm.")
        sd = {(self._PREFIX + k if k.startswith(fam) else k): v for k, v in sd.items()}   # transformers 5.x dropped the prefix
        self._packed = None
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _w(self, t):
        return t.detach().to(self.ops.act_dtype).contiguous()

    @staticmethod
    def _f(t):
        return t.detach().float().contiguous()

    def _pack_layers(self, enc: _Encoder):
        out = []
        for l in enc.layers:
            a = l.self_attn
            out.append(SimpleNamespace(
                n1=(self._f(l.layer_norm1.weight), self._f(l.layer_norm1.bias)),
                qkv=(self._w(torch.cat([a.q_proj.weight.detach(), a.k_proj.weight.detach(), a.v_proj.weight.detach()], 0)),
                     self._f(torch.cat([a.q_proj.bias.detach(), a.k_proj.bias.detach(), a.v_proj.bias.detach()], 0))),
                o=(self._w(a.out_proj.weight), self._f(a.out_proj.bias)),
                n2=(self._f(l.layer_norm2.weight), self._f(l.layer_norm2.bias)),
                fc1=(self._w(l.mlp.fc1.weight), self._f(l.mlp.fc1.bias)), fc2=(self._w(l.mlp.fc2.weight), self._f(l.mlp.fc2.bias))))
        return out

    def _layer(self, x, pk, B, T, causal):
        """transformers CLIPEncoderLayer: x += attn(LN1(x)); x += fc2(act(fc1(LN2(x))))."""
        ops, cfg = self.ops, self.config
        C = x.shape[1]
        h = ops.layer_norm(x, pk.n1[0], pk.n1[1], cfg.layer_norm_eps)
        qkv = ops.gemm(h, pk.qkv[0], pk.qkv[1])
        m = RowMap(gdiv=1, ga=T, gb=0, seg_len=T, seg_stride=0)
        a = ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], m, m, B, cfg.num_attention_heads, T, T, causal=causal)
        x = ops.gemm(a, pk.o[0], pk.o[1], residual=x)
        h = ops.layer_norm(x, pk.n2[0], pk.n2[1], cfg.layer_norm_eps)
        h = ops.activation(ops.gemm(h, pk.fc1[0], pk.fc1[1]), cfg.hidden_act)
        return ops.gemm(h, pk.fc2[0], pk.fc2[1], residual=x)


class CLIPTextEncoder(_Tower):
    """``transformers.CLIPTextModel`` of the SD1.5 pipeline (inference.py:64) — ``forward(input_ids)[0]`` = last hidden state."""
    _PREFIX = "text_model."

    def __init__(self, config: Optional[CLIPTowerConfig] = None, ops=None, device: Optional[Union[str, torch.device]] = None, **overrides):
        cfg = config if config is not None else CLIPTowerConfig(**{**TEXT_SD15, **overrides})
        super().__init__(cfg, ops)
        with (torch.device(device) if device is not None else torch.device("cpu")):
            self.text_model = _TextTransformer(cfg)

    def _pack(self):
        tm = self.text_model
        self._packed = SimpleNamespace(layers=self._pack_layers(tm.encoder),
                                       final=(self._f(tm.final_layer_norm.weight), self._f(tm.final_layer_norm.bias)))
        return self._packed

    @torch.no_grad()
    @on_model_device
    def forward(self, input_ids: torch.Tensor, attention_mask=None, **unused) -> Tuple[torch.Tensor]:
        if attention_mask is not None:
            raise NotImplementedError("the reference passes attention_mask=None (SD1.5 text encoder config has no use_attention_mask)")
        P = self._packed if self._packed is not None else self._pack()
        ops, cfg, emb = self.ops, self.config, self.text_model.embeddings
        B, T = input_ids.shape
        if T > cfg.max_position_embeddings:
            raise ValueError(f"{T} tokens exceed max_position_embeddings = {cfg.max_position_embeddings}")
        ids = input_ids.to(self.device)
        x = (emb.token_embedding.weight[ids].float() + emb.position_embedding.weight[:T].float()[None]).reshape(B * T, -1)
        x = x.to(ops.act_dtype).contiguous()
        for pk in P.layers:
            x = self._layer(x, pk, B, T, causal=True)
        x = ops.layer_norm(x, P.final[0], P.final[1], cfg.layer_norm_eps)
        return (x.reshape(B, T, -1).to(self.dtype if self.dtype != torch.float32 else torch.float32),)


class CLIPVisionEncoderWithProjection(_Tower):
    """``transformers.CLIPVisionModelWithProjection`` (IP-Adapter image encoder, inference.py:78): ``forward(pixels).image_embeds``."""
    _PREFIX = "vision_model."

    def __init__(self, config: Optional[CLIPTowerConfig] = None, ops=None, device: Optional[Union[str, torch.device]] = None, **overrides):
        cfg = config if config is not None else CLIPTowerConfig(**{**VISION_VIT_H, **overrides})
        super().__init__(cfg, ops)
        with (torch.device(device) if device is not None else torch.device("cpu")):
            self.vision_model = _VisionTransformer(cfg)
            self.visual_projection = nn.Linear(cfg.hidden_size, cfg.projection_dim, bias=False)

    def _pack(self):
        vm, cfg = self.vision_model, self.config
        k = cfg.num_channels * cfg.patch_size ** 2
        kp = (k + 63) // 64 * 64                              # the GEMM contracts in steps of 64: zero-padded patch vectors
        wp = torch.zeros(cfg.hidden_size, kp, device=self.device, dtype=torch.float32)
        wp[:, :k] = vm.embeddings.patch_embedding.weight.detach().float().reshape(cfg.hidden_size, k)       # (c, ky, kx) order
        self._packed = SimpleNamespace(
            patch=self._w(wp), kp=kp, pre=(self._f(vm.pre_layrnorm.weight), self._f(vm.pre_layrnorm.bias)),
            layers=self._pack_layers(vm.encoder), post=(self._f(vm.post_layernorm.weight), self._f(vm.post_layernorm.bias)),
            proj=self._w(self.visual_projection.weight))
        return self._packed

    def _grid(self, H: int, W: int):
        ps, emb = self.config.patch_size, self.vision_model.embeddings
        gh, gw = H // ps, W // ps
        if (gh * gw + 1) != emb.position_embedding.weight.shape[0]:
            raise ValueError(f"image {H}x{W} does not match the position table ({emb.position_embedding.weight.shape[0]} entries)")
        return gh, gw

    @torch.no_grad()
    @on_model_device
    def forward(self, pixel_values: torch.Tensor, **unused):
        P = self._packed if self._packed is not None else self._pack()
        ops, cfg = self.ops, self.config
        B, Cc, H, W = pixel_values.shape
        ps = cfg.patch_size
        gh, gw = self._grid(H, W)
        # non-overlapping patches are a pure re-layout: [B, C, gh, ps, gw, ps] -> [(B gh gw), (C ps ps)], zero-padded to the GEMM step
        px = pixel_values.to(self.device).float().reshape(B, Cc, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, Cc * ps * ps)
        pad = torch.zeros(B * gh * gw, P.kp, device=self.device, dtype=ops.act_dtype)
        pad[:, : px.shape[1]] = px.to(ops.act_dtype)
        return self._encode_patch_rows(P, pad, B, gh, gw)

    @torch.no_grad()
    @on_model_device
    def encode_frames(self, rgb: torch.Tensor, image_index: Optional[torch.Tensor] = None):
        """``forward(CLIPImageProcessor(frames))`` for rendered frames ``rgb [N, H, W, 3]`` (float32, on the tower's device; ``image_index``
        picks frames): ``preprocess_frames`` writes the patch rows that ``forward`` lays out with reshape / permute / zeros / copy, so the
        result is bitwise that of ``forward(preprocess_frames(rgb, image_index, size=image_size, crop=image_size))``."""
        require_f32_cuda("rgb", rgb)
        if rgb.device != self.device:
            raise RuntimeError(f"encode_frames: rgb lives on {rgb.device}, the tower on {self.device}")
        P = self._packed if self._packed is not None else self._pack()
        cfg = self.config
        s, ps = cfg.image_size, cfg.patch_size
        if s % ps != 0:
            raise ValueError(f"image_size {s} is not a multiple of patch_size {ps}")
        gh, gw = self._grid(s, s)
        pad = preprocess_frames(rgb, image_index, size=s, crop=s, dtype=self.ops.act_dtype, patch_rows=(ps, P.kp))
        return self._encode_patch_rows(P, pad, pad.shape[0] // (gh * gw), gh, gw)

    def _encode_patch_rows(self, P, pad: torch.Tensor, B: int, gh: int, gw: int):
        """The tower from its first GEMM on: ``pad [(B gh gw), kp]`` patch rows in the activation dtype."""
        ops, cfg, emb = self.ops, self.config, self.vision_model.embeddings
        patches = ops.gemm(pad, P.patch).reshape(B, gh * gw, -1)
        T = gh * gw + 1
        x = torch.cat([emb.class_embedding.to(patches.dtype)[None, None].expand(B, 1, -1), patches], dim=1)
        x = (x.float() + emb.position_embedding.weight[:T].float()[None]).to(ops.act_dtype).reshape(B * T, -1).contiguous()
        x = ops.layer_norm(x, P.pre[0], P.pre[1], cfg.layer_norm_eps)
        for pk in P.layers:
            x = self._layer(x, pk, B, T, causal=False)
        pooled = ops.layer_norm(x.reshape(B, T, -1)[:, 0].contiguous(), P.post[0], P.post[1], cfg.layer_norm_eps)
        embeds = ops.gemm(pooled, P.proj)
        out_dtype = self.dtype
        return SimpleNamespace(image_embeds=embeds.to(out_dtype), last_hidden_state=x.reshape(B, T, -1).to(out_dtype))


@torch.no_grad()
def encode_prompt(text_encoder, input_ids: torch.Tensor, negative_input_ids: Optional[torch.Tensor] = None):
    """pipeline.py:345-524 without the tokenizer: (prompt_embeds, negative_prompt_embeds or None), each [B, 77, 768]."""
    pe = text_encoder(input_ids)[0]
    ne = text_encoder(negative_input_ids)[0] if negative_input_ids is not None else None
    return pe, ne


@torch.no_grad()
def encode_image(image_encoder, pixel_values: torch.Tensor):
    """pipeline.py:527-538: (image_embeds, zeros_like(image_embeds)) — the unconditional half is all zeros."""
    e = image_encoder(pixel_values).image_embeds
    return e, torch.zeros_like(e)


@torch.no_grad()
def encode_image_from_frames(image_encoder, rgb: torch.Tensor, image_index: Optional[torch.Tensor] = None):
    """``encode_image`` from rendered frames ``rgb [N, H, W, 3]`` in [0, 1] instead of processed pixel values: replaces
    animatemv_guidance.py:546-555 (host copy, PIL, ``CLIPImageProcessor``, copy back) and stays on the device."""
    e = image_encoder.encode_frames(rgb, image_index).image_embeds
    return e, torch.zeros_like(e)


# ---- CLIPImageProcessor on the GPU (csrc/clip_preprocess.hip)

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # what CLIPImageProcessor() defaults to
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 32 - 8 - 2                                      # PIL's 8-bit resampler
TILE_ROWS = 14                                                   # output rows per workgroup when no patch size sets them


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _axis_tables(in_size: int, out_size: int):
    """PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for one axis: (ksize, [[first, count]] * out, [[k] * ksize] * out), in Python
    floats (C doubles) and in PIL's order of operations."""
    scale = filterscale = in_size / out_size
    filterscale = max(filterscale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    one = 1 << PRECISION_BITS
    bounds, coefs = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - first
        w = [_bicubic((x + first - center + 0.5) * ss) for x in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds.append([first, count])
        coefs.append([int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w] + [0] * (ksize - count))
    return ksize, bounds, coefs


class ResizePlan:
    """Everything ``preprocess_frames`` needs for one input shape: see ``resize_plan``.  ``coef_* [crop, ksize]`` / ``bounds_* [crop, 2]``
    (int32; x: horizontal pass, y: vertical) hold only the rows and columns inside the crop window and are None with ``ksize_* == 0`` when
    PIL skips that pass (equal sizes); ``table [3, 256]`` float32.  ``host`` keeps CPU copies of the tables."""

    def __init__(self, in_h: int, in_w: int, size: int, crop: int, device):
        short, long = (in_w, in_h) if in_w <= in_h else (in_h, in_w)
        new_long = int(size * long / short)                   # transformers' get_resize_output_image_size, default_to_square=False
        self.out_h, self.out_w = (new_long, size) if in_w <= in_h else (size, new_long)
        if self.out_h < crop or self.out_w < crop:
            raise ValueError(f"a {in_h}x{in_w} frame resized to {self.out_h}x{self.out_w} is smaller than the {crop}x{crop} crop")
        self.in_h, self.in_w, self.size, self.crop, self.device = in_h, in_w, size, crop, torch.device(device)
        self.off_y, self.off_x = (self.out_h - crop) // 2, (self.out_w - crop) // 2
        self.host = SimpleNamespace()
        for axis, n_in, n_out, off in (("x", in_w, self.out_w, self.off_x), ("y", in_h, self.out_h, self.off_y)):
            if n_in == n_out:
                ksize, bounds, coef = 0, None, None
            else:
                ksize, b, k = _axis_tables(n_in, n_out)
                bounds = torch.tensor(b[off:off + crop], dtype=torch.int32)
                coef = torch.tensor(k[off:off + crop], dtype=torch.int32)
            setattr(self, "ksize_" + axis, ksize)
            setattr(self.host, "bounds_" + axis, bounds)
            setattr(self.host, "coef_" + axis, coef)
            setattr(self, "bounds_" + axis, None if bounds is None else bounds.to(self.device))
            setattr(self, "coef_" + axis, None if coef is None else coef.to(self.device))
        v = torch.arange(256, dtype=torch.float64)[None] / 255.0
        mean, std = torch.tensor(OPENAI_CLIP_MEAN, dtype=torch.float64)[:, None], torch.tensor(OPENAI_CLIP_STD, dtype=torch.float64)[:, None]
        self.host.table = ((v - mean) / std).to(torch.float32)
        self.table = self.host.table.to(self.device)
        self._max_rows = {}

    def max_rows(self, tile_rows: int) -> int:
        """The most input rows the vertical pass of one tile of ``tile_rows`` output rows reads: the kernel's LDS intermediate has that
        many rows of 3 * crop bytes."""
        if tile_rows not in self._max_rows:
            if self.ksize_y == 0:
                m = min(tile_rows, self.crop)
            else:
                b = self.host.bounds_y.tolist()
                m = max(b[min(t + tile_rows, self.crop) - 1][0] + b[min(t + tile_rows, self.crop) - 1][1] - b[t][0]
                        for t in range(0, self.crop, tile_rows))
            self._max_rows[tile_rows] = m
        return self._max_rows[tile_rows]


_PLANS = {}


def resize_plan(in_h: int, in_w: int, size: int = 224, crop: int = 224, device="cuda") -> ResizePlan:
    """The plan of ``CLIPImageProcessor(size, crop)`` for ``in_h x in_w`` frames: shortest edge -> ``size`` (the other edge
    ``int(size * long / short)``), centre crop at ``((h - crop) // 2, (w - crop) // 2)``, PIL's bicubic coefficients in fixed point, and the
    normalisation table.  Cached per (in_h, in_w, size, crop, device): after the first call for a shape nothing is computed or uploaded.
    ``ValueError`` when the resized frame is smaller than the crop (the processor would pad; the 4D-SDS step never does)."""
    in_h, in_w, size, crop = int(in_h), int(in_w), int(size), int(crop)
    if min(in_h, in_w, size, crop) < 1:
        raise ValueError(f"sizes must be positive, got {in_h}x{in_w}, size {size}, crop {crop}")
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (in_h, in_w, size, crop, str(dev))
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = ResizePlan(in_h, in_w, size, crop, dev)
    return plan


def preprocess_lds_limit() -> int:
    """Bytes of LDS one tile's intermediate may take (``plan.max_rows(tile_rows) * 3 * crop``); a larger one is refused by the kernel."""
    return int(load_library().a3d_clip_preprocess_lds_limit())


@torch.no_grad()
def preprocess_frames(rgb: torch.Tensor, image_index: Optional[torch.Tensor] = None, *, size: int = 224, crop: int = 224,
                      dtype: torch.dtype = torch.float32, patch_rows: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                      return_u8: bool = False):
    """``CLIPImageProcessor(size, crop)(PIL images of (rgb * 255).astype(uint8))`` on the GPU, bit-equal to it (module docstring).

    ``rgb [N, H, W, 3]`` float32 CUDA, any strides (the permuted view of a ``[N, 3, H, W]`` render is read in place); ``image_index [n]``
    int32 / int64 CUDA picks frames, None takes all.  Returns ``pixel_values [n, 3, crop, crop]`` of ``dtype`` (float32, float16 or
    bfloat16: one rounding of the float32 value) or, with ``patch_rows=(patch, kp)``, the matrix ``[n (crop / patch)^2, kp]`` of patch
    rows in (c, ky, kx) order with columns ``3 patch^2 .. kp`` zero: the first GEMM operand of the image tower.  ``out``: a contiguous
    tensor of that shape and dtype to write into.  ``return_u8``: also the resized and cropped bytes ``[n, crop, crop, 3]`` uint8.
    Nothing synchronises with the host once the shape's plan exists.  Anything but a float32 CUDA ``rgb`` raises; so does a frame too
    small for the crop (``ValueError``) and one so large that a tile's intermediate does not fit LDS (``RuntimeError``)."""
    require_f32_cuda("rgb", rgb)
    if rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.shape[0] < 1:
        raise ValueError(f"rgb: expected [N, H, W, 3], got {tuple(rgb.shape)}")
    if dtype not in _DTYPE_CODE:
        raise ValueError(f"dtype {dtype}: float32, float16 or bfloat16")
    dev = rgb.device
    N, H, W, _ = rgb.shape
    plan = resize_plan(H, W, size, crop, dev)
    crop = plan.crop
    idx, n = None, N
    if image_index is not None:
        require_index_cuda("image_index", image_index)
        if image_index.dim() != 1 or image_index.shape[0] < 1 or image_index.device != dev:
            raise ValueError("image_index: a non-empty 1-D tensor on rgb's device")
        idx = image_index.detach().to(torch.int32).contiguous()
        n = idx.shape[0]
    if patch_rows is not None:
        patch, kp = int(patch_rows[0]), int(patch_rows[1])
        if patch < 1 or crop % patch != 0 or kp < 3 * patch * patch:
            raise ValueError(f"patch_rows=(patch {patch}, kp {kp}): crop {crop} must be a multiple of patch and kp >= 3 * patch ** 2")
        tile_rows, shape = patch, (n * (crop // patch) ** 2, kp)
    else:
        patch, kp, tile_rows, shape = 0, 0, min(TILE_ROWS, crop), (n, 3, crop, crop)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == dtype and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous {dtype} tensor of shape {shape} on {dev}")
    u8 = torch.empty(n, crop, crop, 3, dtype=torch.uint8, device=dev) if return_u8 else None
    src = rgb.detach()
    launch("a3d_clip_preprocess", dev, _p(src), N, H, W, src.stride(0), src.stride(1), src.stride(2), src.stride(3), _p(idx), n, crop,
           _p(plan.coef_x), _p(plan.bounds_x), plan.ksize_x, plan.off_x, _p(plan.coef_y), _p(plan.bounds_y), plan.ksize_y, plan.off_y,
           tile_rows, plan.max_rows(tile_rows), _p(plan.table), _DTYPE_CODE[dtype], _p(out) if patch_rows is None else None,
           _p(out) if patch_rows is not None else None, patch, kp, _p(u8))
    return (out, u8) if return_u8 else out
