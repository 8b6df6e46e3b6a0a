"""ctypes binding of libanimate3d_hip.so + the op set the UNet host code is written against.

The C header include/animate3d_hip.h is the binding's only source: ``parse_header`` reads every entry point's signature, the two enums and
the ``#define A3D_*`` integers from its text, ``load_library`` types the library from that, and the header's constants are this module's
attributes under their own names.  Only the two structs are written out here (tests/test_header_binding.py holds them to the header).

torch is used here only for device memory (``torch.empty``), the current HIP stream handle and
pointer extraction; every arithmetic op goes through the C-ABI.  There is NO fallback: if the
library is missing, fails to load, or a tensor is not a CUDA tensor of the op set's 16-bit storage type, these calls raise.
"""
from __future__ import annotations

import ctypes
import os
import re
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_PKG, "lib", "libanimate3d_hip.so")
_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "animate3d_hip.h")
_lib = None

c_i64, c_int, c_f32, c_f64, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p


class _RowMapC(ctypes.Structure):
    """a3d_rowmap of include/animate3d_hip.h."""
    _fields_ = [("gdiv", c_i64), ("ga", c_i64), ("gb", c_i64), ("seg_len", c_i64), ("seg_stride", c_i64), ("ld", c_i64)]


class StageAdamEntry(ctypes.Structure):
    """a3d_stage_adam_entry of include/animate3d_hip.h: one tensor of a3d_stage_adam_f32's host table."""
    _fields_ = [("p", c_vp), ("g", c_vp), ("m", c_vp), ("v", c_vp), ("step", c_vp), ("n", c_i64), ("lr", c_f64)]


# ---- the header as the binding's source
class Header(NamedTuple):
    functions: dict      # entry point -> (restype, argtypes), in the header's order
    constants: dict      # enumerator or #define A3D_* -> int
    structs: dict        # typedef struct -> [(field, ctypes type)]


_SCALARS = {"int": c_int, "int64_t": c_i64, "float": c_f32, "double": c_f64, "a3d_stream_t": c_vp}
_POINTEES = {"void", "char", "int", "unsigned int", "uint8_t", "int64_t", "float", "double"}


def _c_type(text: str, structs, named: bool = True):
    """(ctypes type, name) of ``[const] T [*] [name]``.  Every pointer is ``c_void_p``, which takes an address, ``ctypes.byref`` and a
    ctypes array alike (``const char*``: ``c_char_p``).  A ``T`` outside the header's vocabulary raises: nothing is guessed."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    name = words.pop() if named and words else None
    base, stars = " ".join(w for w in words if w != "*"), words.count("*")
    if name is None or name.isidentifier():
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base], name
        if stars == 1 and (base in _POINTEES or base in structs):
            return (ctypes.c_char_p if base == "char" else c_vp), name
    raise RuntimeError(f"animate3d_hip.h: no ctypes type known for {' '.join(text.split())!r}")


def parse_header(text: str) -> Header:
    """What the binding needs of the header's text.  Whatever is left over that is not ``T a3d_name(parameters);`` raises."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {m[1]: int(m[2], 0) for m in re.finditer(r"^#define\s+(A3D_\w+)\s+(\S+)\s*$", text, flags=re.M)}
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    wrapped = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    text = wrapped[1] if wrapped else text

    def take(pattern):
        nonlocal text
        found = re.findall(pattern, text, flags=re.S)
        text = re.sub(pattern, "", text, flags=re.S)
        return found

    take(r"\btypedef\s+void\s*\*\s*a3d_stream_t\s*;")
    for body in take(r"\benum\s*\{(.*?)\}\s*;"):
        for item in body.split(","):
            name, _, value = item.partition("=")
            constants[name.strip()] = int(value, 0)
    structs = {}
    for struct, body in take(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"):
        fields = structs[struct] = []
        for decl in filter(str.strip, body.split(";")):          # ``T a, b, c;`` declares three fields of T
            first, *more = decl.split(",")
            ctype, name = _c_type(first, structs)
            fields += [(n.strip(), ctype) for n in (name, *more)]
    functions = {}
    for decl in filter(str.strip, text.split(";")):
        m = re.fullmatch(r"\s*(.+?)\b(a3d_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if not m:
            raise RuntimeError(f"animate3d_hip.h: cannot read {' '.join(decl.split())!r} as a declaration")
        params = [] if m[3].strip() == "void" else m[3].split(",")
        functions[m[2]] = (_c_type(m[1], structs, named=False)[0], [_c_type(p, structs)[0] for p in params])
    return Header(functions, constants, structs)


def read_header(path: str) -> Header:
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise RuntimeError(f"{path}: the C header that types the library cannot be read ({e.strerror})") from e


_HEADER = read_header(_HEADER_PATH)
EXPORTED_SYMBOLS = tuple(_HEADER.functions)
globals().update(_HEADER.constants)          # A3D_EINVAL, A3D_GEMM_RING, A3D_ATTN_PLAIN, A3D_BF16, ...: each under the header's name
STAGE_ADAM_MAX_TENSORS, STAGE_ADAM_BEGIN, STAGE_ADAM_CHECK, STAGE_ADAM_UPDATE = (
    A3D_STAGE_ADAM_MAX_TENSORS, A3D_STAGE_ADAM_BEGIN, A3D_STAGE_ADAM_CHECK, A3D_STAGE_ADAM_UPDATE)   # noqa: F821
_DTYPE_CODE = {torch.float32: A3D_F32, torch.bfloat16: A3D_BF16, torch.float16: A3D_F16}          # noqa: F821


@dataclass(frozen=True)
class RowMap:
    """row(g, s) = (g // gdiv) * ga + (g % gdiv) * gb + (s // seg_len) * seg_stride + s % seg_len
    (include/animate3d_hip.h: a3d_rowmap).  ``ld`` comes from the tensor it is applied to."""
    gdiv: int
    ga: int
    gb: int
    seg_len: int
    seg_stride: int

    def c(self, ld: int) -> _RowMapC:
        return _RowMapC(self.gdiv, self.ga, self.gb, self.seg_len, self.seg_stride, ld)


def rowmap_rows(m: RowMap, groups: int, step: int, length: int, device="cpu") -> torch.Tensor:
    """Rows ``m`` addresses for groups 0, step, 2 step, ... < groups and positions 0 .. length-1, in (group, position) order."""
    g = torch.arange(0, groups, step, device=device).view(-1, 1)
    s = torch.arange(length, device=device).view(1, -1)
    return ((g // m.gdiv) * m.ga + (g % m.gdiv) * m.gb + (s // m.seg_len) * m.seg_stride + s % m.seg_len).reshape(-1)


def rowmap_covers(m: RowMap, groups: int, step: int, length: int, rows: int, device="cpu") -> bool:
    """True when those rows are ALL of 0 .. rows-1, each exactly once: an attention backward whose key map covers K / V writes every row of
    dK / dV, so they need no zero fill (the first-frame maps, which read frame 0 only, do not cover)."""
    if (groups + step - 1) // step * length != rows:
        return False
    idx = rowmap_rows(m, groups, step, length, device)
    return bool(int(idx.min()) >= 0 and int(idx.max()) < rows and torch.unique(idx).numel() == rows)


# ---- the up-sampling conv's phase form (a3d_conv3x3_up2x_folded): pack-time weight folding and the shapes it serves
# taps of one axis that read window position r of phase a: UP2X_TAPS[a][r]  (R_0(0) = {0}, R_0(1) = {1, 2}, R_1(0) = {0, 1}, R_1(1) = {2})
UP2X_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


def fold_up2x_sums(w: torch.Tensor) -> torch.Tensor:
    """float64 [4, Cout, 4 Cin] tap sums of a packed 3x3 weight ``w`` [Cout, 9 Cin] (ky, kx, ci), on the host and UNROUNDED: phase
    p = 2a + b of output pixel (2i + a, 2j + b), a row ordered window position (r, c) then ci (include/animate3d_hip.h)."""
    Cout, K9 = w.shape
    if K9 % 9:
        raise ValueError(f"a packed 3x3 weight has 9 Cin columns, got {tuple(w.shape)}")
    w64 = w.detach().to(device="cpu", dtype=torch.float64).view(Cout, 3, 3, K9 // 9)
    wf = torch.zeros((4, Cout, 2, 2, K9 // 9), dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for c in range(2):
                    for ky in UP2X_TAPS[a][r]:
                        for kx in UP2X_TAPS[b][c]:
                            wf[2 * a + b, :, r, c] += w64[:, ky, kx]
    return wf.view(4, Cout, 4 * (K9 // 9))


def round_once(x64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> bf16 / fp16 with ONE round-to-nearest-even.  torch converts through float32, and two roundings to nearest can land one
    ulp off the single one, so the float32 step rounds to odd instead (truncate, last bit = sticky): float32 keeps 13 bits more than either
    16-bit type, which makes the second, nearest-even rounding exact."""
    f = x64.to(torch.float32)
    inexact = f.to(torch.float64) != x64
    over = f.to(torch.float64).abs() > x64.abs()
    f = torch.where(over, torch.nextafter(f, torch.zeros_like(f)), f)
    bits = f.view(torch.int32) | inexact.to(torch.int32)
    return bits.view(torch.float32).to(dtype)


def fold_up2x_weights(w: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The folded weight [4, Cout, 4 Cin] of ``HipOps.conv3x3(..., folded=)`` for the packed 3x3 weight ``w`` [Cout, 9 Cin]: tap sums in
    float64 on the host, rounded once to ``dtype`` (default: w's), on w's device.  A pack-time operation: never call it per forward."""
    return round_once(fold_up2x_sums(w), dtype or w.dtype).to(w.device).contiguous()


def up2x_folded_applies(B: int, H: int, W: int, Cin: int, Cout: int, *, up2x: bool, up_size=None, stride: int = 1, rowbias=None,
                        residual=None, folded=None, tile128: bool = False, shape_independent: bool = False) -> bool:
    """True when ``HipOps.conv3x3`` takes the phase-form entry point: folded weights are given, the output is the exact (2H, 2W) —
    the cropped sizes' border groups would hold in-image taps — there is no row bias or residual, and the persistent kernel takes the
    shape (a3d_conv3x3_up2x_folded's rules).  ``shape_independent``: the caller compares runs of different row counts bit for bit
    (``HipOps.split_k`` off); whether a shape qualifies depends on its row count, so such runs keep the nine-tap kernel."""
    if folded is None or not up2x or stride != 1 or rowbias is not None or residual is not None or tile128 or shape_independent:
        return False
    if up_size is not None and (int(up_size[0]), int(up_size[1])) != (2 * H, 2 * W):
        return False
    if (B * H * W) % 256 or Cin % 64 or (Cout % 320 and Cout % 256):
        return False
    return (B * H * W + 2 * W + 2) * Cin * 2 < 1 << 32


def lib_path() -> str:
    return _LIB_PATH


def load_library():
    """dlopen the in-tree library and type every entry point as include/animate3d_hip.h declares it.  Raises if either is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} is missing: run `python -m animate3d_amd.build` (or __graft_entry__.build()). "
                               "There is no CPU fallback for the MI355X kernels.")
        functions = read_header(_HEADER_PATH).functions
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in functions.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


GN_PLAN_FIELDS = ("fused", "sg", "nx", "ny", "threads", "rmax", "stream")


def group_norm_plan(rows: int, C: int, groups: int) -> dict:
    """How a3d_group_norm runs a one-source instance (a3d_group_norm_plan: host only, needs no GPU): the fields of GN_PLAN_FIELDS, plus
    ``iters`` = rows a thread of the one-launch kernel owns at most."""
    out = (c_int * len(GN_PLAN_FIELDS))()
    _check(load_library().a3d_group_norm_plan(rows, C, groups, out), f"a3d_group_norm_plan rows={rows} C={C} groups={groups}")
    plan = dict(zip(GN_PLAN_FIELDS, out))
    plan["iters"] = -(-rows // plan["ny"]) if plan["fused"] else 0
    return plan


def _check(rc: int, what: str):
    if rc != 0:
        kind = {A3D_EINVAL: "A3D_EINVAL (shape/alignment precondition)", A3D_EUNSUPPORTED: "A3D_EUNSUPPORTED"}.get(rc, f"hipError {rc}")  # noqa: F821
        raise RuntimeError(f"{what} failed: {kind}")


def call(lib, name: str, stream, args, what: str = "", tolerate=()):
    """The one way a launching entry point is called: ``name(stream, *args)`` of ``lib``, which is the loaded library or the ``_Entry`` of
    an op set (``args`` comes as the caller's tuple: this runs thousands of times per forward).  A return code other than 0 and those of ``tolerate`` raises, naming the symbol that ran (an ``_Entry`` has resolved the
    storage twin) and ``what``, the caller's shapes.  Returns the code."""
    fn = getattr(lib, name)
    rc = fn(stream, *args)
    if rc != 0 and rc not in tolerate:
        _check(rc, f"{fn.__name__} {what}" if what else fn.__name__)
    return rc


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def on_model_device(method):
    """Decorator for the entry points of a module that owns a ``HipOps``: the C-ABI launches on the CURRENT device's stream
    (``torch.cuda.current_stream``) and allocates there, so a model living on cuda:1 must run with cuda:1 current.  One
    process per GPU is the deployment model; this makes a second device in one process work as well."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        dev = self.device
        if dev.type == "cuda" and torch.cuda.current_device() != (dev.index if dev.index is not None else torch.cuda.current_device()):
            with torch.cuda.device(dev):
                return method(self, *args, **kwargs)
        return method(self, *args, **kwargs)
    return wrapper


class _Entry:
    """Entry points of one storage type as plain attributes: ``a3d_gemm_bf16`` is the library's ``a3d_gemm_f16`` for an fp16 op set, and
    so is every name whose ``_f16`` twin the header declares (``a3d_im2col_in`` -> ``a3d_im2col_in_f16``)."""

    def __init__(self, lib, f16: bool):
        for name in EXPORTED_SYMBOLS:
            twin = (name[:-5] if name.endswith("_bf16") else name) + "_f16"
            setattr(self, name, getattr(lib, twin if f16 and twin in EXPORTED_SYMBOLS else name))


class HipOps:
    """The op set of the denoise step, executed by the gfx950 kernels.  All activations are 2-D ``[rows, C]`` CUDA tensors
    (NHWC images flattened to rows) in the op set's storage type: bf16 (default) or IEEE fp16 (``act_dtype=torch.float16``:
    what a model cast with ``.half()`` gets, as the reference's 4D-SDS caller does, animatemv_guidance.py:339-346).  Both use
    fp32 accumulation, statistics and softmax; an fp16 model keeps 11 significant bits where bf16 keeps 8."""

    has_attn_lse = True      # flash_attn(with_lse=True) / flash_attn_bwd(o=..., lse=...): see autograd_ops._FlashAttn
    has_up2x_folded = True   # conv3x3(..., folded=): the packs of unet.py / vae.py fold the up-sampling weights for op sets that say so

    def __init__(self, device: Optional[torch.device] = None, act_dtype: torch.dtype = torch.bfloat16, split_k: bool = True):
        """``split_k`` = False: only kernels whose results do not depend on the launch shape (bit-for-bit batch independence, a sharded forward
        bit-equal to the unsharded one); True (default): the small-M / long-K convolutions and linears split their K sum over idle CUs —
        deterministic per launch shape, equal to the unsplit kernels to fp32 summation order."""
        if not torch.cuda.is_available():
            raise RuntimeError("HipOps needs a visible MI355X (torch.cuda.is_available() is False); no CPU fallback exists")
        if act_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"storage type {act_dtype} is not supported (bfloat16 or float16)")
        self.raw_lib = load_library()
        self._kv_row_cache = {}
        self._kv_cover_cache = {}      # _shared_kv_rows
        self.act_dtype = act_dtype
        self.lib = _Entry(self.raw_lib, act_dtype == torch.float16)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # compute units the persistent GEMM / conv kernels leave free for concurrently running kernels: passed with EVERY launch (the flags
        # word of a3d_gemm / a3d_gemm_geglu / a3d_conv3x3) — the library keeps no state.  Set by animate3d_amd.parallel while an RCCL
        # all-gather is in flight; a HIP graph captured meanwhile replays with the value of its capture.
        self.reserved_cus = 0
        # split-K of the small-M / long-K GEMMs and convs (UNet levels 2 / 3, the whole 4D-SDS shape): on by default; results then agree
        # with the unsplit kernels to fp32 summation order only, so runs that are compared BIT FOR BIT across different row counts
        # (a sharded forward against the unsharded one: animate3d_amd.parallel turns it off) must not use it
        self.split_k = bool(split_k)
        # ... of dense GEMMs too: off.  Measured (profiles/r5_microbench_splitk.log): the mid-block convolutions (K = 11 520 ... 23 040) gain
        # 13-55 %, but the level-2 / 3 linears (K <= 5 120, 35-120 us per launch) LOSE 20-100 %: 84 MB of fp32 partials written and read
        # back plus a second launch cost more than the idle CUs return.  The entry point and its tests stay (a3d_gemm_ws_*).
        self.split_k_gemm = False
        # diagnostics (a3d_flash_attn_counted): an int32 device tensor of 3 words that every plain ``flash_attn`` call adds to while it is set —
        # [0] workgroups of the LDS-DMA staged attention kernels sent to the exact pass by the fp16 spread vote, [1] exact re-runs after an
        # overflow of the max-free pass, [2] workgroups launched.  None (default): the plain entry point.
        self.attn_counters = None
        self._ws_plan = {}           # launch shape -> split-K workspace bytes (0: the shape does not split)
        self._ws_bufs = {}           # stream handle -> ONE split-K workspace per stream, grown to the largest need (launches on one stream
                                     # run in order, so consecutive split launches may share it; a fresh 100-MB torch.empty per call was the
                                     # alternative).  Per stream: two streams sharing one buffer would overwrite each other's partials.

    def _workspace(self, need: int) -> torch.Tensor:
        if torch.cuda.is_current_stream_capturing():
            # a captured graph keeps the pointer for every replay: a buffer of its own, from the graph's private pool, that lives as long as
            # the graph — the eager buffer may be regrown (and its memory handed to another tensor) after the capture
            return torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=self.device)
        stream = self._stream()
        buf = self._ws_bufs.get(stream)
        if buf is None or buf.numel() < need:
            buf = self._ws_bufs[stream] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=self.device)
        return buf

    def _gemm_flags(self, tile128: bool, ring: bool = False) -> int:
        r = int(self.reserved_cus)
        if not 0 <= r <= 0xFF:
            raise ValueError(f"reserved_cus = {self.reserved_cus}: the flags word of a3d_gemm / a3d_conv3x3 carries 0..255 reserved compute units")
        return r | (A3D_GEMM_TILE128 if tile128 else (A3D_GEMM_RING if ring else 0))    # noqa: F821

    # ---- helpers
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _launch(self, name: str, *args, what: str = "", tolerate=()):
        """``call`` on this op set's stream (``_stream()`` spelled out: a frame less per launch); ``name`` is the bf16 spelling, ``self.lib``
        holds the storage twin under it."""
        return call(self.lib, name, torch.cuda.current_stream(self.device).cuda_stream, args, what, tolerate)

    def _split_k(self, name: str, key, args, what: str) -> bool:
        """The split-K sequence of ``name`` (a3d_gemm_ws / a3d_conv3x3_ws): ask once per launch shape ``key`` how many workspace bytes a
        split launch of exactly ``args`` needs, then run it on the stream's workspace.  False: the shape does not split, nothing ran."""
        need = self._ws_plan.get(key)
        if need is None:
            q = c_i64(0)
            self._launch(name, *args, None, 0, ctypes.byref(q), what="(query) " + what)
            need = self._ws_plan[key] = int(q.value)
        if need > 0:
            self._launch(name, *args, _p(self._workspace(need)), need, None, what=what)
        return need > 0

    def _f32(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _gn_workspace(self, B: int, rows: int, groups: int) -> torch.Tensor:
        return self._f32(int(self.lib.a3d_group_norm_ws_floats(B, rows, groups)))

    def _act(self, t: torch.Tensor, name: str):
        if t.dtype != self.act_dtype or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"{name}: expected a 2-D {self.act_dtype} CUDA tensor with contiguous rows, got {t.dtype} {tuple(t.shape)} {t.device} strides {t.stride()}")
        return t

    def split_cols(self, x, *bounds):
        """The column pieces [bounds[i], bounds[i+1]) of a fused projection output as views (the differentiable op set overrides
        this: autograd_ops.AutogradOps.split_cols collects the pieces' gradients in one buffer)."""
        return tuple(x[:, a:b] for a, b in zip(bounds[:-1], bounds[1:]))

    def empty(self, rows: int, cols: int) -> torch.Tensor:
        return torch.empty((rows, cols), dtype=self.act_dtype, device=self.device)

    # ---- GEMM family
    def gemm(self, x, w, bias=None, *, residual=None, alpha: float = 1.0, beta: float = 1.0, rowbias=None, rb_div: int = 1, out=None,
             tile128: bool = False, ring: bool = False):
        """``tile128`` forces the register-staged 128 x 128-tile kernel (A3D_GEMM_TILE128), ``ring`` the LDS-DMA ring kernel where the shape
        allows it (A3D_GEMM_RING): bit-identical results; parity tests and A/B timing."""
        x, w = self._act(x, "gemm.x"), self._act(w, "gemm.w")
        M, K = x.shape
        N = w.shape[0]
        assert w.shape[1] == K, (x.shape, w.shape)
        y = out if out is not None else self.empty(M, N)
        self._act(y, "gemm.out")
        if residual is not None:
            self._act(residual, "gemm.residual")
            assert residual.shape == (M, N)
        if rowbias is not None:
            self._act(rowbias, "gemm.rowbias")
            assert rowbias.is_contiguous() and rowbias.shape[1] == N
        if bias is not None:
            assert bias.dtype == torch.float32 and bias.numel() == N
        flags = self._gemm_flags(tile128, ring)
        args = (_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(rowbias), rb_div,
                _p(residual), residual.stride(0) if residual is not None else 0, _p(y), y.stride(0), M, N, K, alpha, beta, flags)
        what = f"M={M} N={N} K={K}"
        if self.split_k and self.split_k_gemm and not tile128 and M <= 32768 and K >= 1152:
            key = ("gemm", M, N, K, x.stride(0), w.stride(0), y.stride(0), rb_div if rowbias is not None else 0, flags)
            if self._split_k("a3d_gemm_ws_bf16", key, args, what):
                return y
        self._launch("a3d_gemm_bf16", *args, what=what)
        return y

    def gemm2(self, xa, xb, w, bias=None):
        """``[xa | xb] w^T + bias`` without the concatenation (a3d_gemm2: the 1x1 shortcut conv of an up-block ResNet).  None when the
        persistent kernel does not take the shape — the caller then concatenates and calls ``gemm``."""
        xa, xb, w = self._act(xa, "gemm2.xa"), self._act(xb, "gemm2.xb"), self._act(w, "gemm2.w")
        M, K1 = xa.shape
        K = K1 + xb.shape[1]
        N = w.shape[0]
        assert xb.shape[0] == M and w.shape[1] == K
        if K1 % 64 or K % 64 or N % 8:
            return None
        y = self.empty(M, N)
        rc = self._launch("a3d_gemm2_bf16", _p(xa), xa.stride(0), _p(xb), xb.stride(0), K1, _p(w), w.stride(0), _p(bias), _p(y), y.stride(0),
                          M, N, K, self._gemm_flags(False), what=f"M={M} N={N} K={K1}+{K - K1}", tolerate=(A3D_EUNSUPPORTED,))   # noqa: F821
        return None if rc else y

    @staticmethod
    def interleave_geglu(w: torch.Tensor) -> torch.Tensor:
        """[2N, ...] = [h rows | gate rows] -> rows interleaved in blocks of 32 (layout a3d_gemm_geglu_bf16 expects)."""
        n = w.shape[0] // 2
        assert n % 32 == 0
        h, g = w[:n].reshape(n // 32, 32, *w.shape[1:]), w[n:].reshape(n // 32, 32, *w.shape[1:])
        return torch.stack([h, g], dim=1).reshape(w.shape).contiguous()

    def gemm_geglu(self, x, w_il, bias_il, *, tile128: bool = False):
        """GEGLU(x) = (x Wh^T + bh) * gelu(x Wg^T + bg) with interleaved weights (see interleave_geglu)."""
        x, w_il = self._act(x, "geglu.x"), self._act(w_il, "geglu.w")
        M, K = x.shape
        N2 = w_il.shape[0]
        y = self.empty(M, N2 // 2)
        self._launch("a3d_gemm_geglu_bf16", _p(x), x.stride(0), _p(w_il), w_il.stride(0), _p(bias_il), _p(y), y.stride(0), M, N2, K,
                     self._gemm_flags(tile128), what=f"M={M} N2={N2} K={K}")
        return y

    def conv3x3(self, x, B: int, H: int, W: int, w, bias, *, stride: int = 1, up2x: bool = False, rowbias=None, rb_div: int = 1, residual=None,
                up_size=None, tile128: bool = False, folded=None):
        """x [B*H*W, Cin] -> (y [B*Ho*Wo, Cout], Ho, Wo); w packed [Cout, 9*Cin] (ky, kx, ci).  ``up_size`` = (Ho, Wo) forces
        the size of the nearest upsampling in front of the conv (2H or 2H-1, likewise W: unet_motion_mv_model.py:831-837).
        ``folded`` = ``fold_up2x_weights(w)`` [4, Cout, 4*Cin] (inference packs): the up-sampling conv runs in its 2x2 phase form, 16 MACs
        per output pixel instead of 36, wherever ``up2x_folded_applies``; everywhere else this is the nine-tap kernel on ``w``."""
        x, w = self._act(x, "conv.x"), self._act(w, "conv.w")
        Cin = x.shape[1]
        Cout = w.shape[0]
        assert x.is_contiguous() and w.is_contiguous() and x.shape[0] == B * H * W and w.shape[1] == 9 * Cin
        if up2x_folded_applies(B, H, W, Cin, Cout, up2x=up2x, up_size=up_size, stride=stride, rowbias=rowbias, residual=residual,
                               folded=folded, tile128=tile128, shape_independent=not self.split_k):
            assert folded.dtype == self.act_dtype and folded.is_cuda and folded.is_contiguous() and folded.shape == (4, Cout, 4 * Cin)
            if bias is not None:
                assert bias.dtype == torch.float32 and bias.numel() == Cout
            y = self.empty(4 * B * H * W, Cout)
            self._launch("a3d_conv3x3_up2x_folded_bf16", _p(x), _p(folded), _p(bias), None, None, _p(y), B, H, W, Cin, Cout,
                         self._gemm_flags(False), what=f"B={B} H={H} W={W} Cin={Cin} Cout={Cout}")
            return y, 2 * H, 2 * W
        He, We = (2 * H, 2 * W) if up2x else (H, W)
        up_code = 1 if up2x else 0
        if up_size is not None:
            if not up2x or up_size[0] not in (2 * H, 2 * H - 1) or up_size[1] not in (2 * W, 2 * W - 1):
                raise ValueError(f"forced upsample size {tuple(up_size)} is not reachable from {(H, W)} (2x or 2x - 1 per axis)")
            He, We = int(up_size[0]), int(up_size[1])
            up_code |= (2 if He == 2 * H - 1 else 0) | (4 if We == 2 * W - 1 else 0)
        Ho, Wo = (He - 1) // stride + 1, (We - 1) // stride + 1
        y = self.empty(B * Ho * Wo, Cout)
        if residual is not None:
            assert residual.is_contiguous() and residual.shape == y.shape
        if rowbias is not None:
            assert rowbias.is_contiguous() and rowbias.shape[1] == Cout
        flags = self._gemm_flags(tile128)
        args = (_p(x), _p(w), _p(bias), _p(rowbias), rb_div, _p(residual), _p(y), B, H, W, Cin, Cout, stride, up_code, flags)
        what = f"B={B} H={H} W={W} Cin={Cin} Cout={Cout} stride={stride} up={up2x}"
        if self.split_k and not tile128 and B * Ho * Wo <= 32768:
            key = ("conv", B, H, W, Cin, Cout, stride, up_code, rb_div if rowbias is not None else 0, flags)
            if self._split_k("a3d_conv3x3_ws_bf16", key, args, what):
                return y, Ho, Wo
        self._launch("a3d_conv3x3_bf16", *args, what=what)
        return y, Ho, Wo

    # ---- attention
    def flash_attn(self, q, k, v, qmap: RowMap, kmap: RowMap, groups: int, heads: int, q_len: int, kv_len: int, *,
                   out=None, out_scale: float = 1.0, accumulate: bool = False, causal: bool = False, with_lse: bool = False,
                   accumulation_target: bool = False, exact: bool = False, plain: bool = False):
        """``exact`` (A3D_ATTN_EXACT): the LDS-DMA staged kernels skip their max-free first pass; ``plain`` (A3D_ATTN_PLAIN): the generic
        kernel of the short / ragged shapes — per-call choices for the parity tests and A/B timing, results agree to rounding.
        ``accumulation_target`` is a hint for the autograd op set (autograd_ops.AutogradOps.flash_attn), ignored here.  ``with_lse``: returns (o, lse2) with lse2 [groups, heads, q_len] fp32 = log2 of every query's softmax denominator (training:
        ``flash_attn_bwd(stats=...)`` then skips its statistics pass)."""
        q, k, v = self._act(q, "attn.q"), self._act(k, "attn.k"), self._act(v, "attn.v")
        C = q.shape[1]
        D = C // heads
        assert k.stride(0) == v.stride(0)
        o = out if out is not None else self.empty(q.shape[0], C)
        qm, km, om = qmap.c(q.stride(0)), kmap.c(k.stride(0)), qmap.c(o.stride(0))
        flags = ((A3D_ATTN_ACCUMULATE if accumulate else 0) | (A3D_ATTN_CAUSAL if causal else 0) | (A3D_ATTN_EXACT if exact else 0)
                 | (A3D_ATTN_PLAIN if plain else 0))                                                                       # noqa: F821
        name, last = "a3d_flash_attn_bf16", ()            # the _lse and _counted entry points take one more pointer
        if with_lse:
            lse = self._f32(groups, heads, q_len)
            name, last = "a3d_flash_attn_lse_bf16", (_p(lse),)
        elif self.attn_counters is not None:
            cnt = self.attn_counters
            assert cnt.dtype == torch.int32 and cnt.is_cuda and cnt.numel() >= 3 and cnt.is_contiguous()
            name, last = "a3d_flash_attn_counted_bf16", (_p(cnt),)
        self._launch(name, _p(q), _p(k), _p(v), _p(o), ctypes.byref(qm), ctypes.byref(km), ctypes.byref(om), groups, heads, D, q_len, kv_len,
                     float(D) ** -0.5, out_scale, flags, *last, what=f"groups={groups} heads={heads} D={D} q_len={q_len} kv_len={kv_len}")
        return (o, lse) if with_lse else o

    def flash_attn2(self, q, k, v, k2, v2, qmap: RowMap, kmap: RowMap, kmap2: RowMap, groups: int, heads: int, q_len: int, kv_len: int,
                    kv_len2: int, *, out_scale2: float = 1.0):
        """attn(q, k, v) + out_scale2 * attn(q, k2, v2) in one launch (each key set with its own softmax); None when the head
        dimension has no fused kernel (the caller then issues two ``flash_attn`` calls)."""
        D = q.shape[1] // heads
        if D not in (40, 80):
            return None
        q, k, v, k2, v2 = self._act(q, "attn.q"), self._act(k, "attn.k"), self._act(v, "attn.v"), self._act(k2, "attn.k2"), self._act(v2, "attn.v2")
        assert k.stride(0) == v.stride(0) and k2.stride(0) == v2.stride(0)
        o = self.empty(q.shape[0], q.shape[1])
        qm, km, km2, om = qmap.c(q.stride(0)), kmap.c(k.stride(0)), kmap2.c(k2.stride(0)), qmap.c(o.stride(0))
        self._launch("a3d_flash_attn2_bf16", _p(q), _p(k), _p(v), _p(k2), _p(v2), _p(o), ctypes.byref(qm), ctypes.byref(km),
                     ctypes.byref(km2), ctypes.byref(om), groups, heads, D, q_len, kv_len, kv_len2, float(D) ** -0.5, 1.0, out_scale2, 0,
                     what=f"groups={groups} heads={heads} D={D} q_len={q_len} kv_len={kv_len} kv_len2={kv_len2}")
        return o

    def temporal_attn(self, q, k, v, videos: int, frames: int, L: int, heads: int, *, q_f0: int = 0, q_frames: Optional[int] = None,
                      out=None):
        """Unsharded: q / k / v rows ((v F + f) L + l).  Frame-sharded (``q_frames`` < ``frames``): q holds this rank's frames
        [q_f0, q_f0 + q_frames) only; k / v are the all-gathered tensors ``[frames / q_frames blocks, videos * q_frames * L, C]``."""
        q, k, v = self._act(q, "tattn.q"), self._act(k, "tattn.k"), self._act(v, "tattn.v")
        C = q.shape[1]
        D = C // heads
        assert k.stride(0) == v.stride(0)
        o = self._act(out, "tattn.out") if out is not None else self.empty(q.shape[0], C)
        assert o.shape == (q.shape[0], C)
        what = f"videos={videos} frames={frames} L={L} D={D} q_f0={q_f0} q_frames={q_frames}"
        if q_frames is None or q_frames == frames:
            assert q.stride(0) == k.stride(0)
            self._launch("a3d_temporal_attn_bf16", _p(q), _p(k), _p(v), q.stride(0), _p(o), o.stride(0), videos, frames, L, heads, D,
                         float(D) ** -0.5, what=what)
        else:
            assert q.shape[0] == videos * q_frames * L and k.shape[0] == videos * frames * L
            self._launch("a3d_temporal_attn_sharded_bf16", _p(q), q.stride(0), _p(k), _p(v), k.stride(0), _p(o), o.stride(0), videos, frames, L,
                         heads, D, float(D) ** -0.5, q_f0, q_frames, q_frames, videos * q_frames * L, what=what)
        return o

    # ---- normalisation
    def group_norm(self, x, B: int, rows: int, gamma, beta, groups: int, eps: float, silu: bool):
        x = self._act(x, "gn.x")
        assert x.is_contiguous() and x.shape[0] == B * rows
        C = x.shape[1]
        y = self.empty(x.shape[0], C)
        ws = self._gn_workspace(B, rows, groups)
        self._launch("a3d_group_norm_bf16", _p(x), _p(y), _p(gamma), _p(beta), _p(ws), B, rows, C, groups, eps, 1 if silu else 0,
                     what=f"B={B} rows={rows} C={C}")
        return y

    def group_norm2(self, xa, xb, B: int, rows: int, gamma, beta, groups: int, eps: float, silu: bool):
        """GroupNorm (+ SiLU) of ``cat([xa, xb], 1)`` read from its two parts (a3d_group_norm2)."""
        xa, xb = self._act(xa, "gn2.xa"), self._act(xb, "gn2.xb")
        assert xa.is_contiguous() and xb.is_contiguous() and xa.shape[0] == B * rows == xb.shape[0]
        Ca, Cb = xa.shape[1], xb.shape[1]
        y = self.empty(xa.shape[0], Ca + Cb)
        ws = self._gn_workspace(B, rows, groups)
        self._launch("a3d_group_norm2_bf16", _p(xa), Ca, _p(xb), Cb, _p(y), _p(gamma), _p(beta), _p(ws), B, rows, groups, eps, 1 if silu else 0,
                     what=f"B={B} rows={rows} C={Ca}+{Cb}")
        return y

    def group_norm_sums(self, x, B: int, rows: int, groups: int) -> torch.Tensor:
        """fp64 [B, groups, 2] = (sum, sum of squares) of this rank's rows (first half of a GroupNorm spread over ranks)."""
        x = self._act(x, "gn.x")
        assert x.is_contiguous() and x.shape[0] == B * rows
        ws = self._gn_workspace(B, rows, groups)
        sums = torch.empty((B, groups, 2), dtype=torch.float64, device=self.device)
        self._launch("a3d_group_norm_sums_bf16", _p(x), _p(ws), _p(sums), B, rows, x.shape[1], groups, what=f"B={B} rows={rows} C={x.shape[1]}")
        return sums

    def group_norm_apply(self, x, B: int, rows: int, gamma, beta, groups: int, stats: torch.Tensor, silu: bool):
        """Second half: ``stats`` fp32 [B, groups, 2] = (mean, rstd)."""
        x = self._act(x, "gn.x")
        assert x.is_contiguous() and x.shape[0] == B * rows
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape == (B, groups, 2)
        y = self.empty(x.shape[0], x.shape[1])
        self._launch("a3d_group_norm_apply_bf16", _p(x), _p(y), _p(gamma), _p(beta), _p(stats), B, rows, x.shape[1], groups, 1 if silu else 0,
                     what=f"B={B} rows={rows} C={x.shape[1]}")
        return y

    def layer_norm(self, x, gamma, beta, eps: float, pe1=None, pe1_div: int = 1, pe2=None, pe2_div: int = 1, two: bool = False):
        """y1 = LN(x) + pe1[(m // pe1_div) % len(pe1)]; with two=True also y2 with pe2."""
        x = self._act(x, "ln.x")
        assert x.is_contiguous()
        M, C = x.shape
        y1 = self.empty(M, C)
        y2 = self.empty(M, C) if two else None
        for pe in (pe1, pe2):
            if pe is not None:
                self._act(pe, "ln.pe")
                assert pe.is_contiguous() and pe.shape[1] == C
        self._launch("a3d_layer_norm_bf16", _p(x), _p(y1), _p(y2), _p(gamma), _p(beta), M, C, eps,
                     _p(pe1), pe1_div, pe1.shape[0] if pe1 is not None else 1,
                     _p(pe2), pe2_div, pe2.shape[0] if pe2 is not None else 1, what=f"M={M} C={C}")
        return (y1, y2) if two else y1

    # ---- elementwise / layout
    def geglu(self, x):
        x = self._act(x, "geglu.x")
        M, N2 = x.shape
        y = self.empty(M, N2 // 2)
        self._launch("a3d_geglu_bf16", _p(x), x.stride(0), _p(y), y.stride(0), M, N2 // 2)
        return y

    def silu(self, x):
        x = self._act(x, "silu.x")
        assert x.is_contiguous()
        y = torch.empty_like(x)
        self._launch("a3d_silu_bf16", _p(x), _p(y), x.numel())
        return y

    def activation(self, x, kind: str):
        """``kind``: "silu", "quick_gelu" (x * sigmoid(1.702 x)) or "gelu" (erf)."""
        x = self._act(x, "act.x")
        assert x.is_contiguous()
        y = torch.empty_like(x)
        self._launch("a3d_activation_bf16", _p(x), _p(y), x.numel(), {"silu": 0, "quick_gelu": 1, "gelu": 2}[kind], what=kind)
        return y

    def concat(self, a, b):
        a, b = self._act(a, "concat.a"), self._act(b, "concat.b")
        assert a.is_contiguous() and b.is_contiguous() and a.shape[0] == b.shape[0]
        y = self.empty(a.shape[0], a.shape[1] + b.shape[1])
        self._launch("a3d_concat_bf16", _p(a), a.shape[1], _p(b), b.shape[1], _p(y), a.shape[0])
        return y

    def timestep_embed(self, t: torch.Tensor, dim: int):
        assert t.dtype == torch.float32 and t.is_cuda and t.dim() == 1
        y = self.empty(t.shape[0], dim)
        self._launch("a3d_timestep_embed_bf16", _p(t), _p(y), t.shape[0], dim)
        return y

    def im2col_in(self, sample: torch.Tensor):
        """[V, C, F, H, W] (fp32/bf16/fp16) -> [(V F) H W, 64] bf16 3x3 patches."""
        assert sample.is_cuda and sample.dim() == 5 and sample.dtype in _DTYPE_CODE
        sample = sample.contiguous()
        V, C, F, H, W = sample.shape
        y = self.empty(V * F * H * W, 64)
        self._launch("a3d_im2col_in", _p(sample), _DTYPE_CODE[sample.dtype], _p(y), V, C, F, H, W)
        return y

    def unpack_out(self, x, V: int, C: int, F: int, H: int, W: int, dtype: torch.dtype):
        x = self._act(x, "unpack.x")
        assert x.is_contiguous() and x.shape == (V * F * H * W, C)
        y = torch.empty((V, C, F, H, W), dtype=dtype, device=self.device)
        self._launch("a3d_unpack_out", _p(x), _p(y), _DTYPE_CODE[dtype], V, C, F, H, W)
        return y

    def gemm_f32out(self, x, w, bias=None, alpha: float = 1.0):
        """fp32 Y = alpha * (x w^T + bias) for logits that must not be rounded to bf16 (VAE mid-block attention)."""
        x, w = self._act(x, "gemm_f32out.x"), self._act(w, "gemm_f32out.w")
        M, K = x.shape
        N = w.shape[0]
        assert x.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        self._launch("a3d_gemm_f32out_bf16", _p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(y), N, M, N, K, alpha, what=f"M={M} N={N} K={K}")
        return y

    def softmax_rows(self, x, out=None):
        """fp32 logits [M, N] -> bf16 row softmax (``out``: [M, N] view with its own row stride)."""
        assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
        M, N = x.shape
        y = self._act(out, "softmax_rows.out") if out is not None else self.empty(M, N)
        assert y.shape == (M, N)
        self._launch("a3d_softmax_rows_f32_bf16", _p(x), N, _p(y), y.stride(0), M, N, what=f"M={M} N={N}")
        return y

    def channel_mix(self, x, w, bias, scale: float = 1.0):
        """planar fp32 [B, Cin, H, W] -> [B, Cout, H, W]: scale * (w x) + bias per pixel (<= 8 channels)."""
        assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        w = w.to(device=x.device, dtype=torch.float32).contiguous()
        b = None if bias is None else bias.to(device=x.device, dtype=torch.float32).contiguous()
        y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
        self._launch("a3d_channel_mix_f32", _p(x), _p(w), _p(b), _p(y), B, Cin, Cout, H * W, scale)
        return y

    # ---- VAE encoder input gradient (4D-SDS: vae_grad.py)
    def im2col_in_bwd(self, dcol, V: int, C: int, F: int, H: int, W: int, scale: float = 1.0):
        """Adjoint of ``im2col_in``: dCol [(V F) H W, 64] (storage type) -> fp32 [V, C, F, H, W] = scale * col2im(dCol)."""
        dcol = self._act(dcol, "im2col_in_bwd.dcol")
        assert dcol.is_contiguous() and dcol.shape == (V * F * H * W, 64)
        dx = self._f32(V, C, F, H, W)
        self._launch("a3d_im2col_in_bwd", _p(dcol), _p(dx), V, C, F, H, W, scale, what=f"V={V} C={C} F={F} H={H} W={W}")
        return dx

    def softmax_rows_bwd(self, p, dp, alpha: float = 1.0, out=None):
        """dS = alpha * P o (dP - rowsum(P o dP)) for probabilities ``p`` [M, N] (storage type, own row stride) and fp32 ``dp`` [M, N];
        ``out``: [M, N] view with its own row stride."""
        p = self._act(p, "softmax_rows_bwd.p")
        assert dp.dtype == torch.float32 and dp.is_cuda and dp.stride(1) == 1 and dp.shape == p.shape
        M, N = p.shape
        y = self._act(out, "softmax_rows_bwd.out") if out is not None else self.empty(M, N)
        assert y.shape == (M, N)
        self._launch("a3d_softmax_rows_bwd_bf16", _p(p), p.stride(0), _p(dp), dp.stride(0), _p(y), y.stride(0), M, N, alpha, what=f"M={M} N={N}")
        return y

    # ---- training path: backward kernels (reference: torch autograd behind train.py:576-590) and the optimiser step
    def flash_attn_bwd(self, q, k, v, do, qmap: RowMap, kmap: RowMap, groups: int, heads: int, q_len: int, kv_len: int, *,
                       q_per_kv: int = 1, do_scale: float = 1.0, need_dq: bool = True, need_dkv: bool = True, o=None, lse=None,
                       dq_out=None, dk_out=None, dv_out=None, accumulate: bool = False):
        """Gradients of ``flash_attn`` (same maps): ``do`` = gradient of the output buffer (rows as q), scaled by ``do_scale`` (= the
        forward's out_scale).  Returns (dq [q rows, C] | None, dk, dv [k rows, C] | None); rows of dk / dv that the K/V map never
        reads (e.g. frames > 0 in the first-frame branch) are zero.  ``o`` / ``lse`` (the un-accumulated output and the log-sum-exp of
        ``flash_attn(with_lse=True)``): the statistics pass is replaced by one elementwise kernel (delta = rowsum(dO * O) per head).
        ``dq_out`` / ``dk_out`` + ``dv_out``: [rows, C] views with their own row stride (the column blocks of the gradient of a fused
        Q|K|V projection output) that the kernel writes instead of fresh tensors; they are returned.  ``accumulate``: the gradients are
        ADDED to those views (every wanted gradient needs one); ``do_scale`` 0 then leaves them bit for bit as they were."""
        q, k, v, do = self._act(q, "attn_bwd.q"), self._act(k, "attn_bwd.k"), self._act(v, "attn_bwd.v"), self._act(do, "attn_bwd.do")
        C = q.shape[1]
        D = C // heads
        assert k.stride(0) == v.stride(0) and do.shape == q.shape
        def grad_buf(out, rows, covered):
            # rows the map never reaches must still come back defined (zero): the query map reaches all of them in the model's calls, the
            # K / V map does not in the first-frame branches
            if out is not None:
                assert out.shape == (rows, C) and out.stride(1) == 1 and out.dtype == self.act_dtype and out.stride(0) % 8 == 0 and out.data_ptr() % 16 == 0
                if not covered and not accumulate:
                    out.zero_()
                return out
            return self.empty(rows, C) if covered else torch.zeros((rows, C), dtype=self.act_dtype, device=self.device)
        assert (dk_out is None) == (dv_out is None)
        if accumulate:
            assert (dq_out is not None or not need_dq) and (dk_out is not None or not need_dkv), "accumulate adds into dq_out / dk_out / dv_out"
        flags = 1 if accumulate else 0
        dq = grad_buf(dq_out, q.shape[0], q.shape[0] == groups * q_len) if need_dq else None
        kv_covered = need_dkv and self._kv_map_covers(kmap, groups, q_per_kv, kv_len, k.shape[0])
        dk = grad_buf(dk_out, k.shape[0], kv_covered) if need_dkv else None
        dv = grad_buf(dv_out, k.shape[0], kv_covered) if need_dkv else None
        assert dk is None or dk.stride(0) == dv.stride(0)
        qm, km, dom = qmap.c(q.stride(0)), kmap.c(k.stride(0)), qmap.c(do.stride(0))
        dqm, dkm = qmap.c(dq.stride(0) if dq is not None else C), kmap.c(dk.stride(0) if dk is not None else C)
        if lse is not None:
            assert o is not None and lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == groups * heads * q_len
            o = self._act(o, "attn_bwd.o")
            lse2, delta = lse, self._f32(groups * heads * q_len)
            om = qmap.c(o.stride(0))
            self._launch("a3d_attn_delta_bf16", _p(do), _p(o), ctypes.byref(dom), ctypes.byref(om), _p(delta), groups, heads, D, q_len,
                         what=f"groups={groups} heads={heads} D={D} q_len={q_len}")
            flags |= 2
        else:
            stats = self._f32(2, groups * heads * q_len)
            lse2, delta = stats[0], stats[1]
        def run(dq_, dk_, dv_, dkm_, share, fl):
            self._launch("a3d_flash_attn_bwd_bf16", _p(q), _p(k), _p(v), _p(do), _p(dq_), _p(dk_), _p(dv_), _p(lse2), _p(delta),
                         ctypes.byref(qm), ctypes.byref(km), ctypes.byref(dom), ctypes.byref(dqm), ctypes.byref(dkm_),
                         groups, heads, D, q_len, kv_len, share, float(D) ** -0.5, do_scale, fl,
                         what=f"groups={groups} heads={heads} D={D} q_len={q_len} kv_len={kv_len} q_per_kv={share}")

        # Shared keys (first-frame branches: the q_per_kv = F query groups of a video read frame 0's K / V): the kernel sums their dK | dV
        # inside one workgroup per key tile, i.e. groups / q_per_kv x key tiles x heads workgroups — 16 .. 256 at the training shapes,
        # a fraction of the chip (2.5 - 3.8 x the time of the same attention with private keys at head_dim 80 / 160).  When that grid
        # cannot fill the CUs, every query group writes its own partial dK | dV (full-width grid, no sharing) and one reduction over
        # the q_per_kv partials follows (torch.sum accumulates in fp32).
        wgs_shared = (groups // q_per_kv) * heads * ((kv_len + 127) // 128)
        if need_dkv and q_per_kv > 1 and wgs_shared < 512:
            if need_dq:
                run(dq, None, None, dkm, q_per_kv, flags)
            pk = self.empty(groups * kv_len, C)
            pv = self.empty(groups * kv_len, C)
            # (the first call left the statistics in lse2 / delta; the fresh partials are written, never added to)
            run(None, pk, pv, RowMap(1, kv_len, 0, kv_len, 0).c(C), 1, (flags & 2) | (2 if need_dq else 0))
            idx = self._shared_kv_rows(kmap, groups, q_per_kv, kv_len)
            put = dk.index_add_ if accumulate else dk.index_copy_
            put(0, idx, pk.view(groups // q_per_kv, q_per_kv, kv_len, C).sum(dim=1).view(-1, C))
            put = dv.index_add_ if accumulate else dv.index_copy_
            put(0, idx, pv.view(groups // q_per_kv, q_per_kv, kv_len, C).sum(dim=1).view(-1, C))
            return dq, dk, dv
        run(dq, dk, dv, dkm, q_per_kv, flags)
        return dq, dk, dv

    def _kv_map_covers(self, kmap: RowMap, groups: int, q_per_kv: int, kv_len: int, rows: int) -> bool:
        """``rowmap_covers`` for this attention's key map, decided once per map and cached — on the CPU: the answer is a function of a few
        integers, and a device-side unique / min / max with read-backs would be a host synchronisation inside the first backward of every
        map (it would also fail under HIP-graph capture of a training step)."""
        key = (kmap.gdiv, kmap.ga, kmap.gb, kmap.seg_len, kmap.seg_stride, groups, q_per_kv, kv_len, rows)
        hit = self._kv_cover_cache.get(key)
        if hit is None:
            hit = self._kv_cover_cache[key] = rowmap_covers(kmap, groups, q_per_kv, kv_len, rows, "cpu")
        return hit

    def _shared_kv_rows(self, kmap: RowMap, groups: int, q_per_kv: int, kv_len: int) -> torch.Tensor:
        """Rows of the K / V tensor that the first query group of every sharing set reads, in (set, key) order (cached per map)."""
        key = (kmap.gdiv, kmap.ga, kmap.gb, kmap.seg_len, kmap.seg_stride, groups, q_per_kv, kv_len)
        cache = self._kv_row_cache
        if key not in cache:
            cache[key] = rowmap_rows(kmap, groups, q_per_kv, kv_len, self.device)
        return cache[key]

    def temporal_attn_bwd(self, q, k, v, do, videos: int, frames: int, L: int, heads: int):
        """Returns one [rows, 3C] buffer = [dq | dk | dv]."""
        q, k, v, do = self._act(q, "tattn_bwd.q"), self._act(k, "tattn_bwd.k"), self._act(v, "tattn_bwd.v"), self._act(do, "tattn_bwd.do")
        C = q.shape[1]
        assert q.stride(0) == k.stride(0) == v.stride(0)
        d = self.empty(q.shape[0], 3 * C)
        self._launch("a3d_temporal_attn_bwd_bf16", _p(q), _p(k), _p(v), q.stride(0), _p(do), do.stride(0),
                     _p(d), d.data_ptr() + 2 * C, d.data_ptr() + 4 * C, 3 * C,
                     videos, frames, L, heads, C // heads, float(C // heads) ** -0.5, what=f"videos={videos} frames={frames} L={L} C={C}")
        return d

    def layer_norm_bwd(self, x, dy, gamma, eps: float, need_param: bool = True):
        x, dy = self._act(x, "ln_bwd.x"), self._act(dy, "ln_bwd.dy")
        assert x.is_contiguous() and dy.is_contiguous() and x.shape == dy.shape
        M, C = x.shape
        dx = self.empty(M, C)
        dg = self._f32(C) if need_param else None
        db = self._f32(C) if need_param else None
        self._launch("a3d_layer_norm_bwd_bf16", _p(x), _p(dy), _p(gamma), _p(dx), _p(dg), _p(db), M, C, eps, 0, what=f"M={M} C={C}")
        return dx, dg, db

    def group_norm_stats(self, x, B: int, rows: int, groups: int, eps: float) -> torch.Tensor:
        """fp32 [B, groups, 2] = (mean, rstd) from the fp64 sums kernel (the finalisation is a [B, groups] host-side expression)."""
        sums = self.group_norm_sums(x, B, rows, groups)
        m = sums / float(rows * (x.shape[1] // groups))                         # fp64 (E[x], E[x^2]); seven small launches in all
        mean = m[..., 0]
        rstd = torch.addcmul(m[..., 1], mean, mean, value=-1.0).clamp_min_(0.0).add_(eps).rsqrt_()
        return torch.stack([mean, rstd], dim=-1).to(torch.float32)

    def group_norm_bwd(self, x, dy, B: int, rows: int, gamma, beta, groups: int, stats, silu: bool, need_param: bool = False):
        x, dy = self._act(x, "gn_bwd.x"), self._act(dy, "gn_bwd.dy")
        assert x.is_contiguous() and dy.is_contiguous() and x.shape == dy.shape and x.shape[0] == B * rows
        C = x.shape[1]
        dx = self.empty(x.shape[0], C)
        ws = self._f32(B * C * 2)
        dg = torch.zeros(C, dtype=torch.float32, device=self.device) if need_param else None
        db = torch.zeros(C, dtype=torch.float32, device=self.device) if need_param else None
        self._launch("a3d_group_norm_bwd_bf16", _p(x), _p(dy), _p(gamma), _p(beta), _p(stats), _p(dx), _p(ws), _p(dg), _p(db),
                     B, rows, C, groups, 1 if silu else 0, what=f"B={B} rows={rows} C={C}")
        return dx, dg, db

    def geglu_bwd(self, proj_il, dy):
        proj_il, dy = self._act(proj_il, "geglu_bwd.p"), self._act(dy, "geglu_bwd.dy")
        M, N2 = proj_il.shape
        dp = self.empty(M, N2)
        self._launch("a3d_geglu_bwd_bf16", _p(proj_il), proj_il.stride(0), _p(dy), dy.stride(0), _p(dp), N2, M, N2 // 2, what=f"M={M} N={N2 // 2}")
        return dp

    def transpose(self, x, pad: int = 64):
        """[rows, cols] -> [cols, rows rounded up to ``pad``] (zero filled): an operand of the weight-gradient GEMM."""
        x = self._act(x, "transpose.x")
        rows, cols = x.shape
        rp = (rows + pad - 1) // pad * pad
        y = self.empty(cols, rp)
        self._launch("a3d_transpose_bf16", _p(x), x.stride(0), _p(y), rp, rows, cols, rp, what=f"{rows}x{cols}")
        return y

    def wgrad(self, dy, x, alpha: float = 1.0):
        """fp32 [N, K] = alpha * dy^T x: the weight gradient of y = x W^T (split over the token axis, fp32 atomics)."""
        dy, x = self._act(dy, "wgrad.dy"), self._act(x, "wgrad.x")
        assert dy.shape[0] == x.shape[0]
        M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
        dw = self._f32(N, K)
        ws = self._f32(int(self.lib.a3d_wgrad_ws_floats(M, N, K)))
        self._launch("a3d_wgrad_bf16", _p(dy), dy.stride(0), _p(x), x.stride(0), _p(dw), K, _p(ws), M, N, K, alpha, 0, what=f"M={M} N={N} K={K}")
        return dw

    def colsum(self, x, alpha: float = 1.0):
        x = self._act(x, "colsum.x")
        out = self._f32(x.shape[1])
        self._launch("a3d_colsum_bf16", _p(x), x.stride(0), x.shape[0], x.shape[1], _p(out), alpha, 0)
        return out

    def axpby_(self, x, y, a: float = 1.0, b: float = 1.0):
        """y <- a x + b y (in place on ``y``)."""
        x, y = self._act(x, "axpby.x"), self._act(y, "axpby.y")
        assert x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
        self._launch("a3d_axpby_bf16", _p(x), _p(y), x.numel(), a, b)
        return y

    def scaled(self, x, a: float):
        return self.axpby_(x, torch.empty_like(x), a, 0.0)

    def zero_insert2x(self, dy, B: int, H: int, W: int):
        dy = self._act(dy, "zero_insert.dy")
        assert dy.is_contiguous() and dy.shape[0] == B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        z = self.empty(B * H * W, dy.shape[1])
        self._launch("a3d_zero_insert2x_bf16", _p(dy), _p(z), B, H, W, dy.shape[1])
        return z

    def upsample2x_bwd(self, du, B: int, H: int, W: int, He: int, We: int):
        du = self._act(du, "upsample_bwd.du")
        assert du.is_contiguous() and du.shape[0] == B * He * We
        dx = self.empty(B * H * W, du.shape[1])
        self._launch("a3d_upsample2x_bwd_bf16", _p(du), _p(dx), B, H, W, He, We, du.shape[1])
        return dx

    def sqnorm(self, g: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False):
        assert g.dtype == torch.float32 and g.is_contiguous()
        out = out if out is not None else self._f32(1)
        self._launch("a3d_sqnorm_f32", _p(g), g.numel(), _p(out), 1 if accumulate else 0)
        return out

    def clip_ctrl(self, sq: torch.Tensor, max_norm: float, inv_loss_scale: float = 1.0):
        ctrl = self._f32(3)
        self._launch("a3d_clip_ctrl_f32", _p(sq), max_norm, inv_loss_scale, _p(ctrl))
        return ctrl

    def adamw_(self, p, g, m, v, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, step: int = 1, ctrl=None):
        for t in (p, g, m, v):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
        b1, b2 = betas
        self._launch("a3d_adamw_f32", _p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, weight_decay, 1.0 - b1 ** step, 1.0 - b2 ** step, _p(ctrl))
        return p

    def cfg_ddim_step(self, eps_pair, x, first_frame, guidance: float, alpha_t: float, alpha_prev: float):
        """Fused pipeline epilogue (pipeline.py:1023-1031); fp32 [n, C, F, H, W] tensors."""
        for t in (eps_pair, x, first_frame):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        n, C, F, H, W = x.shape
        assert eps_pair.shape == (2 * n, C, F, H, W) and first_frame.numel() == n * C * H * W
        y = torch.empty_like(x)
        self._launch("a3d_cfg_ddim_step_f32", _p(eps_pair), _p(x), _p(first_frame), _p(y), n, C, F, H * W, guidance, alpha_t, alpha_prev)
        return y
