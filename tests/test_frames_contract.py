"""CPU checks of the frame entry points (include/animate3d_hip.h, csrc/stage_frames.hip, the rgba8 pair of csrc/recon_loss.hip): a NULL or
misaligned pointer, a bad extent or factor and a wrong partial count are refused with A3D_EINVAL before anything reaches the GPU.  As in
tests/test_stage4d_contract.py the device addresses are made up and never dereferenced, every call differs from a valid launch in exactly
one operand, and no call may pass with everything valid: that would launch a kernel on made-up addresses."""
import pytest

A3D_EINVAL = -1
BASE = 0x7F00_0010_0000
B, H, W = 3, 33, 65                                    # 2145 pixels per image: two blocks each
N_PARTIALS = B * 2
FWD = ("image", "alpha", "gt_rgba8", "index", "partials", "out")
BWD = ("image", "alpha", "gt_rgba8", "index", "grad_out", "d_image", "d_alpha")
OPTIONAL = {"index", "d_image", "d_alpha"}
LOSS = pytest.mark.parametrize("entry", ["a3d_recon_loss_rgba8_f32", "a3d_recon_loss_rgba8_bwd_f32"])


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _addresses(names, ptr):
    p = {n: BASE + 0x10_0000 * i for i, n in enumerate(names)}
    p.update(ptr or {})
    return p


def _loss(lib, entry, ptr=None, **geometry):
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _addresses(FWD if entry == "a3d_recon_loss_rgba8_f32" else BWD, ptr)
    g = dict(dict(B=B, H=H, W=W, n_partials=N_PARTIALS), **geometry)
    head = [None, g["B"], g["H"], g["W"], p["image"], p["alpha"], p["gt_rgba8"], p["index"], 0.5]
    if entry == "a3d_recon_loss_rgba8_f32":
        return lib.a3d_recon_loss_rgba8_f32(*head, 100.0, 100.0, p["partials"], g["n_partials"], p["out"])
    return lib.a3d_recon_loss_rgba8_bwd_f32(*head, 1e-3, 1e-3, p["grad_out"], p["d_image"], p["d_alpha"])


@LOSS
def test_rgba8_loss_refuses_misaligned_or_missing_operand(lib, entry):
    names = FWD if entry == "a3d_recon_loss_rgba8_f32" else BWD
    for operand in names:
        for off in (1, 2, 3):                                                               # gt_rgba8 too: a pixel is one 4-byte load
            rc = _loss(lib, entry, ptr={operand: BASE + off})
            assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"
        if operand not in OPTIONAL:
            assert _loss(lib, entry, ptr={operand: None}) == A3D_EINVAL, f"{entry}: NULL {operand}"
    if entry == "a3d_recon_loss_rgba8_bwd_f32":
        assert _loss(lib, entry, ptr={"d_image": None, "d_alpha": None}) == A3D_EINVAL       # nothing to write


@LOSS
def test_rgba8_loss_refuses_bad_sizes(lib, entry):
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1),
           dict(B=1, H=2 ** 20, W=2 ** 20), dict(B=4, H=2 ** 19, W=2 ** 19), dict(B=2 ** 20, H=2 ** 10, W=2 ** 10),       # B H W = 2^40
           dict(B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1), dict(B=2 ** 31 - 1, H=1, W=2049)]
    for g in bad:
        assert _loss(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"
    if entry == "a3d_recon_loss_rgba8_f32":
        for n in (0, -1, N_PARTIALS - 1, N_PARTIALS + 1, B):
            assert _loss(lib, entry, n_partials=n) == A3D_EINVAL, f"n_partials = {n}"


UNPACK = ("rgba8", "out8", "rgb", "mask")


def _unpack(lib, ptr=None, **geometry):
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _addresses(UNPACK, ptr)
    g = dict(dict(S=2, h=12, w=8, k=2), **geometry)
    return lib.a3d_frames_unpack_u8(None, g["S"], g["h"], g["w"], g["k"], p["rgba8"], p["out8"], p["rgb"], p["mask"])


def test_unpack_refusals(lib):
    assert _unpack(lib, ptr={"rgba8": None}) == A3D_EINVAL
    assert _unpack(lib, ptr={"out8": None, "rgb": None, "mask": None}) == A3D_EINVAL          # nothing to write
    for operand in ("rgba8", "out8", "rgb"):                                                   # mask is bytes: any address is aligned
        for off in (1, 2, 3):
            assert _unpack(lib, ptr={operand: BASE + off}) == A3D_EINVAL, f"{operand} at +{off} bytes"
    bad = [dict(k=0), dict(k=-1), dict(k=17), dict(k=5), dict(h=13), dict(w=7), dict(h=8, w=12, k=3), dict(S=0), dict(S=-1), dict(h=0), dict(w=0),
           dict(h=-12), dict(w=-8), dict(k=3, h=0, w=0), dict(S=2 ** 19, h=2 ** 10, w=2 ** 10), dict(S=2 ** 31 - 1, h=2 ** 30, w=2 ** 30)]
    for g in bad:
        assert _unpack(lib, **g) == A3D_EINVAL, g


def _pack(lib, ptr=None, **geometry):
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _addresses(("image", "alpha", "rgba8"), ptr)
    g = dict(dict(B=2, H=6, W=8), **geometry)
    return lib.a3d_frames_pack_u8(None, g["B"], g["H"], g["W"], p["image"], p["alpha"], p["rgba8"])


def test_pack_refusals(lib):
    for operand in ("image", "alpha", "rgba8"):
        assert _pack(lib, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand}"
        for off in (1, 2, 3):
            assert _pack(lib, ptr={operand: BASE + off}) == A3D_EINVAL, f"{operand} at +{off} bytes"
    for g in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-6), dict(W=-8), dict(B=2 ** 19, H=2 ** 10, W=2 ** 10),
              dict(B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)):
        assert _pack(lib, **g) == A3D_EINVAL, g
