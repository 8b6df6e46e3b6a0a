"""CPU checks of the reconstruction loss's entry points (include/animate3d_hip.h, csrc/recon_loss.hip): a NULL or misaligned pointer, a
non-positive or oversized extent and a wrong partial count are refused with A3D_EINVAL before anything reaches the GPU.  As in
tests/test_cabi_contract.py the device addresses are made up and never dereferenced, every call differs from a valid launch in exactly
one operand, and no call may pass with everything valid: that would launch a kernel on made-up addresses."""
import pytest

A3D_EINVAL = -1
BASE = 0x7F00_0010_0000
B, H, W = 3, 33, 65                                    # 2145 pixels per image: two blocks each
N_PARTIALS = B * 2
FWD = ("image", "alpha", "gt_rgb", "gt_mask", "index", "partials", "out")
BWD = ("image", "alpha", "gt_rgb", "gt_mask", "index", "grad_out", "d_image", "d_alpha")
OPTIONAL = {"index": "any", "d_image": "one", "d_alpha": "one"}


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _call(lib, entry, ptr=None, **geometry):
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    names = FWD if entry == "a3d_recon_loss_f32" else BWD
    p = {n: BASE + 0x10_0000 * i for i, n in enumerate(names)}
    p.update(ptr or {})
    g = dict(dict(B=B, H=H, W=W, n_partials=N_PARTIALS), **geometry)
    head = [None, g["B"], g["H"], g["W"], p["image"], p["alpha"], p["gt_rgb"], p["gt_mask"], p["index"], 0.5]
    if entry == "a3d_recon_loss_f32":
        return lib.a3d_recon_loss_f32(*head, 100.0, 100.0, p["partials"], g["n_partials"], p["out"])
    return lib.a3d_recon_loss_bwd_f32(*head, 1e-3, 1e-3, p["grad_out"], p["d_image"], p["d_alpha"])


ENTRY = pytest.mark.parametrize("entry", ["a3d_recon_loss_f32", "a3d_recon_loss_bwd_f32"])


@ENTRY
def test_recon_loss_refuses_misaligned_or_missing_operand(lib, entry):
    names = FWD if entry == "a3d_recon_loss_f32" else BWD
    for operand in names:
        if operand != "gt_mask":                                                        # bytes: any address is aligned
            for off in (1, 2):
                rc = _call(lib, entry, ptr={operand: BASE + off})
                assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"
        if operand not in OPTIONAL:
            assert _call(lib, entry, ptr={operand: None}) == A3D_EINVAL, f"{entry}: NULL {operand}"
    if entry == "a3d_recon_loss_bwd_f32":
        assert _call(lib, entry, ptr={"d_image": None, "d_alpha": None}) == A3D_EINVAL                # nothing to write


@ENTRY
def test_recon_loss_refuses_bad_sizes(lib, entry):
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1),
           dict(B=1, H=2 ** 20, W=2 ** 20), dict(B=4, H=2 ** 19, W=2 ** 19), dict(B=2 ** 20, H=2 ** 10, W=2 ** 10),       # B H W = 2^40
           dict(B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1), dict(B=2 ** 31 - 1, H=1, W=2049)]
    for g in bad:
        assert _call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"
    if entry == "a3d_recon_loss_f32":
        for n in (0, -1, N_PARTIALS - 1, N_PARTIALS + 1, B):
            assert _call(lib, entry, n_partials=n) == A3D_EINVAL, f"n_partials = {n}"
