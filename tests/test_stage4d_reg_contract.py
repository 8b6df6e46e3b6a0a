"""CPU checks of the regularisers' entry points (include/animate3d_hip.h, csrc/stage_reg.hip): a NULL or misaligned pointer, a non-positive
or oversized extent, a TV term on an image with one row or column and a wrong partial count are refused with A3D_EINVAL before anything
reaches the GPU.  As in tests/test_stage4d_contract.py the device addresses are made up and never dereferenced, every call differs from
a valid launch in exactly one respect, and no call may pass with everything valid: that would launch a kernel on made-up addresses."""
import pytest

A3D_EINVAL = -1
BASE = 0x7F00_0010_0000
B, H, W = 3, 33, 300                                   # 9900 pixels per image: two blocks each
N = 700                                                # 2100 (image, Gaussian) pairs: three blocks

# entry -> its pointer operands in call order
ENTRIES = {
    "a3d_image_reg_f32": ("image", "depth", "alpha", "partials", "out"),
    "a3d_image_reg_bwd_f32": ("image", "depth", "alpha", "grad_out", "d_image", "d_depth", "d_alpha"),
    "a3d_gaussian_reg_f32": ("means", "scales", "scaling", "opacity", "partials", "out"),
    "a3d_gaussian_reg_bwd_f32": ("means", "scaling", "grad_out", "d_means", "d_scales", "d_opacity"),
}
ENTRY = pytest.mark.parametrize("entry", list(ENTRIES))


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _call(lib, entry, ptr=None, **other):
    assert ptr or other, "a fully valid call would launch a kernel on made-up addresses"
    names = ENTRIES[entry]
    p = {n: BASE + 0x10_0000 * i for i, n in enumerate(names)}
    p.update(ptr or {})
    g = dict(dict(B=B, H=H, W=W, N=N, n_partials=B * 2 if "image" in entry else 3, scales_bs=3 * N, lambdas=(1.0, 1.0, 1.0)), **other)
    if entry == "a3d_image_reg_f32":
        return lib.a3d_image_reg_f32(None, g["B"], g["H"], g["W"], p["image"], p["depth"], p["alpha"], *g["lambdas"], p["partials"],
                                     g["n_partials"], p["out"])
    if entry == "a3d_image_reg_bwd_f32":
        return lib.a3d_image_reg_bwd_f32(None, g["B"], g["H"], g["W"], p["image"], p["depth"], p["alpha"], 1e-3, 1e-3, 1e-3, 1e-3, 1e-3,
                                         p["grad_out"], p["d_image"], p["d_depth"], p["d_alpha"])
    if entry == "a3d_gaussian_reg_f32":
        return lib.a3d_gaussian_reg_f32(None, g["B"], g["N"], p["means"], p["scales"], g["scales_bs"], p["scaling"], p["opacity"],
                                        *g["lambdas"], p["partials"], g["n_partials"], p["out"])
    return lib.a3d_gaussian_reg_bwd_f32(None, g["B"], g["N"], p["means"], p["scaling"], 1e-3, 1e-3, 1e-3, p["grad_out"], p["d_means"],
                                        p["d_scales"], p["d_opacity"])


@ENTRY
def test_refuses_a_misaligned_operand(lib, entry):
    for operand in ENTRIES[entry]:
        for off in (1, 2):
            rc = _call(lib, entry, ptr={operand: BASE + off})
            assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"


def test_forward_refuses_a_missing_operand_of_a_term_that_is_on(lib):
    """With all three weights non-zero every input is needed; the workspace and the output always are."""
    for entry in ("a3d_image_reg_f32", "a3d_gaussian_reg_f32"):
        for operand in ENTRIES[entry]:
            assert _call(lib, entry, ptr={operand: None}) == A3D_EINVAL, f"{entry}: NULL {operand}"
        assert _call(lib, entry, lambdas=(0.0, 0.0, 0.0)) == A3D_EINVAL, f"{entry}: nothing to compute"


def test_backward_refuses_an_output_without_its_input_and_no_output_at_all(lib):
    assert _call(lib, "a3d_image_reg_bwd_f32", ptr={"grad_out": None}) == A3D_EINVAL
    assert _call(lib, "a3d_gaussian_reg_bwd_f32", ptr={"grad_out": None}) == A3D_EINVAL
    for operand in ("image", "depth", "alpha"):                                        # d_image / d_depth / d_alpha are asked for
        assert _call(lib, "a3d_image_reg_bwd_f32", ptr={operand: None}) == A3D_EINVAL, operand
    for operand in ("means", "scaling"):                                               # d_means / d_opacity are asked for
        assert _call(lib, "a3d_gaussian_reg_bwd_f32", ptr={operand: None}) == A3D_EINVAL, operand
    assert _call(lib, "a3d_image_reg_bwd_f32", ptr={"d_image": None, "d_depth": None, "d_alpha": None}) == A3D_EINVAL
    assert _call(lib, "a3d_gaussian_reg_bwd_f32", ptr={"d_means": None, "d_scales": None, "d_opacity": None}) == A3D_EINVAL


@pytest.mark.parametrize("entry", ["a3d_image_reg_f32", "a3d_image_reg_bwd_f32"])
def test_image_entries_refuse_bad_sizes(lib, entry):
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1),
           dict(H=1), dict(W=1), dict(H=1, W=1),                                        # a TV term divides by H - 1 and W - 1
           dict(B=1, H=2 ** 15, W=2 ** 15 + 4), dict(B=1, H=2 ** 20, W=2 ** 20), dict(B=1, H=2 ** 31 - 1, W=2 ** 31 - 1),     # H W > 2^30
           dict(B=2 ** 31 - 1, H=2, W=8192 + 1), dict(B=2 ** 20, H=2 ** 10, W=2 ** 14)]                                       # the grid
    for g in bad:
        if entry == "a3d_image_reg_f32":                         # a partial count that fits the sizes, where one exists: only the sizes are wrong
            b, h, w = g.get("B", B), g.get("H", H), g.get("W", W)
            g = dict(g, n_partials=max(b, 0) * ((max(h, 0) * max(w, 0) + 8191) // 8192))
        assert _call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"
    if entry == "a3d_image_reg_f32":
        for n in (0, -1, B * 2 - 1, B * 2 + 1, B):
            assert _call(lib, entry, n_partials=n) == A3D_EINVAL, f"n_partials = {n}"


@pytest.mark.parametrize("entry", ["a3d_gaussian_reg_f32", "a3d_gaussian_reg_bwd_f32"])
def test_gaussian_entries_refuse_bad_sizes(lib, entry):
    bad = [dict(B=0), dict(B=-1), dict(N=0), dict(N=-5), dict(B=2 ** 11, N=2 ** 20), dict(B=2 ** 31 - 1, N=2 ** 31 - 1), dict(B=1, N=2 ** 30 + 1)]
    for g in bad:
        if entry == "a3d_gaussian_reg_f32":
            b, n = g.get("B", B), g.get("N", N)
            g = dict(g, n_partials=(max(b, 0) * max(n, 0) + 1023) // 1024, scales_bs=3 * n)
        assert _call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"
    if entry == "a3d_gaussian_reg_f32":
        for n in (0, -1, 2, 4, 2100):
            assert _call(lib, entry, n_partials=n) == A3D_EINVAL, f"n_partials = {n}"
        for bs in (1, 3, N, 3 * N + 3, -3 * N):                                         # neither per image nor shared
            assert _call(lib, entry, scales_bs=bs) == A3D_EINVAL, f"scales_bs = {bs}"
