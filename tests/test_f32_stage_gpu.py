"""The launch helper of animate3d_amd/f32_stage.py on a second device: tensors on cuda:1 while cuda:0 is current must be launched on
cuda:1, with results bit-identical to the same calls on cuda:0.  Needs two visible GPUs; everything else of the shared layer is covered by
tests/test_f32_stage_host.py and, through the three modules, by tests/test_{splat,deform4d,arap}_gpu.py."""
import math

import pytest
import torch

from animate3d_amd import arap, deform4d, splat
from tests import gs_ref

pytestmark = pytest.mark.gpu


def _stage(dev):
    """knn_graph (N = 256, K = 3), deform_gaussians (T = 2) and rasterize_gaussians (B = 2, 32 x 32) with every input on ``dev``, built on
    the CPU from fixed seeds; the outputs and the gradients of scaling and rotation, on the CPU."""
    N, B, H, W = 256, 2, 32, 32
    g = torch.Generator().manual_seed(3)
    xyz = (torch.randn(N, 3, generator=g) * 0.5).to(dev)
    scaling = (torch.rand(N, 3, generator=g) * 2 - 4).to(dev).requires_grad_(True)
    rotation = torch.randn(N, 4, generator=g).to(dev).requires_grad_(True)
    opac = torch.sigmoid(torch.randn(N, 1, generator=g)).to(dev)
    colors = torch.rand(N, 3, generator=g).to(dev)
    torch.manual_seed(0)
    field = deform4d.HexPlaneDeformation(grid_size=((6, 5, 7, 3), (12, 10, 14, 6)), use_global_trans=True)
    with torch.no_grad():
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.normal_(0.0, 0.05, generator=g)
    field = field.to(dev)
    c2w = torch.stack([gs_ref.look_at((3.5, 0.0, 0.5)), gs_ref.look_at((0.0, 3.5, 0.5))])
    fov = torch.full((B,), math.radians(40.0))
    w2c, full, center = splat.get_cam_info_gaussian(c2w, fov, fov, 0.1, 100.0)
    tan = torch.tan(fov / 2).to(dev)
    nn_idx, nn_dist = arap.knn_graph(xyz, 3)
    means, scales, rots = field(xyz, scaling, rotation, torch.tensor([-0.3, 0.7]).to(dev))
    img, radii, dep, alp = splat.rasterize_gaussians(means, scales, rots, opac, colors_precomp=colors, viewmatrix=w2c.to(dev),
                                                     projmatrix=full.to(dev), campos=center.to(dev), tanfovx=tan, tanfovy=tan,
                                                     image_height=H, image_width=W, bg=torch.ones(3, device=dev))
    grads = torch.autograd.grad(img.sum() + 0.1 * dep.sum() + alp.sum(), [scaling, rotation])
    outs = dict(nn_idx=nn_idx, nn_dist=nn_dist, means=means, scales=scales, rotations=rots, image=img, radii=radii, depth=dep, alpha=alp,
                d_scaling=grads[0], d_rotation=grads[1])
    assert all(t.device == torch.device(dev) for t in outs.values())
    return {k: t.detach().cpu() for k, t in outs.items()}


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="the device guard needs two visible GPUs: cuda:0 current, every input on cuda:1")
def test_inputs_on_a_device_that_is_not_current_launch_on_their_own_device():
    torch.cuda.set_device(0)
    want = _stage("cuda:0")
    got = _stage("cuda:1")
    assert torch.cuda.current_device() == 0
    assert float(want["alpha"].max()) > 0.0 and int((want["radii"] > 0).sum()) > 0 and float(want["d_scaling"].abs().max()) > 0.0
    for k in want:
        assert torch.equal(got[k], want[k]), k
