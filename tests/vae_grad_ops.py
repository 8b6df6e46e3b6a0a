"""Plain-PyTorch statements of the VAE-encoder backward entry points (TEST INFRASTRUCTURE, as tests/torch_ops.py is for the rest of the
op set): ``im2col_in_bwd`` (the adjoint of a3d_im2col_in) and ``softmax_rows_bwd``, in fp32.  The product never imports this file."""
import torch
import torch.nn.functional as F

from tests.torch_ops import TorchRefOps


class VaeGradRefOps(TorchRefOps):
    def im2col_in_bwd(self, dcol, V, C, Fr, H, W, scale=1.0):
        cols = dcol.float()[:, : 9 * C].reshape(V * Fr, H * W, 9, C).permute(0, 3, 2, 1).reshape(V * Fr, C * 9, H * W)   # unfold's c*9 + tap
        img = F.fold(cols, output_size=(H, W), kernel_size=3, padding=1)                                                   # [(V F), C, H, W]
        return (scale * img).reshape(V, Fr, C, H, W).permute(0, 2, 1, 3, 4).contiguous()

    def softmax_rows_bwd(self, p, dp, alpha=1.0, out=None):
        pf = p.float()
        y = self._o(alpha * pf * (dp.float() - (pf * dp.float()).sum(dim=-1, keepdim=True)))
        if out is not None:
            out.copy_(y)
            return out
        return y
