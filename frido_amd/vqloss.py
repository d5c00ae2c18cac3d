"""The MS-VQGAN's codebook loss on the HIP engine: frido_vq_commit_loss (frido_amd/csrc/vqloss.hip), the `emb_loss` of
MSFPNVQModel.encode (taming/models/msvqgan.py:116-154; taming/modules/vqvae/quantize.py:286-291).  Op kind
FRIDO_OP_VQ_COMMIT_LOSS inside a program; launch_vq_commit_loss is the one-launch form."""
import ctypes as C

import torch

from . import _lib


def launch_vq_commit_loss(desc, stream):
    _lib.check(_lib.lib().frido_vq_commit_loss(C.byref(desc), stream), "frido_vq_commit_loss")


def commit_loss_desc(scales, *, partials, out, emb_loss, beta, legacy):
    """scales: per scale, coarse first, (z_ptr, zq_ptr, npix, C, c0, e); partials / out / emb_loss: device pointers (a
    _lib.VQLOSS_WS_BYTES buffer, [n] floats, one float)."""
    d = _lib.STRUCTS["FridoVqCommitLoss"](partials=partials, out=out, emb_loss=emb_loss, beta=float(beta), n_scales=len(scales),
                                          legacy=int(bool(legacy)))
    for k, (z, zq, npix, Cn, c0, e) in enumerate(scales[:_lib.VQLOSS_MAX_SCALES]):
        d.z[k], d.zq[k], d.npix[k], d.C[k], d.c0[k], d.e[k] = z, zq, npix, Cn, c0, e
    return d


class CommitLoss:
    """Device state of one encode plan's loss: the workspace, the per-scale means and the total, and the descriptor over the plan's
    pre-quant / quantised maps."""

    def __init__(self, plan, embed, beta, legacy, device):
        n = len(embed)
        if n > _lib.VQLOSS_MAX_SCALES:
            raise NotImplementedError(f"{n} scales: frido_vq_commit_loss takes at most {_lib.VQLOSS_MAX_SCALES}")
        self.partials = torch.zeros(_lib.VQLOSS_WS_BYTES // 8, dtype=torch.float64, device=device)
        self.means = torch.zeros(n, dtype=torch.float32, device=device)
        self.total = torch.zeros((), dtype=torch.float32, device=device)
        scales = [(hq.data_ptr(), zq.data_ptr(), hq.shape[0], embed[i], 0, embed[i])
                  for i, ((hq, _, _), (zq, _, _)) in enumerate(zip(plan.h_out, plan.zq))]
        self.desc = commit_loss_desc(scales, partials=self.partials.data_ptr(), out=self.means.data_ptr(), emb_loss=self.total.data_ptr(),
                                     beta=beta, legacy=legacy)
        self.keep = plan
