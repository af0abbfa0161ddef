"""Argument helpers the host modules share: ctypes views of arrays and tensors, and the checks more than one entry point makes."""
import ctypes as C

import numpy as np
import torch

from ._lib import Y3Error


def _fptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dev(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_cuda(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise Y3Error("expected contiguous CUDA(HIP) tensors; the y3 kernels have no CPU fallback")


def _anchors(anchors_table, reshape=False, scales=3):
    """-> float32 [scales,3,2], contiguous (scales: the grids / the net's heads, three or two).  reshape: any scales * 6 values are taken
    (the Net methods); otherwise the shape is checked."""
    a = np.ascontiguousarray(anchors_table.detach().cpu().numpy() if isinstance(anchors_table, torch.Tensor)
                             else anchors_table, np.float32)
    if reshape:
        if a.size != scales * 6:
            raise Y3Error(f"anchors_table must hold {scales} x 3 (w, h) pairs (got {a.size} values)")
        a = np.ascontiguousarray(a.reshape(scales, 3, 2))
    if a.shape != (scales, 3, 2):
        raise Y3Error(f"anchors_table must be [{scales},3,2]")
    return a


def _images_arg(images):
    """The image batch of Net.forward_decode / Net.detect: fp32 [B,H,W,3] on the GPU."""
    _need_cuda(images)
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[3] != 3:
        raise Y3Error("images must be float32 [B,H,W,3]")
