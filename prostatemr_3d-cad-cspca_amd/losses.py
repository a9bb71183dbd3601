"""Loss functions with the class surface of the reference's losses.py (tf2.5/scripts/model/losses.py):
``Focal`` (L:20-49) and ``EvidenceLowerBound`` (L:52-63).  ``Focal.loss`` is one fused HIP pass over the softmax heads
(hip.ops.focal_loss: m1_focal_fwd / m1_focal_bwd); like every op of the package it raises on host tensors (the
plain expression it is tested against lives in the oracle, oracle/m1_oracle.py focal_loss).
``SoftDicePlusBoundarySurface`` (L:66-130, ``--LOSS_MODE region_boundary``) is HIP end to end as well: the signed distance map
of the label that the reference computes with scipy inside ``tf.py_function`` is an exact Euclidean distance transform on the GPU
(hip.ops.dist_map: m1_dist_map, three separable passes), and the Dice and boundary terms of every head are one fused pass
(hip.ops.dice_boundary_loss: m1_dice_bd_fwd / m1_dice_bd_bwd), so the loss captures into the train-step graph.
One deviation: a class that fills a whole sample (no background voxel) gets a distance map of 0 there, the same as an empty
class; scipy's transform is degenerate for it (it measures to a voxel outside the array).
"""
from __future__ import annotations

import torch

K_EPSILON = 1e-7   # tf.keras.backend.epsilon()


class Focal:
    """[1] T.Y. Lin et al. (2017), "Focal Loss for Dense Object Detection".
    Requires 'y_pred': softmax prediction, 'y_true': one-hot label."""

    def __init__(self, alpha=[0.25, 0.75], gamma=2.00):
        self.alpha = alpha
        self.gamma = gamma

    @staticmethod
    def _gpu(y_pred):
        if not y_pred.is_cuda:
            raise RuntimeError("Focal loss runs on the HIP extension only: move the tensors to a GPU device "
                               "(no CPU fallback exists in this package)")

    def FL(self, y_true, y_pred):
        """L:32-41 for ONE head: renormalise -> clip [eps, 1-eps] -> -y*log p -> * y(1-p)^gamma -> * alpha -> sum_{DHWC} -> mean_b
        (the fused kernel m1_focal_fwd / m1_focal_bwd; head.hip)."""
        self._gpu(y_pred)
        from .hip import ops
        return ops.focal_loss(y_true, y_pred[..., :int(y_true.shape[-1])].contiguous(), self.alpha, self.gamma)

    def loss(self, y_true, y_pred):
        """L:43-49: mean over the y_pred.shape[-1]//y_true.shape[-1] prediction heads (deep supervision), one fused launch."""
        self._gpu(y_pred)
        from .hip import ops
        return ops.focal_loss(y_true, y_pred, self.alpha, self.gamma)


class EvidenceLowerBound:
    """Dummy wrapper: the KL is computed inside the model and passed via y_pred (L:52-63)."""

    def __init__(self, beta=1.00):
        self.beta = beta

    def loss(self, y_true, y_pred):
        return self.beta * y_pred.sum()


class SoftDicePlusBoundarySurface:
    """Soft Dice loss + Boundary/Surface loss for multi-class segmentation (L:66-130).
    [1] H. Kervadec et al. (2021), "Boundary Loss for Highly Unbalanced Segmentation", MedIA.
    Requires 'y_pred': softmax prediction, 'y_true': one-hot label.  As in the reference, the Dice term is ONE ratio over the
    whole batch and every foreground class (K.flatten) and the boundary term is a SUM over the batch (not a mean).
    Distance map: distance to the lesion outside it, 1 - (distance to the background) inside it, 0 for an empty class and
    (the one deviation from scipy) 0 for a class that fills the sample."""

    def __init__(self, loss_weights=[1.00, 1.50], smooth=K_EPSILON):
        self.smooth = smooth
        self.loss_weights = loss_weights

    @staticmethod
    def _gpu(t):
        if not t.is_cuda:
            raise RuntimeError("SoftDicePlusBoundarySurface runs on the HIP extension only: move the tensors to a GPU device "
                               "(no CPU fallback exists in this package)")

    def calc_dist_map(self, seg):
        """L:83-92 for ONE sample seg (D,H,W,C): the signed distance map of every channel of seg, (D,H,W,C) fp32."""
        return self.calc_dist_map_batch(seg[None])[0]

    def calc_dist_map_batch(self, y_true):
        """L:94-96: calc_dist_map of every sample of y_true (N,D,H,W,C), (N,D,H,W,C) fp32 (m1_dist_map; the kernel skips channel 0,
        so a zero channel is put in front)."""
        self._gpu(y_true)
        from .hip import ops
        z = torch.zeros(y_true.shape[:-1] + (1,), dtype=y_true.dtype, device=y_true.device)
        return ops.dist_map(torch.cat([z, y_true], dim=-1))

    def _one_head(self, y_true, y_pred, weights):
        self._gpu(y_pred)
        from .hip import ops
        return ops.dice_boundary_loss(y_true, y_pred[..., :int(y_true.shape[-1])].contiguous(), weights, self.smooth)

    def dice_loss(self, y_true, y_pred):
        """L:99-107 for ONE head: renormalise -> clip [eps, 1-eps] -> 1 - 2 sum(y q) / (sum(y + q) + smooth) over classes >= 1."""
        return self._one_head(y_true, y_pred, (1.0, 0.0))

    def boundary_surface_loss(self, y_true, y_pred):
        """L:110-114 for ONE head: renormalise -> clip -> sum(q * dist_map(y_true)) over classes >= 1."""
        return self._one_head(y_true, y_pred, (0.0, 1.0))

    def DB(self, y_true, y_pred):
        """L:117-119: w0 * dice_loss + w1 * boundary_surface_loss for ONE head, one fused pass."""
        return self._one_head(y_true, y_pred, self.loss_weights)

    def loss(self, y_true, y_pred):
        """L:123-130: mean of DB over the y_pred.shape[-1]//y_true.shape[-1] prediction heads (deep supervision), one fused call."""
        self._gpu(y_pred)
        from .hip import ops
        return ops.dice_boundary_loss(y_true, y_pred, self.loss_weights, self.smooth)
