"""FALoss and SupConLoss: drop-ins for the reference's ``models/losses.py`` (same constructors, defaults and forward
signatures), on the fused gfx950 kernels of csrc/losses.hip.

    from transmf_ad_amd.losses import FALoss, SupConLoss

fp32 tensors on a HIP device take the kernels (``fa_kernel_ok`` / ``supcon_kernel_ok`` tell); every other call — another
dtype, a CPU tensor, ``reduction='none'``, a channel count or a SupCon problem the kernels do not cover — runs the same
formula in plain torch ops on the caller's device (``fa_loss_torch`` / ``supcon_loss_torch``), the library's rule for a
``--dim`` it does not cover.

FALoss:  with F1, F2 the maps flattened to (B, C, N),  D_b = F1_b^T F1_b - F2_b^T F2_b  (N x N);  'mean' is
sum |D| / (B N^2), 'sum' is sum |D|, 'none' the (B, N^2) tensor |D|.  The kernel never writes D: see DESIGN.md 3.21.

SupConLoss:  anchors a_i, contrast rows c_j (all views of all samples, view-major);  l_ij = a_i . c_j / T;  the self
column is left out of the log-sum-exp and of the positives m_ij;
loss_i = -(T / T_base) sum_j m_ij (l_ij - log sum_{k != i} exp l_ik) / sum_j m_ij;  the result is the mean over anchors.
An anchor without a positive gives 0 / 0 = NaN, as in the reference.

CrossEntropyLoss and AdversarialCriterion (csrc/criterion.hip): the step's criterion.

    from transmf_ad_amd.losses import CrossEntropyLoss, AdversarialCriterion

CrossEntropyLoss has torch.nn.CrossEntropyLoss's constructor; AdversarialCriterion()(output_logits, D_MRI_logits,
D_PET_logits, label) returns (ce_loss, ad_loss) of kfold_train_adversarial.py:119-125 from one launch.  fp32 (B, C) logits
and int64 targets on a HIP device take the kernels (``ce_kernel_ok`` / ``adversarial_kernel_ok`` tell), every other call
F.cross_entropy.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.nn.modules.loss import _Loss

from . import _lib, ops

_REDUCTION = {"mean": 0, "sum": 1}


# ---------------------------------------------------------------------------------------------------------------------
# FALoss
# ---------------------------------------------------------------------------------------------------------------------

def fa_loss_torch(feature_map1, feature_map2, reduction="mean"):
    """The reference's op sequence (losses.py:122-128): two (B, N, N) similarity matrices and an L1 loss between them."""
    f1, f2 = feature_map1.flatten(2), feature_map2.flatten(2)
    s1 = torch.matmul(f1.transpose(1, 2), f1).flatten(1)
    s2 = torch.matmul(f2.transpose(1, 2), f2).flatten(1)
    return F.l1_loss(s1, s2, reduction=reduction)


def fa_shape_ok(C, N, reduction="mean"):
    """Whether the kernels cover (C channels, N tokens, reduction): tmf_faloss_ok."""
    return reduction in _REDUCTION and bool(_lib.query("tmf_faloss_ok", int(C), int(N), _REDUCTION[reduction]))


def _on_hip_fp32(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


def fa_kernel_ok(feature_map1, feature_map2, reduction="mean"):
    """True when FALoss(reduction=reduction)(feature_map1, feature_map2) runs on the fused kernels."""
    a, b = feature_map1, feature_map2
    if not (_on_hip_fp32(a) and _on_hip_fp32(b)) or a.dim() != 5 or a.shape != b.shape or a.device != b.device:
        return False
    return a.numel() > 0 and fa_shape_ok(a.shape[1], a.shape[2] * a.shape[3] * a.shape[4], reduction)


def _fa_storage(a, b):
    """The two maps as the storage the kernel reads, and its layout flag: NCDHW-contiguous as they are; the channels-last
    storage behind a (B, C, h, w, d) view (sNet's output) as its (B, h, w, d, C) view — no copy either way; any other
    striding is made NCDHW-contiguous first."""
    if a.is_contiguous() and b.is_contiguous():
        return a, b, False
    pa, pb = a.permute(0, 2, 3, 4, 1), b.permute(0, 2, 3, 4, 1)
    if pa.is_contiguous() and pb.is_contiguous():
        return pa, pb, True
    return a.contiguous(), b.contiguous(), False


class FALoss(_Loss):
    __constants__ = ["reduction"]

    def __init__(self, subsample_factor: int = 8, size_average=None, reduce=None, reduction="mean") -> None:
        super().__init__(size_average=None, reduce=None, reduction=reduction)
        self.subsample_factor = subsample_factor          # stored and unused, as in the reference

    def forward(self, feature_map1, feature_map2):
        if not fa_kernel_ok(feature_map1, feature_map2, self.reduction):
            return fa_loss_torch(feature_map1, feature_map2, self.reduction)
        B, C = feature_map1.shape[:2]
        N = feature_map1.numel() // (B * C)
        s1, s2, channels_last = _fa_storage(feature_map1, feature_map2)
        with torch.cuda.device(feature_map1.device):
            return ops.faloss(s1, s2, B, C, N, channels_last, _REDUCTION[self.reduction])


# ---------------------------------------------------------------------------------------------------------------------
# SupConLoss
# ---------------------------------------------------------------------------------------------------------------------

def supcon_loss_torch(features, base_mask, anchors_all, temperature, base_temperature):
    """The formula of the module docstring in plain torch ops.  features (bs, views, d); base_mask (bs, bs) float."""
    bs, views, _ = features.shape
    contrast = features.transpose(0, 1).reshape(views * bs, -1)             # row v * bs + s
    anchors = contrast if anchors_all else features[:, 0]
    count = views if anchors_all else 1
    logits = torch.div(torch.matmul(anchors, contrast.T), temperature)
    logits = logits - logits.max(dim=1, keepdim=True).values.detach()
    not_self = torch.ones(count * bs, views * bs, dtype=base_mask.dtype, device=features.device)
    not_self.fill_diagonal_(0)
    positives = base_mask.repeat(count, views) * not_self
    log_prob = logits - torch.log((torch.exp(logits) * not_self).sum(1, keepdim=True))
    mean_log_prob_pos = (positives * log_prob).sum(1) / positives.sum(1)
    return (-(temperature / base_temperature) * mean_log_prob_pos).mean()


def supcon_shape_ok(bs, views, d):
    """Whether the kernel covers (bs, views, flattened feature length d): tmf_supcon_ok."""
    return bool(_lib.query("tmf_supcon_ok", int(bs), int(views), int(d)))


def supcon_kernel_ok(features, labels=None, mask=None):
    """True when SupConLoss()(features, labels, mask) runs on the fused kernel."""
    if not _on_hip_fp32(features) or features.dim() < 3 or features.numel() == 0:
        return False
    bs, views = features.shape[:2]
    return supcon_shape_ok(bs, views, features.numel() // (bs * views))


class SupConLoss(torch.nn.Module):
    """Supervised contrastive loss (arXiv:2004.11362); with neither labels nor mask the SimCLR loss (arXiv:2002.05709)."""

    def __init__(self, temperature=0.07, contrast_mode="all", base_temperature=0.07):
        super().__init__()
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature

    def forward(self, features, labels=None, mask=None):
        """features: (bsz, n_views, ...); labels: (bsz,); mask: (bsz, bsz), mask[i, j] = 1 if sample j is a positive of
        sample i (may be asymmetric).  Returns a scalar."""
        if features.dim() < 3:
            raise ValueError("`features` needs to be [bsz, n_views, ...], at least 3 dimensions are required")
        use_kernel = supcon_kernel_ok(features, labels, mask)
        if features.dim() > 3:
            features = features.reshape(features.shape[0], features.shape[1], -1)
        bs = features.shape[0]
        dev = features.device
        if labels is not None and mask is not None:
            raise ValueError("Cannot define both `labels` and `mask`")
        if labels is not None:
            labels = labels.contiguous().view(-1)
            if labels.shape[0] != bs:
                raise ValueError("Num of labels does not match num of features")
        if self.contrast_mode not in ("one", "all"):
            raise ValueError("Unknown mode: {}".format(self.contrast_mode))
        anchors_all = self.contrast_mode == "all"

        if use_kernel:
            klabels = kmask = None
            if labels is not None:
                if labels.dtype.is_floating_point or labels.dtype.is_complex:
                    kmask = torch.eq(labels.view(-1, 1), labels.view(1, -1)).float().to(dev)
                else:
                    klabels = labels.to(device=dev, dtype=torch.int64)
            elif mask is not None:
                kmask = mask.float().to(dev).contiguous()
                if kmask.shape != (bs, bs):
                    raise ValueError("`mask` needs to be [bsz, bsz]")
            with torch.cuda.device(dev):
                return ops.supcon_loss(features.contiguous(), klabels, kmask, anchors_all, self.temperature,
                                       self.base_temperature)

        if labels is not None:
            base = torch.eq(labels.view(-1, 1), labels.view(1, -1)).float().to(dev)
        elif mask is not None:
            base = mask.float().to(dev)
        else:
            base = torch.eye(bs, dtype=torch.float32, device=dev)
        return supcon_loss_torch(features, base, anchors_all, self.temperature, self.base_temperature)


# ---------------------------------------------------------------------------------------------------------------------
# CrossEntropyLoss and the adversarial criterion (csrc/criterion.hip)
# ---------------------------------------------------------------------------------------------------------------------

def ce_shape_ok(B, C):
    """Whether the kernels cover B rows of C classes: tmf_ce_ok."""
    return bool(_lib.query("tmf_ce_ok", int(B), int(C)))


def ce_kernel_ok(logits, target, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
    """True when CrossEntropyLoss(weight, ignore_index=..., reduction=..., label_smoothing=...)(logits, target) runs on the
    kernels: fp32 (B, C) logits and int64 (B,) class indices on one HIP device, the default ignore_index and
    label_smoothing, 'mean' or 'sum'."""
    if reduction not in _REDUCTION or ignore_index != -100 or label_smoothing != 0.0:
        return False
    if not _on_hip_fp32(logits) or logits.dim() != 2 or not torch.is_tensor(target):
        return False
    if target.dtype != torch.int64 or target.device != logits.device or target.shape != logits.shape[:1]:
        return False
    if weight is not None and not (_on_hip_fp32(weight) and weight.device == logits.device
                                   and weight.shape == logits.shape[1:]):
        return False
    return ce_shape_ok(logits.shape[0], logits.shape[1])


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """torch.nn.CrossEntropyLoss (same constructor) on tmf_ce_fwd / tmf_ce_bwd: one launch forward, one backward.  Every call
    the kernels do not cover (``ce_kernel_ok``) runs F.cross_entropy with the same arguments."""

    def forward(self, input, target):
        if not ce_kernel_ok(input, target, self.weight, self.ignore_index, self.reduction, self.label_smoothing):
            return F.cross_entropy(input, target, weight=self.weight, ignore_index=self.ignore_index,
                                   reduction=self.reduction, label_smoothing=self.label_smoothing)
        weight = None if self.weight is None else self.weight.contiguous()
        with torch.cuda.device(input.device):
            return ops.cross_entropy(input, target.contiguous(), weight, _REDUCTION[self.reduction])


def adversarial_criterion_torch(output_logits, D_MRI_logits, D_PET_logits, label, weight=None):
    """The criterion of kfold_train_adversarial.py:119-125 in torch ops: (ce_loss, ad_loss)."""
    ce_loss = F.cross_entropy(output_logits, label, weight=weight)
    mri_gt = torch.ones(D_MRI_logits.shape[0], dtype=torch.int64, device=D_MRI_logits.device)
    pet_gt = torch.zeros(D_PET_logits.shape[0], dtype=torch.int64, device=D_PET_logits.device)
    ad_loss = (F.cross_entropy(D_MRI_logits, mri_gt) + F.cross_entropy(D_PET_logits, pet_gt)) / 2
    return ce_loss, ad_loss


def adversarial_kernel_ok(output_logits, D_MRI_logits, D_PET_logits, label, weight=None):
    """True when AdversarialCriterion(weight)(...) runs on the one-launch kernel: the label head as for ``ce_kernel_ok``, the
    two domain heads fp32 (B, 2) on the same device."""
    if not ce_kernel_ok(output_logits, label, weight):
        return False
    want = (output_logits.shape[0], 2)
    return all(_on_hip_fp32(d) and d.device == output_logits.device and tuple(d.shape) == want
               for d in (D_MRI_logits, D_PET_logits))


class AdversarialCriterion(torch.nn.Module):
    """``ce_loss, ad_loss = criterion(output_logits, D_MRI_logits, D_PET_logits, label)``: CE(output_logits, label) and
    (CE(D_MRI_logits, ones) + CE(D_PET_logits, zeros)) / 2, two 0-dim views of one 2-float device tensor (``.base``) from one
    launch; ``(ad_loss + ce_loss).backward()`` is one more.  ``weight`` weighs the classes of the label head."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", weight)

    def forward(self, output_logits, D_MRI_logits, D_PET_logits, label):
        if not adversarial_kernel_ok(output_logits, D_MRI_logits, D_PET_logits, label, self.weight):
            return adversarial_criterion_torch(output_logits, D_MRI_logits, D_PET_logits, label, self.weight)
        weight = None if self.weight is None else self.weight.contiguous()
        with torch.cuda.device(output_logits.device):
            return ops.adversarial_criterion(output_logits, D_MRI_logits, D_PET_logits, label.contiguous(), weight)
