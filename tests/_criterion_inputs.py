"""Inputs of the criterion / epoch-metric tests (tests/test_host_criterion.py, tests/test_gpu_criterion.py),
reproducible from a few integers, and the references both files share: the integer AUC formula and
cal_confusion_metrics restated in numpy."""
import numpy as np

U = 2.0 ** -24

# (B, C) of the value tests; the GPU file adds B = 4096
SHAPES = [(B, C) for C in (2, 3, 10) for B in (1, 8, 16)]
EPOCH_SIZES = (16, 131, 1000, 4096)


def ce_inputs(B, C, scale=3.0, seed=0):
    """(logits float32 (B, C), target int64 (B,), weight float32 (C,) in [0.5, 2))."""
    rs = np.random.RandomState(1000 * C + B + seed)
    logits = (scale * rs.standard_normal((B, C))).astype(np.float32)
    target = rs.randint(0, C, B).astype(np.int64)
    weight = (0.5 + 1.5 * rs.rand(C)).astype(np.float32)
    return logits, target, weight


def adv_inputs(B, C, scale=3.0, seed=0):
    """(logits (B, C), D_MRI_logits (B, 2), D_PET_logits (B, 2), label (B,), weight (C,))."""
    logits, label, weight = ce_inputs(B, C, scale, seed)
    rs = np.random.RandomState(77 + 1000 * C + B + seed)
    d_mri = (scale * rs.standard_normal((B, 2))).astype(np.float32)
    d_pet = (scale * rs.standard_normal((B, 2))).astype(np.float32)
    return logits, d_mri, d_pet, label, weight


def uneven_splits(n, seed=0):
    """Batch boundaries [0, ..., n] with batch sizes between 1 and 37, not all equal."""
    rs = np.random.RandomState(seed + n)
    cuts, at = [0], 0
    while at < n:
        at = min(n, at + int(rs.randint(1, 38)))
        cuts.append(at)
    return cuts


def epoch_inputs(n, seed=0, C=2):
    """An evaluation epoch: random logits, a quarter of the rows exact duplicates of other rows (tied scores), and rows of
    +-40 (scores saturated at 1 and at the smallest values).  -> logits float32 (n, C), label int64 (n,)."""
    rs = np.random.RandomState(31 * n + seed)
    logits = (2.0 * rs.standard_normal((n, C))).astype(np.float32)
    label = rs.randint(0, C, n).astype(np.int64)
    dup = rs.choice(n, n // 4, replace=False)
    logits[dup] = logits[rs.randint(0, n, dup.size)]
    sat = rs.choice(n, max(2, n // 8), replace=False)
    logits[sat] = 0.0
    logits[sat, C - 1] = np.where(rs.rand(sat.size) < 0.5, 40.0, -40.0).astype(np.float32)
    return logits, label


def grid_epoch_inputs(n, seed=0):
    """An epoch on which two fp32 softmax implementations must rank the samples alike: two-class rows (c_k, c_k + 0.05 k),
    k an integer in [-80, 80] and c_k a function of k alone, so equal logit differences are equal ROWS (exact ties in any
    implementation) and different ones give scores at least sigmoid'(4) * 0.05 = 8.8e-4 apart, three orders above the
    score bound u (4 C + 4) = 7e-7; plus rows (0, +-40) and (0, +-50): saturated, and apart by orders of magnitude or
    equal to 1 exactly.  Labels follow the scores loosely, so the AUC is well inside (0.5, 1)."""
    rs = np.random.RandomState(17 * n + seed)
    k = rs.randint(-80, 81, n)
    base = ((k % 7) * 0.25).astype(np.float32)
    logits = np.stack([base, base + (0.05 * k).astype(np.float32)], axis=1).astype(np.float32)
    d = 0.05 * k
    sat = rs.choice(n, max(4, n // 16), replace=False)
    big = rs.choice(np.array([40.0, -40.0, 50.0, -50.0], dtype=np.float32), sat.size)
    logits[sat, 0] = 0.0
    logits[sat, 1] = big
    d[sat] = big
    label = (rs.rand(n) < 1.0 / (1.0 + np.exp(-0.5 * d))).astype(np.int64)
    return logits, label


def auc_integers(scores, labels):
    """T = sum over (positive i, negative j) of 2 [s_i > s_j] + [s_i == s_j], P, N as Python ints: the negatives sorted and
    each positive's count of smaller / equal negatives by binary search — the pair count, in integers."""
    scores = np.asarray(scores)
    labels = np.asarray(labels)
    pos, neg = scores[labels != 0], np.sort(scores[labels == 0])
    below = np.searchsorted(neg, pos, side="left").astype(np.int64)
    upto = np.searchsorted(neg, pos, side="right").astype(np.int64)
    return int((below + upto).sum()), int(pos.size), int(neg.size)


def auc_from_integers(T, P, N):
    return T / (2 * P * N) if P and N else float("nan")


def auc_pairs_dense(scores, labels):
    """The same T by the definition, all P x N pairs (small n only)."""
    scores = np.asarray(scores)
    labels = np.asarray(labels)
    pos, neg = scores[labels != 0], scores[labels == 0]
    return int(2 * (pos[:, None] > neg[None, :]).sum() + (pos[:, None] == neg[None, :]).sum())


def confusion_metrics_numpy(cm):
    """(sensitivity, specificity, f1) of a 2 x 2 matrix, row true / column predicted, class 1 positive."""
    cm = np.asarray(cm, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp, fn, fp, tn = cm[1, 1], cm[1, 0], cm[0, 1], cm[0, 0]
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        return recall, tn / (tn + fp), 2 * precision * recall / (precision + recall)


def ce64(logits, target, weight=None, reduction="mean"):
    """fp64 F.cross_entropy on the same fp32 inputs: (loss, dloss/dlogits (B, C), softmax (B, C), per-sample loss (B,))."""
    import torch
    import torch.nn.functional as F
    x = torch.as_tensor(logits).double().requires_grad_(True)
    y = torch.as_tensor(target)
    w = None if weight is None else torch.as_tensor(weight).double()
    loss = F.cross_entropy(x, y, weight=w, reduction=reduction)
    loss.backward()
    per = F.cross_entropy(x.detach(), y, reduction="none")
    return loss.item(), x.grad.numpy(), torch.softmax(x.detach(), 1).numpy(), per.numpy()


def loss_bound_rows(logits):
    """u (4 C + 3 ln C + 2 R_i + 2) per row (derivation: the docstring of tests/test_gpu_criterion.py)."""
    x = np.asarray(logits, dtype=np.float64)
    C = x.shape[1]
    return U * (4 * C + 3 * np.log(C) + 2 * (x.max(1) - x.min(1)) + 2)
