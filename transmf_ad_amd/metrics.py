"""Epoch metrics that stay on the device: what the reference attaches to every trainer and evaluator
(kfold_train_adversarial.py:178-194 — ignite's Accuracy, Average, ConfusionMatrix, ROC_AUC and Loss), on the kernels of
csrc/criterion.hip.

    from transmf_ad_amd.metrics import TrainMetrics, EvalMetrics, cal_confusion_metrics

On the kernels ``update`` is one launch and no host synchronisation, and ``compute`` makes one device-to-host copy per
epoch.  fp32 logits and int64 labels on a HIP device with 2 to 16 classes take the kernels; a batch of more than 4096
samples goes to ``EvalMetrics.update`` in chunks of 4096 (one launch each, still no synchronisation).  Every other call —
CPU tensors, another dtype, more than 16 classes, a ``TrainMetrics`` batch above 4096 — runs the same formulas in torch ops
on the caller's device, into the same state; that path launches what torch launches and may synchronise (``bincount``
does), so the promise above is the kernel path's alone.

TrainMetrics state, 8 words of 8 bytes: updates, samples (int64); sum ce_loss, sum ad_loss (double); correct predictions
of the label head, of the MRI domain head (target 1) and of the PET domain head (target 0) (int64); one unused.
EvalMetrics state, 2 + C*C + 3 words: sum of the per-sample cross entropy (double); samples; the C x C confusion counts,
row = true class, column = predicted class; and the AUC's integers T, P, N (written by ``compute``).

AUC: T = sum over (positive i, negative j) of 2 [s_i > s_j] + [s_i == s_j] over the fp32 scores softmax(logits)[:, -1],
AUC = T / (2 P N) — the Mann-Whitney statistic, which is the area under the ROC curve with ties counted half (what
scikit-learn's trapezoid rule gives).  Integer counts: exact, independent of the order of the samples.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, losses, ops

_i64 = torch.int64


def cal_confusion_metrics(c_matrix):
    """(sensitivity, specificity, f1) of a 2 x 2 confusion matrix with row = true class, column = predicted class and
    class 1 positive: the formula and return order of utils/utils.py:44-51.  0-dim float64 tensors; an empty denominator
    gives NaN."""
    m = torch.as_tensor(c_matrix).to(torch.float64)
    tn, fp, fn, tp = m[0, 0], m[0, 1], m[1, 0], m[1, 1]
    precision = tp / (tp + fp)
    sensitivity = tp / (tp + fn)                 # = recall
    specificity = tn / (tn + fp)
    f1 = 2 * precision * sensitivity / (precision + sensitivity)
    return sensitivity, specificity, f1


def auc_counts_torch(scores, labels):
    """The AUC's integers (T, P, N) as an int64 tensor, in torch ops: the negatives sorted, each positive's count of smaller
    and of equal negatives by binary search.  A label of 0 is negative, any other positive."""
    pos = scores[labels != 0]
    neg = torch.sort(scores[labels == 0]).values
    below = torch.searchsorted(neg, pos, right=False)             # negatives <  s_i
    upto = torch.searchsorted(neg, pos, right=True)               # negatives <= s_i
    T = (below + upto).sum()                                      # 2 * below + (upto - below)
    return torch.stack([T, T.new_tensor(pos.numel()), T.new_tensor(neg.numel())]).to(_i64)


def _as_f64(words):
    return words.view(torch.float64)


_KERNEL_BATCH = 4096                             # the largest batch tmf_ce_ok takes


def _logits_on_kernel(logits, label):
    """Whether EvalMetrics.update feeds the kernel: ``losses.ce_kernel_ok`` but for the batch size, which is chunked."""
    return logits.dim() == 2 and torch.is_tensor(label) and losses.ce_kernel_ok(logits[:_KERNEL_BATCH], label[:_KERNEL_BATCH])


class TrainMetrics:
    """accuracy, MRI_accuracy, PET_accuracy (ignite Accuracy of the three heads), ce_loss, ad_loss (ignite Average of the
    step's two scalars: means over updates)."""

    def __init__(self):
        self._state = None

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def _state_on(self, device):
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(_lib.TRAIN_METRICS_WORDS, dtype=_i64, device=device)
        return self._state

    def update(self, ce_loss, ad_loss, output_logits, D_MRI_logits, D_PET_logits, label):
        """Adds one step.  ce_loss / ad_loss: the step's scalars, read on the device (the two views AdversarialCriterion
        returns are read in place; other scalars are packed first)."""
        state = self._state_on(output_logits.device)
        if losses.adversarial_kernel_ok(output_logits, D_MRI_logits, D_PET_logits, label):
            pair = _loss_pair(ce_loss, ad_loss, output_logits.device)
            with torch.cuda.device(output_logits.device):
                ops.train_metrics_update(state, pair, output_logits.detach(), D_MRI_logits.detach(), D_PET_logits.detach(),
                                         label.contiguous())
            return
        with torch.no_grad():
            state[0] += 1
            state[1] += output_logits.shape[0]
            sums = _as_f64(state[2:4])
            sums[0] += torch.as_tensor(ce_loss, device=state.device).detach().double()
            sums[1] += torch.as_tensor(ad_loss, device=state.device).detach().double()
            state[4] += (output_logits.argmax(1) == label).sum()
            state[5] += (D_MRI_logits.argmax(1) == 1).sum()
            state[6] += (D_PET_logits.argmax(1) == 0).sum()

    def compute(self):
        if self._state is None:
            raise RuntimeError("TrainMetrics.compute() before any update()")
        host = self._state.cpu()                 # the one device-to-host copy
        updates, samples = int(host[0]), int(host[1])
        if updates == 0:
            raise RuntimeError("TrainMetrics.compute() before any update()")
        sums = _as_f64(host[2:4])
        return {"accuracy": int(host[4]) / samples, "MRI_accuracy": int(host[5]) / samples,
                "PET_accuracy": int(host[6]) / samples, "ce_loss": float(sums[0]) / updates,
                "ad_loss": float(sums[1]) / updates}


def _loss_pair(ce_loss, ad_loss, device):
    """The two step losses as two adjacent device floats: the storage AdversarialCriterion returned, or a packed copy."""
    if (torch.is_tensor(ce_loss) and torch.is_tensor(ad_loss) and ce_loss.dtype == ad_loss.dtype == torch.float32
            and ce_loss.device == ad_loss.device == device and ce_loss.numel() == ad_loss.numel() == 1
            and ce_loss.data_ptr() + 4 == ad_loss.data_ptr()):
        return ce_loss.detach()
    both = [torch.as_tensor(t, dtype=torch.float32, device=device).detach().reshape(()) for t in (ce_loss, ad_loss)]
    return torch.stack(both)


class EvalMetrics:
    """loss (ignite Loss of the cross entropy: the per-sample mean), accuracy, confusion (C x C int64, row true, column
    predicted) and, for two classes, sensitivity, specificity, f1 (``cal_confusion_metrics``) and auc (ignite ROC_AUC over
    softmax(logits)[:, -1]; NaN when a class is absent, where scikit-learn raises)."""

    def __init__(self, num_classes=2):
        if num_classes < 2:
            raise ValueError("num_classes must be at least 2")
        self.num_classes = int(num_classes)
        self._words = 2 + self.num_classes ** 2 + 3
        self._state = self._scores = self._labels = self._workspace = None
        self._n = 0

    def reset(self):
        self._n = 0
        if self._state is not None:
            self._state.zero_()

    @property
    def scores(self):
        """The fp32 scores softmax(logits)[:, -1] of the epoch so far, in the order of the updates (a view, on the device)."""
        return None if self._scores is None else self._scores[:self._n]

    @property
    def labels(self):
        return None if self._labels is None else self._labels[:self._n]

    def _reserve(self, device, more):
        """State and epoch buffers on `device` with room for `more` further samples; the buffers grow geometrically."""
        if self._state is None or self._state.device != device:
            if self._n:
                raise RuntimeError(f"EvalMetrics: update on {device} after updates on {self._state.device}; reset() first")
            self._state = torch.zeros(self._words, dtype=_i64, device=device)
            self._scores = self._labels = self._workspace = None
        need = self._n + more
        if self._scores is None or self._scores.numel() < need:
            cap = max(need, 1024, 2 * (0 if self._scores is None else self._scores.numel()))
            scores = torch.empty(cap, dtype=torch.float32, device=device)
            labels = torch.empty(cap, dtype=_i64, device=device)
            if self._n:
                scores[:self._n] = self._scores[:self._n]
                labels[:self._n] = self._labels[:self._n]
            self._scores, self._labels = scores, labels

    def update(self, logits, label):
        C = self.num_classes
        if logits.dim() != 2 or logits.shape[1] != C:
            raise ValueError(f"EvalMetrics(num_classes={C}): logits of shape {tuple(logits.shape)}")
        B = logits.shape[0]
        self._reserve(logits.device, B)
        state = self._state
        if _logits_on_kernel(logits, label):
            logits, label = logits.detach(), label.contiguous()
            with torch.cuda.device(logits.device):
                for at in range(0, B, _KERNEL_BATCH):            # the host knows every offset: no device cursor
                    ops.eval_metrics_update(state, self._scores, self._labels, self._n + at, logits[at:at + _KERNEL_BATCH],
                                            label[at:at + _KERNEL_BATCH])
        else:
            with torch.no_grad():
                label = label.to(_i64)
                _as_f64(state[0:1])[0] += F.cross_entropy(logits.double(), label, reduction="sum")
                state[1] += B
                state[2:2 + C * C] += torch.bincount(label * C + logits.argmax(1), minlength=C * C)
                self._scores[self._n:self._n + B] = torch.softmax(logits.float(), 1)[:, C - 1]
                self._labels[self._n:self._n + B] = label
        self._n += B

    def compute(self):
        n, C = self._n, self.num_classes
        if n == 0:
            raise RuntimeError("EvalMetrics.compute() before any update()")
        state = self._state
        if C == 2:
            out = state[2 + C * C:]
            if self._scores.is_cuda and _lib.query("tmf_auc_ok", n):
                words = _lib.query("tmf_auc_workspace_bytes", n) // 8
                if self._workspace is None or self._workspace.numel() < words:
                    self._workspace = torch.empty(words, dtype=_i64, device=state.device)
                with torch.cuda.device(state.device):
                    ops.auc_counts(self._scores, self._labels, n, self._workspace, out)
            else:
                out.copy_(auc_counts_torch(self._scores[:n], self._labels[:n]))
        host = state.cpu()                       # the one device-to-host copy
        confusion = host[2:2 + C * C].reshape(C, C).clone()
        result = {"loss": float(_as_f64(host[0:1])[0]) / n, "accuracy": int(confusion.diagonal().sum()) / n,
                  "confusion": confusion}
        if C == 2:
            sen, spe, f1 = cal_confusion_metrics(confusion)
            T, P, N = (int(v) for v in host[2 + C * C:])
            result.update(sensitivity=float(sen), specificity=float(spe), f1=float(f1),
                          auc=T / (2 * P * N) if P and N else float("nan"))
        return result
