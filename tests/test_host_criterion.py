"""CrossEntropyLoss / AdversarialCriterion / TrainMetrics / EvalMetrics without a GPU: on CPU tensors the package runs the
same formulas in torch ops, which pins the semantics — the losses against F.cross_entropy and the oracle bit for bit, the
evaluator's metrics against scikit-learn and the integer AUC formula, the trainer's against a plain-Python restatement of
ignite's Accuracy and Average — plus the C-ABI bindings and the scratch budget of csrc/criterion.hip."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _criterion_inputs as CI                  # noqa: E402
from transmf_ad_amd import losses as L          # noqa: E402
from transmf_ad_amd import metrics as M         # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# 1: the losses on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,C", CI.SHAPES)
def test_cross_entropy_on_cpu_is_f_cross_entropy(B, C, weighted, reduction):
    logits, target, weight = CI.ce_inputs(B, C)
    w = torch.from_numpy(weight) if weighted else None
    y = torch.from_numpy(target)
    x = torch.from_numpy(logits).requires_grad_(True)
    x0 = torch.from_numpy(logits.copy()).requires_grad_(True)
    crit = L.CrossEntropyLoss(weight=w, reduction=reduction)
    assert isinstance(crit, torch.nn.CrossEntropyLoss)
    assert not L.ce_kernel_ok(x, y, w, reduction=reduction)
    loss = crit(x, y)
    want = F.cross_entropy(x0, y, weight=w, reduction=reduction)
    loss.backward()
    want.backward()
    assert torch.equal(loss, want) and torch.equal(x.grad, x0.grad)


def test_cross_entropy_passes_every_other_call_through():
    logits, target, weight = CI.ce_inputs(8, 3)
    x, y = torch.from_numpy(logits), torch.from_numpy(target)
    assert torch.equal(L.CrossEntropyLoss(reduction="none")(x, y), F.cross_entropy(x, y, reduction="none"))
    assert torch.equal(L.CrossEntropyLoss(label_smoothing=0.1)(x, y), F.cross_entropy(x, y, label_smoothing=0.1))
    assert torch.equal(L.CrossEntropyLoss(ignore_index=1)(x, y), F.cross_entropy(x, y, ignore_index=1))
    prob = torch.softmax(torch.from_numpy(CI.ce_inputs(8, 3, seed=1)[0]), 1)
    assert torch.equal(L.CrossEntropyLoss()(x, prob), F.cross_entropy(x, prob))
    assert torch.equal(L.CrossEntropyLoss()(x.double(), y), F.cross_entropy(x.double(), y))
    # positional constructor order of torch.nn.CrossEntropyLoss
    c = L.CrossEntropyLoss(torch.from_numpy(weight), None, -100, None, "sum", 0.0)
    assert c.reduction == "sum" and c.ignore_index == -100 and torch.equal(c.weight, torch.from_numpy(weight))
    assert not L.ce_kernel_ok(x, y) and not L.ce_kernel_ok(x, y, reduction="none")
    assert L.ce_shape_ok(1, 2) and L.ce_shape_ok(4096, 16) and L.ce_shape_ok(8, 2)
    assert not L.ce_shape_ok(0, 2) and not L.ce_shape_ok(4097, 2) and not L.ce_shape_ok(8, 1) and not L.ce_shape_ok(8, 17)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,C", CI.SHAPES)
def test_adversarial_criterion_on_cpu_is_the_reference_formula(B, C, weighted):
    from oracle import tmf_oracle
    logits, d_mri, d_pet, label, weight = CI.adv_inputs(B, C)
    w = torch.from_numpy(weight) if weighted else None
    y = torch.from_numpy(label)
    ours = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (logits, d_mri, d_pet)]
    ref = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (logits, d_mri, d_pet)]
    crit = L.AdversarialCriterion(weight=w)
    assert not L.adversarial_kernel_ok(*ours, y, w)
    ce_loss, ad_loss = crit(*ours, y)
    ce_ref = F.cross_entropy(ref[0], y, weight=w)
    ad_ref = (F.cross_entropy(ref[1], torch.ones(B, dtype=torch.int64))
              + F.cross_entropy(ref[2], torch.zeros(B, dtype=torch.int64))) / 2
    assert torch.equal(ce_loss, ce_ref) and torch.equal(ad_loss, ad_ref)
    all_loss = ad_loss + ce_loss
    all_loss.backward()
    (ad_ref + ce_ref).backward()
    for a, b in zip(ours, ref):
        assert torch.equal(a.grad, b.grad)
    if not weighted:
        with torch.no_grad():
            assert torch.equal(all_loss, tmf_oracle.adversarial_loss(ref[0], ref[1], ref[2], y))


# ---------------------------------------------------------------------------------------------------------------------
# 2: EvalMetrics against scikit-learn
# ---------------------------------------------------------------------------------------------------------------------

def feed(em, logits, label, cuts):
    for a, b in zip(cuts[:-1], cuts[1:]):
        em.update(torch.from_numpy(logits[a:b]), torch.from_numpy(label[a:b]))


@pytest.mark.parametrize("n", CI.EPOCH_SIZES)
def test_eval_metrics_on_cpu_against_the_integer_formula_and_sklearn(n):
    logits, label = CI.epoch_inputs(n)
    em = M.EvalMetrics()
    feed(em, logits, label, CI.uneven_splits(n))
    got = em.compute()
    scores = torch.softmax(torch.from_numpy(logits), 1)[:, -1].numpy()
    assert scores.dtype == np.float32 and np.array_equal(em.scores.numpy(), scores) and np.array_equal(em.labels.numpy(), label)
    pred = logits.argmax(1)
    # the numpy integer formula: the second reference, always there
    T, P, N = CI.auc_integers(scores, label)
    if n <= 1000:
        assert T == CI.auc_pairs_dense(scores, label)
    assert got["auc"] == CI.auc_from_integers(T, P, N)
    cm = np.zeros((2, 2), dtype=np.int64)
    np.add.at(cm, (label, pred), 1)
    assert got["confusion"].dtype == torch.int64 and np.array_equal(got["confusion"].numpy(), cm)
    assert got["accuracy"] == float((pred == label).sum()) / n
    sen, spe, f1 = CI.confusion_metrics_numpy(cm)
    assert (got["sensitivity"], got["specificity"], got["f1"]) == (sen, spe, f1)
    # loss: the fp64 per-sample mean, to fp64 rounding of a sum of n terms
    per = CI.ce64(logits, label)[3]
    want = math.fsum(per) / n
    assert abs(got["loss"] - want) <= n * 2.0 ** -52 * float(np.abs(per).max())
    # scikit-learn
    skm = pytest.importorskip("sklearn.metrics")
    auc = skm.roc_auc_score(label, scores)
    print(f"n={n}: auc {got['auc']!r}, roc_auc_score {auc!r}, difference {got['auc'] - auc!r}")
    assert abs(got["auc"] - auc) <= 1e-15
    assert np.array_equal(got["confusion"].numpy(), skm.confusion_matrix(label, pred, labels=[0, 1]))
    assert got["accuracy"] == skm.accuracy_score(label, pred)


def test_cal_confusion_metrics_formula_and_order():
    cm = np.array([[50, 7], [3, 40]])
    sen, spe, f1 = M.cal_confusion_metrics(torch.from_numpy(cm))
    assert (float(sen), float(spe)) == (40 / 43, 50 / 57)
    precision = 40 / 47
    assert abs(float(f1) - 2 * precision * (40 / 43) / (precision + 40 / 43)) <= 2.0 ** -52
    assert tuple(float(v) for v in M.cal_confusion_metrics(cm)) == CI.confusion_metrics_numpy(cm)
    assert all(math.isnan(float(v)) for v in M.cal_confusion_metrics(np.zeros((2, 2))))


def test_eval_metrics_one_class_epoch_reset_and_repeat():
    logits, label = CI.epoch_inputs(131)
    em = M.EvalMetrics()
    with pytest.raises(RuntimeError):
        em.compute()
    feed(em, logits, np.ones_like(label), CI.uneven_splits(131))
    one_class = em.compute()
    assert math.isnan(one_class["auc"]) and one_class["confusion"][0].sum() == 0
    em.reset()
    with pytest.raises(RuntimeError):
        em.compute()
    feed(em, logits, label, CI.uneven_splits(131))
    first = em.compute()
    again = em.compute()                        # compute() does not change the state
    em.reset()
    feed(em, logits, label, CI.uneven_splits(131, seed=5))
    second = em.compute()
    for k in ("auc", "accuracy", "sensitivity", "specificity", "f1"):
        assert first[k] == second[k] == again[k]
    assert torch.equal(first["confusion"], second["confusion"])
    assert abs(first["loss"] - second["loss"]) <= 131 * 2.0 ** -52 * first["loss"]
    assert int(first["confusion"].sum()) == 131


def test_eval_metrics_more_classes_and_auc_torch_formula():
    logits, label = CI.epoch_inputs(131, C=3)
    em = M.EvalMetrics(num_classes=3)
    feed(em, logits, label, CI.uneven_splits(131))
    got = em.compute()
    cm = np.zeros((3, 3), dtype=np.int64)
    np.add.at(cm, (label, logits.argmax(1)), 1)
    assert np.array_equal(got["confusion"].numpy(), cm) and "auc" not in got
    with pytest.raises(ValueError):
        em.update(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64))
    s = torch.tensor([0.5, 0.5, 0.1, 0.9, 0.5], dtype=torch.float32)
    y = torch.tensor([1, 0, 1, 0, 0])
    # pairs (positive, negative): (.5,.5) tie 1, (.5,.9) 0, (.5,.5) tie 1, (.1,*) 0
    assert M.auc_counts_torch(s, y).tolist() == [2, 2, 3]


# ---------------------------------------------------------------------------------------------------------------------
# 3: TrainMetrics
# ---------------------------------------------------------------------------------------------------------------------

def test_train_metrics_on_cpu_match_ignite_accuracy_and_average():
    tm = M.TrainMetrics()
    with pytest.raises(RuntimeError):
        tm.compute()
    correct = {"accuracy": 0, "MRI_accuracy": 0, "PET_accuracy": 0}
    seen, ce_items, ad_items = 0, [], []
    crit = L.AdversarialCriterion()
    for step, B in enumerate((8, 3, 16, 1, 5)):
        logits, d_mri, d_pet, label, _ = CI.adv_inputs(B, 2, seed=step)
        if step == 2:
            logits[0] = 1.5                     # a tied row: argmax is the first maximal index, class 0
        t = [torch.from_numpy(a) for a in (logits, d_mri, d_pet, label)]
        ce_loss, ad_loss = crit(*t)
        tm.update(ce_loss, ad_loss, *t)
        # ignite Accuracy: correct predictions over samples seen; Average of a scalar: the mean over updates
        for name, lo, y in (("accuracy", logits, label), ("MRI_accuracy", d_mri, np.ones(B)), ("PET_accuracy", d_pet, np.zeros(B))):
            for row, yi in zip(lo, y):
                best = 0
                for c in range(1, len(row)):
                    if row[c] > row[best]:
                        best = c
                correct[name] += int(best == yi)
        seen += B
        ce_items.append(ce_loss.item())
        ad_items.append(ad_loss.item())
    got = tm.compute()
    assert seen == 33
    for name, n in correct.items():
        assert got[name] == n / seen
    assert abs(got["ce_loss"] - sum(ce_items) / 5) <= 5 * 2.0 ** -52 * max(ce_items)
    assert abs(got["ad_loss"] - sum(ad_items) / 5) <= 5 * 2.0 ** -52 * max(ad_items)
    tm.reset()
    with pytest.raises(RuntimeError):
        tm.compute()
    tm.update(0.25, 0.5, *[torch.from_numpy(a) for a in CI.adv_inputs(4, 2)[:4]])      # plain floats are taken too
    assert tm.compute()["ce_loss"] == 0.25 and tm.compute()["ad_loss"] == 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 4, 5: symbols and resources
# ---------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("tmf_ce_ok", "tmf_ce_fwd", "tmf_ce_bwd", "tmf_adv_criterion_fwd", "tmf_adv_criterion_bwd",
               "tmf_train_metrics_update", "tmf_eval_metrics_update", "tmf_auc_ok", "tmf_auc_workspace_bytes", "tmf_auc")


def test_new_symbols_are_bound_and_validate_arguments():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    import transmf_ad_amd
    assert not hasattr(transmf_ad_amd, "AdversarialCriterion") and not hasattr(transmf_ad_amd, "TrainMetrics")
    assert _lib.query("tmf_auc_ok", 1) and _lib.query("tmf_auc_ok", 65536) and not _lib.query("tmf_auc_ok", 0)
    assert _lib.query("tmf_auc_workspace_bytes", 1) == 8
    assert _lib.query("tmf_auc_workspace_bytes", 65536) == 64 * 32 * 8
    assert _lib.query("tmf_auc_workspace_bytes", 0) == 0
    a = 16                                       # a non-NULL pointer value; nothing is launched on a refused call
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_ce_fwd", None, a, None, a, None, 8, 2, 0, None)
    with pytest.raises(_lib.TmfError, match="2 <= C <= 16"):
        _lib.call("tmf_ce_fwd", a, a, None, a, None, 8, 17, 0, None)
    with pytest.raises(_lib.TmfError, match="1 <= B <= 4096"):
        _lib.call("tmf_ce_fwd", a, a, None, a, None, 4097, 2, 0, None)
    with pytest.raises(_lib.TmfError, match="reduction"):
        _lib.call("tmf_ce_fwd", a, a, None, a, None, 8, 2, 2, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_ce_bwd", a, None, a, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="2 <= C <= 16"):
        _lib.call("tmf_ce_bwd", a, a, a, 8, 1, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_adv_criterion_fwd", a, a, None, a, None, a, None, None, None, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="go together"):
        _lib.call("tmf_adv_criterion_fwd", a, a, a, a, None, a, a, None, a, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="1 <= B <= 4096"):
        _lib.call("tmf_adv_criterion_fwd", a, a, a, a, None, a, None, None, None, 0, 2, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_adv_criterion_bwd", a, a, a, None, None, a, a, None, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="2 <= C <= 16"):
        _lib.call("tmf_adv_criterion_bwd", a, a, a, None, None, a, a, a, 8, 40, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_train_metrics_update", None, a, a, a, a, a, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="1 <= B <= 4096"):
        _lib.call("tmf_train_metrics_update", a, a, a, a, a, a, 5000, 2, None)
    with pytest.raises(_lib.TmfError, match="8-byte aligned"):
        _lib.call("tmf_train_metrics_update", 12, a, a, a, a, a, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_eval_metrics_update", a, a, None, 0, a, a, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="2 <= C <= 16"):
        _lib.call("tmf_eval_metrics_update", a, a, a, 0, a, a, 8, 17, None)
    with pytest.raises(_lib.TmfError, match="negative"):
        _lib.call("tmf_eval_metrics_update", a, a, a, -1, a, a, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_auc", a, a, 100, None, a, None)
    with pytest.raises(_lib.TmfError, match="1 <= n <= 65536"):
        _lib.call("tmf_auc", a, a, 65537, a, a, None)
    with pytest.raises(_lib.TmfError, match="8-byte aligned"):
        _lib.call("tmf_auc", a, a, 100, a, 12, None)


@pytest.fixture(scope="module")
def criterion_kernels():
    from tools import resources as R
    obj = os.path.join(R.CSRC, "criterion.o")
    if not os.path.exists(obj):
        pytest.skip("objects not built (python -m transmf_ad_amd.build)")
    if not os.path.exists(f"{R.LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm llvm tools not present")
    return R.kernels_of(obj)


def test_criterion_kernels_use_no_scratch(criterion_kernels):
    names = " ".join(k["name"] for k in criterion_kernels)
    for want in ("ce_fwd_kernel", "adv_fwd_kernel", "scale3_kernel", "train_metrics_kernel", "eval_metrics_kernel",
                 "auc_pairs_kernel", "auc_finalize_kernel"):
        assert want in names, want
    assert len(criterion_kernels) == 7
    for k in criterion_kernels:
        print(k)
        assert k.get("scratch", 0) == 0, k
        assert k["vgpr"] <= 128, k
