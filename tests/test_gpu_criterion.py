"""CrossEntropyLoss / AdversarialCriterion / TrainMetrics / EvalMetrics on the kernels of csrc/criterion.hip (MI355X):
values under bounds DERIVED from fp32 rounding, exact integer statistics, determinism, launch counts, no host
synchronisation, and three train steps of model_CNN_ad.

The bounds.  u = 2^-24 (every fp32 operation rounds to nearest: relative error <= u); R_i = max - min of row i; C classes.
expf and logf are the accurate device-library functions, taken at 2 ulp: HIP's math API reference (the table of
single-precision functions, "maximum ULP difference" column) lists expf and logf below that, and the device library's
own documentation (ROCm-Device-Libs, doc/OCML.md) states that its fp32 functions meet the OpenCL accuracy table.  One ulp
of a result v is at most 2 u |v|, so 2 ulp is a relative error of at most 4u.

The kernel computes, for a row x and target y:  m = max x (exact);  d_c = fl(x_c - m) <= 0;  e_c = expf(d_c);
s = e_0 + ... + e_{C-1} in fp32;  l = fl(logf(s) - fl(x_y - m));  p_c = fl(e_c / s).
 * d_c carries u |d_c|; through exp that is a relative error u |d_c| of e_c, an absolute one of u |d_c| e^{d_c} <= u / e
   (t e^-t <= 1/e).  With expf's 4u:  |e_c - exp(x_c - m)| <= 4u e_c + u / e.
 * s has C terms in [0, 1] and s >= 1 (the maximal term is 1): the C - 1 additions add at most (C - 1) u s, so
   |s - S| <= S u (4 + C / e + C - 1) <= S u (1.37 C + 3)                                                     (rel. error of s).
 * log: |log s - log S| <= u (1.37 C + 3) (first order), logf adds 4u log s <= 4u ln C.  fl(x_y - m) carries u R_i.  The last
   subtraction rounds its result l <= R_i + ln C: u (R_i + ln C).  In all
       |l - l64| <= u (1.37 C + 3 + 5 ln C + 2 R_i)  <=  u (4 C + 3 ln C + 2 R_i + 2),
   the right side being the bound used below (2.63 C - 1 >= 2 ln C for every C >= 2).
 * probabilities: |p_c - P_c| <= P_c u (4 + 1.37 C + 3 + 1) + u / e <= u (1.37 C + 8.4) <= u (4 C + 4) for C >= 2.
 * 'sum' / 'mean' (weights w_i = weight[y_i], or 1; W = sum w_i): the kernel rounds w_i l_i once (u w_i l_i), adds the terms
   and W in double (2^-53: not counted) and rounds the quotient to fp32 once:
       |L - L64| <= sum_i w_i (b_i + u l_i) / W + 2 u |L64|        (b_i the per-sample bound; 'sum': W = 1).
   losses[1] of the adversarial criterion is half the sum of two such means: half the sum of their bounds.
 * gradients: g_ic = k_i (p_ic - [c == y_i]) with k_i = fl(fl(1 / W) w_i) (relative error 2u; 'sum': W = 1).  p carries
   u (4 C + 4), the subtraction and the product round once each, and |p - [c == y]| <= 1:
       |g_ic - g64_ic| <= (w_i / W) u (4 C + 8).
   The domain heads carry the factor 1/2, a power of two and so exact: half the bound.  The backward multiplies by the
   device scalar t autograd hands over.  t = 1 (loss.backward(), ad_loss + ce_loss) is exact and the bound stays; any other
   t rounds once more, |t| times the bound plus u |t g64|, which (w_i / W) |t| u (4 C + 9) covers (|g64| <= w_i / W).
Nothing here is a measured tolerance."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _criterion_inputs as CI

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
U = CI.U


def _L():
    from transmf_ad_amd import losses
    return losses


def _M():
    from transmf_ad_amd import metrics
    return metrics


def dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def loss_bound(logits, target, weight, reduction, loss64):
    """sum_i w_i (b_i + u l_i) / W + 2 u |L64| (module docstring)."""
    per = CI.ce64(logits, target)[3]
    w = np.ones(len(target)) if weight is None else np.asarray(weight, dtype=np.float64)[target]
    W = w.sum() if reduction == "mean" else 1.0
    return float((w * (CI.loss_bound_rows(logits) + U * per)).sum() / W + 2 * U * abs(loss64))


def grad_bound(logits, target, weight, reduction, half=1.0, t=1.0):
    """(w_i / W) half |t| u (4 C + 8) per row, as a (B, 1) array; 4 C + 9 when the backward scales by a t other than 1
    (module docstring).  half: the exact 1/2 of the domain heads."""
    assert half in (1.0, 0.5)
    C = logits.shape[1]
    w = np.ones(len(target)) if weight is None else np.asarray(weight, dtype=np.float64)[target]
    W = w.sum() if reduction == "mean" else 1.0
    return (w / W * half * abs(t) * U * (4 * C + (8 if abs(t) == 1.0 else 9)))[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# 6: values
# ---------------------------------------------------------------------------------------------------------------------

VALUE_SHAPES = CI.SHAPES + [(4096, 2), (4096, 16), (257, 16)]


@pytest.mark.parametrize("scale", [0.1, 3.0, 30.0])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,C", VALUE_SHAPES)
def test_cross_entropy_against_fp64(B, C, weighted, reduction, scale):
    L = _L()
    logits, target, weight = CI.ce_inputs(B, C, scale)
    w = weight if weighted else None
    x, y = dev(logits, grad=True), dev(target)
    crit = L.CrossEntropyLoss(weight=None if w is None else dev(w), reduction=reduction)
    assert L.ce_kernel_ok(x, y, crit.weight, reduction=reduction)
    loss = crit(x, y)
    assert type(loss.grad_fn).__name__ == "CrossEntropyFnBackward"
    loss.backward()
    torch.cuda.synchronize()
    loss64, g64, _p, _per = CI.ce64(logits, target, w, reduction)
    lb = loss_bound(logits, target, w, reduction, loss64)
    gb = grad_bound(logits, target, w, reduction)
    le = abs(loss.item() - loss64)
    ge = np.abs(x.grad.cpu().numpy().astype(np.float64) - g64)
    ref32 = F.cross_entropy(torch.from_numpy(logits), torch.from_numpy(target),
                            weight=None if w is None else torch.from_numpy(w), reduction=reduction).item()
    print(f"B={B} C={C} w={weighted} {reduction} scale={scale}: loss error / bound {le / lb:.3f} (torch fp32 "
          f"{abs(ref32 - loss64) / lb:.3f}), gradient error / bound {(ge / gb).max():.3f}")
    assert le <= lb
    assert np.all(ge <= gb)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,C", CI.SHAPES + [(4096, 2), (4096, 16)])
def test_adversarial_criterion_against_the_three_ce_formula_in_fp64(B, C, weighted):
    L = _L()
    logits, d_mri, d_pet, label, weight = CI.adv_inputs(B, C)
    w = weight if weighted else None
    ones, zeros = np.ones(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    ce64, g_ce, _, _ = CI.ce64(logits, label, w)
    m64, g_m, _, _ = CI.ce64(d_mri, ones)
    p64, g_p, _, _ = CI.ce64(d_pet, zeros)
    ad64 = (m64 + p64) / 2
    ce_b = loss_bound(logits, label, w, "mean", ce64)
    ad_b = (loss_bound(d_mri, ones, None, "mean", m64) + loss_bound(d_pet, zeros, None, "mean", p64)) / 2
    crit = L.AdversarialCriterion(weight=None if w is None else dev(w))
    y = dev(label)
    # backward of ad_loss + ce_loss, of ce_loss alone, of 3 * ad_loss: grads present, absent, scaled
    for which, t_ce, t_ad in (("ad_loss + ce_loss", 1.0, 1.0), ("ce_loss", 1.0, 0.0), ("3 * ad_loss", 0.0, 3.0)):
        xs = [dev(a, grad=True) for a in (logits, d_mri, d_pet)]
        assert L.adversarial_kernel_ok(*xs, y, crit.weight)
        ce_loss, ad_loss = crit(*xs, y)
        assert ce_loss.dim() == 0 and ad_loss.dim() == 0 and ce_loss._base is ad_loss._base and ce_loss._base.shape == (2,)
        total = {"ad_loss + ce_loss": lambda: ad_loss + ce_loss, "ce_loss": lambda: ce_loss, "3 * ad_loss": lambda: 3 * ad_loss}[which]()
        total.backward()
        torch.cuda.synchronize()
        assert abs(ce_loss.item() - ce64) <= ce_b, (ce_loss.item(), ce64, ce_b)
        assert abs(ad_loss.item() - ad64) <= ad_b, (ad_loss.item(), ad64, ad_b)
        worst = 0.0
        for x, g64, t, bound in ((xs[0], g_ce, t_ce, grad_bound(logits, label, w, "mean", t=t_ce)),
                                 (xs[1], g_m / 2, t_ad, grad_bound(d_mri, ones, None, "mean", half=0.5, t=t_ad)),
                                 (xs[2], g_p / 2, t_ad, grad_bound(d_pet, zeros, None, "mean", half=0.5, t=t_ad))):
            got = x.grad.cpu().numpy().astype(np.float64)
            if t == 0.0:
                assert not got.any()            # an absent grad is zero
                continue
            err = np.abs(got - t * g64)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), which
        print(f"B={B} C={C} w={weighted} {which}: ce error / bound {abs(ce_loss.item() - ce64) / ce_b:.3f}, ad "
              f"{abs(ad_loss.item() - ad64) / ad_b:.3f}, worst gradient error / bound {worst:.3f}")


def test_ignored_and_no_grad_calls():
    """-100 (the default ignore_index) has weight 0, as in torch; a call that wants no gradient writes none."""
    L = _L()
    logits, target, _ = CI.ce_inputs(16, 3)
    target = target.copy()
    target[[2, 7]] = -100
    x, y = dev(logits, grad=True), dev(target)
    loss = L.CrossEntropyLoss()(x, y)
    loss.backward()
    keep = target != -100
    loss64, g64, _, _ = CI.ce64(logits[keep], target[keep])
    assert abs(loss.item() - loss64) <= loss_bound(logits[keep], target[keep], None, "mean", loss64)
    g = x.grad.cpu().numpy()
    assert not g[~keep].any()
    assert np.all(np.abs(g[keep].astype(np.float64) - g64) <= grad_bound(logits[keep], target[keep], None, "mean"))
    with torch.no_grad():
        again = L.CrossEntropyLoss()(x, y)
    assert again.grad_fn is None and torch.equal(again, loss.detach())


# ---------------------------------------------------------------------------------------------------------------------
# 7: exact statistics
# ---------------------------------------------------------------------------------------------------------------------

def feed(em, logits, label, cuts):
    x, y = dev(logits), dev(label)
    for a, b in zip(cuts[:-1], cuts[1:]):
        em.update(x[a:b], y[a:b])


def cuts_for(n, seed=0):
    """Uneven batches; the 65 536 case in batches of up to 4096 (the kernel's largest), uneven as well."""
    if n <= 4096:
        return CI.uneven_splits(n, seed)
    rs = np.random.RandomState(n + seed)
    cuts, at = [0], 0
    while at < n:
        at = min(n, at + int(rs.randint(2048, 4097)))
        cuts.append(at)
    return cuts


@pytest.mark.parametrize("n", CI.EPOCH_SIZES + (65536,))
def test_eval_metrics_exact_statistics(n):
    M = _M()
    logits, label = CI.epoch_inputs(n)
    em = M.EvalMetrics()
    feed(em, logits, label, cuts_for(n))
    got = em.compute()
    scores = em.scores.cpu().numpy()
    assert scores.dtype == np.float32 and scores.shape == (n,) and np.array_equal(em.labels.cpu().numpy(), label)
    # confusion and accuracy: exact, against the host argmax
    pred = logits.argmax(1)
    cm = np.zeros((2, 2), dtype=np.int64)
    np.add.at(cm, (label, pred), 1)
    assert np.array_equal(got["confusion"].numpy(), cm)
    assert got["accuracy"] == float((pred == label).sum()) / n
    assert (got["sensitivity"], got["specificity"], got["f1"]) == CI.confusion_metrics_numpy(cm)
    # AUC: ==, against the integer formula on the scores the kernel stored
    T, P, N = CI.auc_integers(scores, label)
    assert got["auc"] == CI.auc_from_integers(T, P, N)
    # the stored scores against fp64 softmax; the loss against the fp64 per-sample mean
    _l, _g, p64, per = CI.ce64(logits, label)
    se = np.abs(scores.astype(np.float64) - p64[:, 1]).max()
    lb = float(CI.loss_bound_rows(logits).mean())
    le = abs(got["loss"] - math.fsum(per) / n)
    print(f"n={n}: score error / bound {se / (U * 12):.3f}, loss error / bound {le / lb:.3f}, auc {got['auc']!r}")
    assert se <= U * (4 * 2 + 4)
    assert le <= lb
    skm = pytest.importorskip("sklearn.metrics")
    assert np.array_equal(got["confusion"].numpy(), skm.confusion_matrix(label, pred, labels=[0, 1]))
    assert got["accuracy"] == skm.accuracy_score(label, pred)


@pytest.mark.parametrize("n", CI.EPOCH_SIZES + (65536,))
def test_eval_metrics_auc_end_to_end_against_roc_auc_score(n):
    """The kernel's own fp32 scores against roc_auc_score over torch's softmax on the host, on inputs whose ranking no
    fp32 softmax can change (CI.grid_epoch_inputs)."""
    M = _M()
    logits, label = CI.grid_epoch_inputs(n)
    em = M.EvalMetrics()
    feed(em, logits, label, cuts_for(n, seed=3))
    got = em.compute()
    host_scores = torch.softmax(torch.from_numpy(logits), 1)[:, -1].numpy()
    T, P, N = CI.auc_integers(host_scores, label)
    want = CI.auc_from_integers(T, P, N)
    print(f"n={n}: auc {got['auc']!r}, integer formula on the host's scores {want!r}")
    assert 0.5 < want < 1.0
    assert got["auc"] == want
    skm = pytest.importorskip("sklearn.metrics")
    auc = skm.roc_auc_score(label, host_scores)
    print(f"n={n}: roc_auc_score {auc!r}, difference {got['auc'] - auc!r}")
    assert abs(got["auc"] - auc) <= 1e-15


def test_eval_metrics_one_class_more_classes_and_the_torch_auc_above_the_kernel_size():
    M = _M()
    logits, label = CI.epoch_inputs(131)
    em = M.EvalMetrics()
    feed(em, logits, np.zeros_like(label), CI.uneven_splits(131))
    assert math.isnan(em.compute()["auc"])
    em.reset()
    feed(em, logits, label, CI.uneven_splits(131))
    first = em.compute()
    em.reset()
    feed(em, logits, label, CI.uneven_splits(131))
    second = em.compute()
    assert first["auc"] == second["auc"] and first["loss"] == second["loss"] and torch.equal(first["confusion"], second["confusion"])
    logits3, label3 = CI.epoch_inputs(1000, C=3)
    em3 = M.EvalMetrics(num_classes=3)
    feed(em3, logits3, label3, CI.uneven_splits(1000))
    cm = np.zeros((3, 3), dtype=np.int64)
    np.add.at(cm, (label3, logits3.argmax(1)), 1)
    assert np.array_equal(em3.compute()["confusion"].numpy(), cm)
    # 65 537 samples: past tmf_auc_ok, the same integers from torch ops on the device
    n = 65537
    lg, lb = CI.grid_epoch_inputs(n)
    big = M.EvalMetrics()
    feed(big, lg, lb, cuts_for(n))
    got = big.compute()
    T, P, N = CI.auc_integers(big.scores.cpu().numpy(), lb)
    assert got["auc"] == CI.auc_from_integers(T, P, N)


def test_train_metrics_on_the_device():
    L, M = _L(), _M()
    tm, host = M.TrainMetrics(), M.TrainMetrics()
    crit = L.AdversarialCriterion()
    ce_items, ad_items = [], []
    for step, B in enumerate((8, 3, 16, 1, 5)):
        logits, d_mri, d_pet, label, _ = CI.adv_inputs(B, 2, seed=step)
        if step == 2:
            logits[0] = 1.5                     # a tie: the first maximal index
        t = [dev(a) for a in (logits, d_mri, d_pet, label)]
        ce_loss, ad_loss = crit(*t)
        tm.update(ce_loss, ad_loss, *t)
        ce_items.append(ce_loss.item())
        ad_items.append(ad_loss.item())
        host.update(ce_items[-1], ad_items[-1], *[torch.from_numpy(a) for a in (logits, d_mri, d_pet, label)])
    got, want = tm.compute(), host.compute()
    for k in ("accuracy", "MRI_accuracy", "PET_accuracy"):
        assert got[k] == want[k], k
    assert abs(got["ce_loss"] - want["ce_loss"]) <= 5 * 2.0 ** -52 * max(ce_items)
    assert abs(got["ad_loss"] - want["ad_loss"]) <= 5 * 2.0 ** -52 * max(ad_items)
    # separate scalars (the stock criterion's) are packed and read on the device too
    tm.reset()
    t = [dev(a) for a in CI.adv_inputs(8, 2)[:4]]
    ce = F.cross_entropy(t[0], t[3])
    tm.update(ce, ce * 2, *t)
    r = tm.compute()
    assert r["ce_loss"] == ce.item() and r["ad_loss"] == (ce * 2).item()


# ---------------------------------------------------------------------------------------------------------------------
# 8: determinism
# ---------------------------------------------------------------------------------------------------------------------

def test_every_entry_is_bitwise_reproducible():
    L, M = _L(), _M()

    def run():
        out = []
        logits, target, weight = CI.ce_inputs(4096, 16)
        x = dev(logits, grad=True)
        loss = L.CrossEntropyLoss(weight=dev(weight))(x, dev(target))
        loss.backward()
        out += [loss.detach(), x.grad]
        a = CI.adv_inputs(257, 10)
        xs = [dev(v, grad=True) for v in a[:3]]
        ce_loss, ad_loss = L.AdversarialCriterion()(*xs, dev(a[3]))
        (ad_loss + ce_loss).backward()
        out += [ce_loss.detach(), ad_loss.detach()] + [v.grad for v in xs]
        tm = M.TrainMetrics()
        tm.update(ce_loss, ad_loss, *[v.detach() for v in xs], dev(a[3]))
        out.append(tm._state.clone())
        em = M.EvalMetrics()
        lg, lb = CI.epoch_inputs(4096)
        feed(em, lg, lb, cuts_for(4096))
        em.compute()
        out += [em._state.clone(), em.scores.clone()]
        torch.cuda.synchronize()
        return [t.cpu() for t in out]
    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_batch_splits_do_not_change_the_epoch():
    M = _M()
    n = 4096
    logits, label = CI.epoch_inputs(n)
    results = []
    for cuts in (cuts_for(n), cuts_for(n, seed=9), [0, n], [0, 1, n]):
        em = M.EvalMetrics()
        feed(em, logits, label, cuts)
        results.append(em.compute())
    for r in results[1:]:
        assert torch.equal(r["confusion"], results[0]["confusion"]) and r["auc"] == results[0]["auc"]
        assert abs(r["loss"] - results[0]["loss"]) <= n * 2.0 ** -52 * results[0]["loss"]


# ---------------------------------------------------------------------------------------------------------------------
# 9: launch counts, no synchronisation
# ---------------------------------------------------------------------------------------------------------------------

def count_launches(fn):
    """Device kernels launched by fn() (torch.profiler; memory copies / fills of the runtime are not kernels)."""
    from torch.profiler import ProfilerActivity, profile
    from torch.autograd import DeviceType
    fn()                                         # warm-up: lazy module loading, allocator
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA
             and not e.name.lower().startswith(("memcpy", "memset"))]
    return names


def test_launch_counts():
    L, M = _L(), _M()
    logits, d_mri, d_pet, label, _ = CI.adv_inputs(8, 2)
    xs = [dev(a, grad=True) for a in (logits, d_mri, d_pet)]
    y = dev(label)
    ones, zeros = torch.ones_like(y), torch.zeros_like(y)
    crit, stock = L.AdversarialCriterion(), torch.nn.CrossEntropyLoss()
    out = {}

    def adv_fwd():
        out["losses"] = crit(*xs, y)
    names = count_launches(adv_fwd)
    print("AdversarialCriterion forward:", names)
    assert len(names) == 1, names

    unit = torch.ones((), device=DEV)

    def adv_bwd():
        for x in xs:
            x.grad = None
        torch.autograd.backward(list(out["losses"]), [unit, unit], retain_graph=True)
    names = count_launches(adv_bwd)
    print("AdversarialCriterion backward:", names)
    assert len(names) == 1, names

    ce = L.CrossEntropyLoss()

    def ce_fwd():
        out["ce"] = ce(xs[0], y)
    names = count_launches(ce_fwd)
    print("CrossEntropyLoss forward:", names)
    assert len(names) == 1, names

    def ce_bwd():
        xs[0].grad = None
        out["ce"].backward(unit, retain_graph=True)
    names = count_launches(ce_bwd)
    print("CrossEntropyLoss backward:", names)
    assert len(names) == 1, names

    tm, em = M.TrainMetrics(), M.EvalMetrics()
    det = [x.detach() for x in xs]
    names = count_launches(lambda: tm.update(*out["losses"], *det, y))
    print("TrainMetrics.update:", names)
    assert len(names) == 1, names
    names = count_launches(lambda: em.update(det[0], y))
    print("EvalMetrics.update:", names)
    assert len(names) == 1, names
    names = count_launches(em.compute)
    print("EvalMetrics.compute:", names)
    assert 1 <= len(names) <= 3, names

    # the whole tail: the stock sequence (three criterion calls, two .item() reads, the sum, backward) against ours
    def stock_tail():
        for x in xs:
            x.grad = None
        ce_loss = stock(xs[0], y)
        ad_loss = (stock(xs[1], ones) + stock(xs[2], zeros)) / 2
        ce_loss.item()
        ad_loss.item()
        loss = ad_loss + ce_loss
        loss.backward()

    def our_tail():
        for x in xs:
            x.grad = None
        ce_loss, ad_loss = crit(*xs, y)
        tm.update(ce_loss, ad_loss, *det, y)
        all_loss = ad_loss + ce_loss
        all_loss.backward()
    n_stock, n_ours = count_launches(stock_tail), count_launches(our_tail)
    print(f"tail of a step: stock {len(n_stock)} kernels, ours {len(n_ours)} kernels: {n_ours}")
    assert len(n_ours) < len(n_stock)


def test_updates_do_not_synchronise():
    """A long queue of work, an event behind it, then the updates: when they return, the event has not completed — the host
    did not wait for the device.  (The queue is ~0.1 s of matrix products; an update returns in well under a millisecond.)"""
    L, M = _L(), _M()
    logits, d_mri, d_pet, label, _ = CI.adv_inputs(8, 2)
    xs = [dev(a, grad=True) for a in (logits, d_mri, d_pet)]
    y = dev(label)
    crit, tm, em = L.AdversarialCriterion(), M.TrainMetrics(), M.EvalMetrics()
    det = [x.detach() for x in xs]
    a = torch.randn(4096, 4096, device=DEV)
    for _ in range(2):                           # warm-up: modules loaded, buffers allocated
        ce_loss, ad_loss = crit(*xs, y)
        tm.update(ce_loss, ad_loss, *det, y)
        em.update(det[0], y)
        (ad_loss + ce_loss).backward()
        a @ a
    torch.cuda.synchronize()
    for _ in range(100):
        a = (a @ a) * 1e-4
    ev = torch.cuda.Event()
    ev.record()
    ce_loss, ad_loss = crit(*xs, y)
    tm.update(ce_loss, ad_loss, *det, y)
    em.update(det[0], y)
    (ad_loss + ce_loss).backward()
    still_running = not ev.query()
    torch.cuda.synchronize()
    assert still_running
    assert tm.compute()["accuracy"] >= 0.0


# ---------------------------------------------------------------------------------------------------------------------
# NaN logits, batches above the kernel's
# ---------------------------------------------------------------------------------------------------------------------

def test_nan_logits_are_predicted_as_torch_argmax_does():
    """torch.argmax takes a NaN for the maximum (the first one of a row); the kernels' accuracy and confusion counts do the
    same, so a diverged model reads alike on the kernels and on the torch-ops path."""
    M = _M()
    nan = float("nan")
    logits = np.array([[nan, 1.0, 2.0], [0.0, nan, 5.0], [3.0, 0.0, nan], [nan, nan, 9.0], [1.0, nan, nan],
                       [0.5, 2.0, 1.0], [2.0, 2.0, 0.0]], dtype=np.float32)
    label = np.array([0, 1, 2, 1, 1, 1, 0], dtype=np.int64)
    pred = torch.from_numpy(logits).argmax(1).numpy()
    assert pred.tolist() == [0, 1, 2, 0, 1, 1, 0]
    assert torch.equal(dev(logits).argmax(1).cpu(), torch.from_numpy(pred))
    cm = np.zeros((3, 3), dtype=np.int64)
    np.add.at(cm, (label, pred), 1)
    em, host = M.EvalMetrics(num_classes=3), M.EvalMetrics(num_classes=3)
    x, y = dev(logits), dev(label)
    assert M._logits_on_kernel(x, y)
    em.update(x, y)
    host.update(torch.from_numpy(logits), torch.from_numpy(label))
    got, want = em.compute(), host.compute()
    assert np.array_equal(got["confusion"].numpy(), cm) and torch.equal(got["confusion"], want["confusion"])
    assert got["accuracy"] == want["accuracy"] == 6 / 7
    assert math.isnan(got["loss"]) and math.isnan(want["loss"])
    # the three heads of TrainMetrics: label head as above (two classes here), MRI target 1, PET target 0
    two = np.array([[nan, 1.0], [0.0, nan], [nan, nan], [1.0, 0.0]], dtype=np.float32)
    lab2 = np.array([0, 1, 1, 1], dtype=np.int64)
    tm, th = M.TrainMetrics(), M.TrainMetrics()
    tm.update(dev(np.float32(1.0)), dev(np.float32(2.0)), dev(two), dev(two), dev(two), dev(lab2))
    th.update(1.0, 2.0, *[torch.from_numpy(two)] * 3, torch.from_numpy(lab2))
    assert tm.compute() == th.compute() == {"accuracy": 0.5, "MRI_accuracy": 0.25, "PET_accuracy": 0.75,
                                            "ce_loss": 1.0, "ad_loss": 2.0}


def test_eval_update_above_the_kernel_batch_is_fed_in_chunks():
    """One update of 9001 samples: three launches of the kernel (4096 + 4096 + 809), nothing else, and the state, scores and
    labels of the same epoch fed in batches of at most 4096."""
    M = _M()
    n = 9001
    logits, label = CI.epoch_inputs(n)
    x, y = dev(logits), dev(label)
    whole, parts = M.EvalMetrics(), M.EvalMetrics()
    whole.update(x, y)                           # allocates the epoch buffers
    whole.reset()
    names = count_launches(lambda: (whole.reset(), whole.update(x, y)))
    names = [k for k in names if "fill" not in k.lower()]         # reset()'s zero_()
    print("EvalMetrics.update of 9001 samples:", names)
    assert len(names) == 3 and len(set(names)) == 1, names
    feed(parts, logits, label, cuts_for(n))
    assert torch.equal(whole.scores, parts.scores) and torch.equal(whole.labels, parts.labels)
    a, b = whole.compute(), parts.compute()
    assert torch.equal(a["confusion"], b["confusion"]) and a["auc"] == b["auc"]
    assert abs(a["loss"] - b["loss"]) <= n * 2.0 ** -52 * b["loss"]


# ---------------------------------------------------------------------------------------------------------------------
# 10: a step
# ---------------------------------------------------------------------------------------------------------------------

def test_three_train_steps_of_model_cnn_ad():
    """model_CNN_ad at the cnn_mid fixture's shape (dim 128, 48 x 40 x 48, batch 2), three Adam steps (lr 1e-4) from equal
    initial state: (A) the stock tail, (B) the stock tail with its cross entropies in fp64, (C) AdversarialCriterion.

    What is asserted, at every one of the three steps: the two losses C returns and the three logit gradients it hands to
    the network's backward are within the bounds of item 6 (module docstring) of the fp64 formula on the logits C's own
    network produced at that step.  Everything after the tail — the network's backward, Adam — is the same code in A and C,
    so this is the whole of what the criterion contributes to a step, stated where a derived bound exists.  The first
    step's forward is also bit-identical in A and C (equal state, equal code ahead of the tail).

    What is only printed: the distances between the parameter vectors, max |A - B|, max |C - A|, max |C - B| after each
    step.  Carried through Adam, the gradient bounds give no usable limit on them.  Adam's first update of a parameter with
    gradient g is lr g / (|g| + eps), eps = 1e-8, so a gradient perturbation dg moves it by up to lr min(2, |dg| / eps); the
    bound of item 6 on a logit gradient is u (4 C + 8) / B = 4.8e-7 here, far above eps, and the network has parameters whose
    own gradient is at that size or below (a convolution bias ahead of a train-mode BatchNorm has a gradient of exactly zero
    in real arithmetic, fp32 leaves rounding noise there).  For those a last-bit difference in the tail flips the update
    from -lr to +lr, and the maximum over all parameters is 2 lr per step whatever the criterion does: a limit every pair of
    finite runs meets, so asserting it would check nothing."""
    L = _L()
    import transmf_ad_amd as T
    LR = 1e-4
    torch.manual_seed(11)
    net0 = T.model_CNN_ad(dim=128).to(DEV)
    rs = np.random.RandomState(23)
    mri = dev(rs.rand(2, 1, 48, 40, 48).astype(np.float32))
    pet = dev(rs.rand(2, 1, 48, 40, 48).astype(np.float32))
    label_np = np.array([0, 1], dtype=np.int64)
    label = dev(label_np)
    ones, zeros = torch.ones_like(label), torch.zeros_like(label)
    stock, ours = torch.nn.CrossEntropyLoss(), L.AdversarialCriterion()

    def tail_a(lo, dm, dp):
        return stock(lo, label), (stock(dm, ones) + stock(dp, zeros)) / 2

    def tail_b(lo, dm, dp):
        return stock(lo.double(), label), (stock(dm.double(), ones) + stock(dp.double(), zeros)) / 2

    def tail_c(lo, dm, dp):
        assert L.adversarial_kernel_ok(lo, dm, dp, label)
        return ours(lo, dm, dp, label)

    def run(tail):
        net = copy.deepcopy(net0).train()
        opt = T.optim.Adam(net.parameters(), lr=LR)
        torch.manual_seed(29)
        states, seen = [], []
        for it in range(3):
            opt.zero_grad()
            outs = net(mri, pet)
            rec = {}                             # this step's logits, losses and the gradients the tail hands back
            for k, o in zip(("lo", "dm", "dp"), outs):
                rec[k] = o.detach().cpu().numpy()
                o.register_hook(lambda g, k=k, rec=rec: rec.__setitem__("g_" + k, g.detach().cpu().numpy()))
            ce_loss, ad_loss = tail(*outs)
            all_loss = ad_loss + ce_loss
            all_loss.backward()
            opt.step()
            rec["ce"], rec["ad"] = ce_loss.item(), ad_loss.item()
            seen.append(rec)
            states.append(torch.cat([p.detach().reshape(-1) for p in net.parameters()]).double().cpu())
        return states, seen
    (a, sa), (a2, _), (b, _), (c, sc) = run(tail_a), run(tail_a), run(tail_b), run(tail_c)
    for t in range(3):
        assert torch.equal(a[t], a2[t]), "the model does not repeat: the distances below would measure that instead"
    for k in ("lo", "dm", "dp"):                 # step 1: equal state, the same forward
        assert np.array_equal(sa[0][k], sc[0][k])
    heads = (("lo", label_np, 1.0), ("dm", np.ones(2, dtype=np.int64), 0.5), ("dp", np.zeros(2, dtype=np.int64), 0.5))
    for t, rec in enumerate(sc):
        l64 = {k: CI.ce64(rec[k], tgt)[0] for k, tgt, _ in heads}
        ce_b = loss_bound(rec["lo"], label_np, None, "mean", l64["lo"])
        ad64 = (l64["dm"] + l64["dp"]) / 2
        ad_b = sum(loss_bound(rec[k], tgt, None, "mean", l64[k]) for k, tgt, _ in heads[1:]) / 2
        ce_e, ad_e = abs(rec["ce"] - l64["lo"]), abs(rec["ad"] - ad64)
        print(f"step {t + 1}: ce_loss {rec['ce']!r} error / bound {ce_e / ce_b:.3f}, ad_loss {rec['ad']!r} error / bound "
              f"{ad_e / ad_b:.3f}")
        assert ce_e <= ce_b and ad_e <= ad_b
        for k, tgt, half in heads:
            g64 = CI.ce64(rec[k], tgt)[1] * half
            err = np.abs(rec["g_" + k].astype(np.float64) - g64)
            bound = grad_bound(rec[k], tgt, None, "mean", half=half)
            print(f"step {t + 1}, {k}: logit gradient error / bound {(err / bound).max():.3f}")
            assert np.all(err <= bound)
        assert torch.isfinite(c[t]).all()
        print(f"step {t + 1}: max |A - B| = {(a[t] - b[t]).abs().max().item():.3e} (stock fp32 against its fp64 tail), "
              f"max |C - A| = {(c[t] - a[t]).abs().max().item():.3e}, max |C - B| = {(c[t] - b[t]).abs().max().item():.3e}")
