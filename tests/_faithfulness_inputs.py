"""Cases and CPU references of the deletion / insertion curve tests (tests/test_host_faithfulness.py,
tests/test_gpu_faithfulness.py): the kernels of csrc/faithfulness.hip and transmf_ad_amd.faithfulness_curve.

  Ordering.  a = attr + 0.0 (-0.0 ranks with +0.0), compared as floats; ties go together.
  Thresholds.  thr[b, k] = the counts[k]-th largest a of row b; removed[b, k] = #{v: a[b, v] >= thr[b, k]}.
  Jobs.  Job j = b*(S+1) + s: m = (s > 0) & (a[b] >= thr[b, s-1]); deletion: where(m, f, vol[b]), insertion: where(m, vol[b], f),
    f = base[b] or fill[b].

Both kernels are exact: thr is compared as bits, removed and the masks with torch.equal - against a float32 torch.sort
(thresholds_ref) and torch.where (mask_ref).  Nothing here touches a GPU or reads a file."""
import math

import torch

F32 = torch.float32
MAX_STEPS = 64

# (B, V) of the threshold cases: one voxel; odd and short (one element per lane, % 4 == 1); one workgroup pass of the 16-byte
# path; several workgroups per row; 33 x 35 x 38 = 43890 (% 4 == 2: the scalar path over more than one workgroup).
RANK_SHAPES = [(1, 1), (2, 105), (2, 4096), (3, 32768), (2, 43890)]
RANK_STEPS = (1, 8, 64)
REPEATING = ((2, 5), 64)        # V < steps: counts repeat
VALUE_SETS = ("permutation", "equal", "two", "signed_zeros", "denormals", "infinities", "low10", "one_bin", "quantised")


def counts_ref(V, steps):
    """n_k = ceil(k*V / steps) by exact integer arithmetic, k = 1..steps."""
    return [(k * V + steps - 1) // steps for k in range(1, steps + 1)]


def _from_bits(bits):
    return bits.to(torch.int32).view(F32)


def values(kind, B, V, seed=0):
    """(B, V) float32 of one value set.
    permutation   distinct integers in random order: removed == counts
    equal         one value: every threshold is it, removed == V
    two           two values
    signed_zeros  mixed signs with +0.0 and -0.0 among them (they rank together, thr is +0.0 there)
    denormals     +- denormals and a few normal values
    infinities    +inf and -inf among finite values
    low10         values that differ in the lowest 10 mantissa bits only: the last digit decides
    one_bin       one first-pass bin (the top 11 bits shared): half share the top 22 bits too, half differ in the lowest 21
    quantised     floor(x*16)/16 of smooth bumps plus noise: long runs of ties"""
    g = torch.Generator().manual_seed(1009 * B + V + 7919 * seed + 31 * VALUE_SETS.index(kind))
    if kind == "permutation":
        return torch.stack([torch.randperm(V, generator=g) for _ in range(B)]).to(F32) - float(V // 2)
    if kind == "equal":
        return torch.full((B, V), 0.37, dtype=F32)
    if kind == "two":
        return torch.where(torch.rand((B, V), generator=g) < 0.3, torch.tensor(2.25), torch.tensor(-1.5))
    x = torch.randn((B, V), generator=g)
    pick = torch.randint(0, 7, (B, V), generator=g)
    if kind == "signed_zeros":
        x[pick == 0] = 0.0
        x[pick == 1] = -0.0
        return x
    if kind == "denormals":
        bits = torch.randint(0, 1 << 23, (B, V), generator=g) | (torch.randint(0, 2, (B, V), generator=g) << 31)
        bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits)
        return torch.where(pick == 0, x * 1e-30, _from_bits(bits))
    if kind == "infinities":
        x[pick == 0] = float("inf")
        x[pick == 1] = float("-inf")
        return x
    if kind == "low10":
        return _from_bits(0x3F800000 | torch.randint(0, 1 << 10, (B, V), generator=g))
    if kind == "one_bin":
        low = torch.where(pick < 4, torch.randint(0, 1 << 10, (B, V), generator=g), torch.randint(0, 1 << 21, (B, V), generator=g))
        return _from_bits(0x3F800000 | low)
    if kind == "quantised":
        t = torch.linspace(0, 1, V).view(1, V)
        c = torch.rand((B, 3, 1), generator=g)
        bumps = torch.exp(-((t.view(1, 1, V) - c) / 0.07) ** 2).sum(1)
        return torch.floor((bumps + 0.02 * x) * 16) / 16
    raise KeyError(kind)


def thresholds_ref(attr, counts):
    """float32 torch.sort: -> (thr (B, S) float32, removed (B, S) int32)."""
    a = attr.reshape(attr.shape[0], -1) + 0.0
    srt = a.sort(1, descending=True).values
    thr = srt[:, torch.tensor(counts) - 1]
    removed = torch.stack([(a >= thr[:, k:k + 1]).sum(1) for k in range(len(counts))], 1).to(torch.int32)
    return thr, removed


def thresholds_brute(row, counts):
    """One row in plain Python: sorted() and a count."""
    a = [float(x) + 0.0 for x in row]
    srt = sorted(a, reverse=True)
    thr = [srt[n - 1] for n in counts]
    return thr, [sum(1 for x in a if x >= t) for t in thr]


def bits(t):
    return t.contiguous().view(torch.int32)


# (B, V, S) of the mask cases: V % 4 == 1; the 16-byte path; 43890 voxels (% 4 == 2) over several workgroups
MASK_CASES = [(2, 105, 3), (2, 4096, 8), (2, 43890, 5)]
MODES = ("deletion", "insertion")


def chunkings(B, S):
    """(j0, K): K = 1 at s = 0 and at s = S; a chunk that starts mid-sample and crosses into the next sample (B == 1: to the
    end); the short last chunk of a walk in chunks of 5; all jobs."""
    n, total = S + 1, B * (S + 1)
    mid = n // 2
    cross = (mid, n) if B > 1 else (mid, n - mid)
    last = (total - 1) // 5 * 5
    return [(0, 1), (S, 1), cross, (last, total - last), (0, total)]


def mask_inputs(B, V, S):
    """-> vol (B, V), attr (B, V) quantised (thresholds with ties), thr (B, S), fill (B,) values no voxel holds, base (B, V)."""
    g = torch.Generator().manual_seed(17 + B + 3 * V + S)
    vol = torch.rand((B, V), generator=g)
    attr = values("quantised", B, V, seed=5)
    attr[:, ::11] = -0.0
    thr, _removed = thresholds_ref(attr, counts_ref(V, S))
    fill = -1.0 - torch.rand((B,), generator=g)
    base = 2.0 + torch.rand((B, V), generator=g)
    return vol, attr, thr, fill, base


def mask_ref(vol, attr, thr, fill, mode, j0, K, base=None):
    """torch.where, job by job."""
    S = thr.shape[1]
    a = attr + 0.0
    out = []
    for j in range(j0, j0 + K):
        b, s = divmod(j, S + 1)
        m = a[b] >= thr[b, s - 1] if s else torch.zeros_like(a[b], dtype=torch.bool)
        f = base[b] if base is not None else fill[b]
        out.append(torch.where(m, f, vol[b]) if mode == "deletion" else torch.where(m, vol[b], f))
    return torch.stack(out)


def curve_loop(net, vols, volume, attr, steps, mode, fills, base, target, chunk, score):
    """The user's loop on whatever device the tensors live on: torch.sort, torch.where, the model's own forward in chunks ->
    (scores (B, S+1), removed (B, S+1), thresholds (B, S), the logits of every job (B, S+1, classes), the base logits)."""
    B = vols[0].shape[0]
    v = vols[volume]
    a = attr.reshape(B, -1) + 0.0
    V = a.shape[1]
    counts = counts_ref(V, steps)
    srt = a.sort(1, descending=True).values
    thr = srt[:, torch.tensor(counts, device=a.device) - 1]
    removed = torch.stack([torch.zeros(B, dtype=torch.long, device=a.device)]
                          + [(a >= thr[:, k:k + 1]).sum(1) for k in range(steps)], 1).to(torch.int32)
    n = steps + 1
    first = lambda o: o[0] if isinstance(o, tuple) else o
    with torch.no_grad():
        logits = first(net(*vols))
        outs = []
        for j0 in range(0, B * n, chunk):
            jobs = range(j0, min(j0 + chunk, B * n))
            rows = torch.tensor([j // n for j in jobs], device=v.device)
            batch = [x.index_select(0, rows).clone() for x in vols]
            for k, j in enumerate(jobs):
                b, s = divmod(j, n)
                m = (a[b] >= thr[b, s - 1] if s else torch.zeros_like(a[b], dtype=torch.bool)).view(v.shape[1:])
                f = base[b] if base is not None else fills[b]
                batch[volume][k] = torch.where(m, f, v[b]) if mode == "deletion" else torch.where(m, v[b], f)
            outs.append(first(net(*batch)))
        jobs = torch.cat(outs)
    rows = torch.arange(B * n, device=v.device) // n
    s = jobs if score == "logit" else torch.softmax(jobs, 1)
    scores = s.gather(1, target.index_select(0, rows).view(-1, 1))[:, 0].view(B, n)
    return scores, removed, thr, jobs.view(B, n, -1), logits


def auc_ref(scores):
    """(s_0/2 + s_1 + .. + s_{S-1} + s_S/2) / S in float64 from Python numbers."""
    out = []
    for row in scores.tolist():
        S = len(row) - 1
        out.append((row[0] / 2 + math.fsum(row[1:S]) + row[S] / 2) / S)
    return torch.tensor(out, dtype=torch.float64)
