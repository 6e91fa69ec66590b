"""CPU-only checks of the region Shapley values (transmf_ad_amd/region_shap.py, the torch twins of ops.py, the host entry of
csrc/shap.hip): the binding, the size table, the coalition sampler against the host Philox model of tests/_shap_inputs.py, the
exactness of the fit (additive games, efficiency, the closed form against the KKT system, a 6-player game against brute force),
the singular case, and region_shap_torch on a toy model whose shares are known."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import _shap_inputs as si

F32, F64, I32 = torch.float32, torch.float64, torch.int32


def test_symbols_and_exports():
    import transmf_ad_amd
    from transmf_ad_amd import _lib, ops
    from transmf_ad_amd.build import FILE_FLAGS, SOURCES
    C, P = ctypes, _lib.PROTOTYPES
    assert P["tmf_shap_size_table"] == (C.c_int, [C.c_int, C.c_void_p])
    assert P["tmf_shap_coalitions"] == (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_ulonglong, C.c_int, C.c_int, C.c_void_p])
    assert P["tmf_shap_apply"] == (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 10 + [C.c_void_p])
    assert P["tmf_shap_gram"] == (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p])
    assert P["tmf_shap_solve_workspace"] == (C.c_size_t, [C.c_int] * 2)
    assert P["tmf_shap_solve"] == (C.c_int, [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 3 + [C.c_size_t, C.c_int, C.c_int, C.c_void_p])
    assert _lib.SHAP_MAX_PLAYERS == _lib.REGION_MAX == ops.SHAP_MAX_PLAYERS == 1024
    assert "shap.hip" in SOURCES and FILE_FLAGS["shap.hip"] == ["-ffp-contract=off"]
    for name in ("region_shap", "region_shap_torch", "RegionShap"):
        assert name in transmf_ad_amd.__all__ and callable(getattr(transmf_ad_amd, name))
    for name in ("shap_size_table", "shap_coalitions", "shap_coalitions_torch", "shap_apply", "shap_apply_torch", "shap_gram",
                 "shap_gram_torch", "shap_solve", "shap_solve_torch", "shap_ok"):
        assert callable(getattr(ops, name)), name


@pytest.mark.parametrize("P", si.TABLE_PLAYERS)
def test_size_table_equals_the_restatement(P):
    """tmf_shap_size_table (the host entry), ops.shap_size_table_torch and the model agree word for word; the table ascends and
    is symmetric in probability: size s and size P - s are as likely."""
    from transmf_ad_amd import _lib, ops
    want = si.size_table(P)
    got = ops.shap_size_table(P)
    assert got.dtype == torch.int64 and tuple(got.shape) == (max(P - 2, 0),)
    assert np.array_equal(got.numpy().astype(np.uint64), want)
    assert np.array_equal(ops.shap_size_table_torch(P).numpy().astype(np.uint64), want)
    assert bool((np.diff(want.astype(np.int64)) >= 0).all())
    if P > 2:
        edges = np.concatenate([[0], want.astype(np.float64), [2.0 ** 32]])
        prob = np.diff(edges) / 2.0 ** 32
        assert np.allclose(prob, prob[::-1], atol=2.0 ** -30)
    lib = _lib.load()
    assert lib.tmf_shap_size_table(1, None) == lib.tmf_shap_size_table(1025, None) == _lib.E_SHAPE
    assert lib.tmf_shap_size_table(3, None) == _lib.E_NULL and lib.tmf_shap_size_table(2, None) == 0


@pytest.mark.parametrize("P", si.PLAYERS)
def test_coalitions_are_a_function_of_seed_and_row(P):
    """shap_coalitions_torch equals the host Philox model bit for bit, paired or not; sizes in 1..P-1; odd rows of a pair are
    complements; the padding bits are zero; a row does not change with m0 or N; another seed: other rows."""
    from transmf_ad_amd import ops
    N = 66 if P < 1024 else 6
    for paired in (True, False):
        coal = ops.shap_coalitions_torch(P, paired, si.SEEDS[0], 0, N)
        assert coal.dtype == I32 and tuple(coal.shape) == (N, si.words_of(P))
        assert torch.equal(coal, si.coalitions(P, paired, si.SEEDS[0], 0, N)), paired
        z, pad = si.unpack(coal, P)
        sizes = z.sum(1)
        assert sizes.min() >= 1 and sizes.max() <= P - 1 and not pad.any()
        if paired:
            assert np.array_equal(z[1::2], ~z[0::2])
        late = ops.shap_coalitions_torch(P, paired, si.SEEDS[0], 3, N - 3)                 # an odd m0: a pair is cut in two
        assert torch.equal(late, coal[3:])
        assert torch.equal(ops.shap_coalitions_torch(P, paired, si.SEEDS[0], 0, 3), coal[:3])
        if P > 3:
            assert not torch.equal(ops.shap_coalitions_torch(P, paired, si.SEEDS[1], 0, N), coal)
    assert torch.equal(ops.shap_unpack(coal, P), torch.from_numpy(z))


def test_coalition_sizes_follow_the_shapley_kernel():
    """P = 10, 4000 unpaired rows: the share of every size within 4 sigma of w_s / sum w; every player in about half the rows."""
    from transmf_ad_amd import ops
    P, N = 10, 4000
    z, _pad = si.unpack(ops.shap_coalitions_torch(P, False, 9, 0, N), P)
    w = np.array([1.0 / (s * (P - s)) for s in range(1, P)])
    w /= w.sum()
    share = np.bincount(z.sum(1), minlength=P)[1:] / N
    assert bool((np.abs(share - w) < 4 * np.sqrt(w * (1 - w) / N)).all())
    assert bool((np.abs(z.mean(0) - 0.5) < 4 * 0.5 / np.sqrt(N)).all())
    for kw in (dict(P=1), dict(P=1025), dict(seed=-1), dict(seed=1 << 64), dict(N=0), dict(m0=-1), dict(m0=2 ** 31 - 2, N=4)):
        args = dict(P=5, paired=True, seed=1, m0=0, N=4)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.shap_coalitions_torch(**args)


def _dyadic_game(P, B, N, seed):
    """An additive game whose sums are exact in float32 and float64: a (B, P) multiples of 1/8, scores = offset + Z a."""
    g = np.random.default_rng(seed)
    a = g.integers(-32, 33, (B, P)) / 8.0
    offset = g.integers(-16, 17, (B,)) / 4.0
    z = si.coalition_bits(P, True, si.SEEDS[1], 0, N)
    scores = offset[:, None] + a @ z.T.astype(np.float64)
    return a, z, torch.from_numpy(scores.astype(np.float32)), torch.from_numpy(offset.astype(np.float32))


@pytest.mark.parametrize("P", (2, 3, 33, 116))
def test_additive_game_is_recovered_and_efficiency_holds(P):
    """Exact inputs, so only the solve's rounding is left: phi = a within the header's solve bound; sum(phi) - delta within
    4 P 2^-53 sum|phi| (P roundings of the phi_i of at most 2^-53 |phi_i| each, the rounding of t = (sum x_b - delta) / sum x_1
    times sum|x_1 t| <= sum|phi| + sum|x_b|, and the test's own summation; 4 P covers them); the closed form equals the KKT
    system within the same bound; A equals the integer reference."""
    from transmf_ad_amd import ops
    B, N = 3, 4 * P + 64
    a, z, scores, offset = _dyadic_game(P, B, N, 3 + P)
    coal = si.pack(z)
    A, rhs = ops.shap_gram_torch(coal, scores, offset, P)
    wantA, want_rhs, _tol = si.gram_reference(z, scores, offset)
    assert A.dtype == I32 and np.array_equal(A.numpy(), wantA) and np.array_equal(rhs.numpy(), want_rhs)        # exact sums
    delta = torch.from_numpy(a.sum(1))
    phi, info = ops.shap_solve_torch(A, rhs, delta)
    assert int(info) == 0 and phi.dtype == F64 and tuple(phi.shape) == (B, P)
    bound, cond = si.solve_bound(wantA, 0.0, a)
    err = np.abs(phi.numpy() - a).max(1)
    print(f"P = {P}: cond {cond:.3g}, additive err / bound {(err / bound).max():.3g}")
    assert bool((err <= bound).all())
    gap = np.abs(np.array([float(np.sum(p.astype(np.longdouble))) for p in phi.numpy()]) - delta.numpy())
    assert bool((gap <= 4 * P * si.U * np.abs(phi.numpy()).sum(1)).all()), gap
    ref = si.kkt(wantA, want_rhs, delta.numpy())
    assert bool((np.abs(phi.numpy() - ref).max(1) <= si.solve_bound(wantA, 0.0, ref)[0]).all())


@pytest.mark.parametrize("B", (1, 3))
def test_closed_form_equals_the_kkt_system_on_a_noisy_game(B):
    from transmf_ad_amd import ops
    for P in (33, 116):
        A, rhs, delta = si.fit_case(P, B)
        phi, info = ops.shap_solve_torch(A, rhs, delta)
        ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy())
        bound, cond = si.solve_bound(A.numpy(), 0.0, ref)
        err = np.abs(phi.numpy() - ref).max(1)
        print(f"P = {P}, B = {B}: cond {cond:.3g}, err / bound {(err / bound).max():.3g}")
        assert int(info) == 0 and bool((err <= bound).all())
        r = ops.shap_solve_torch(A, rhs, delta, ridge=0.25)[0]
        ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy(), 0.25)
        assert bool((np.abs(r.numpy() - ref).max(1) <= si.solve_bound(A.numpy(), 0.25, ref)[0]).all())


def test_six_player_game_equals_brute_force_on_the_full_fit():
    """Every proper subset of 6 players, repeated in proportion to its Shapley-kernel weight w_s / C(6, s) = 12 : 3 : 2 : 3 : 12
    (times 1 / 360): the unweighted constrained fit is then the Shapley value itself.  A random game under a fixed seed against
    the subset formula.  Tolerance: the solve bound plus the propagated rounding of the right-hand sides, N 2^-53 sum|y| * sqrt(P)
    / lambda_min(M)."""
    from transmf_ad_amd import ops
    P, reps = 6, {1: 12, 2: 3, 3: 2, 4: 3, 5: 12}
    g = np.random.default_rng(2024)
    table = {s: float(g.standard_normal()) for s in itertools.product((0, 1), repeat=P)}
    rows = [s for s in table if 0 < sum(s) < P for _ in range(reps[sum(s)])]
    z = np.asarray(rows, dtype=bool)
    assert z.shape == (274, P)
    scores = torch.tensor([[table[s] for s in rows]], dtype=F64)
    offset = torch.tensor([table[(0,) * P]], dtype=F64)
    delta = torch.tensor([table[(1,) * P] - table[(0,) * P]], dtype=F64)
    A, rhs = ops.shap_gram_torch(si.pack(z), scores, offset, P)
    phi, info = ops.shap_solve_torch(A, rhs, delta)
    want = si.brute_force_shapley(lambda s: table[s], P)
    bound, _cond = si.solve_bound(A.numpy(), 0.0, want[None])
    lam = np.linalg.eigvalsh(A.numpy().astype(np.float64))[0]
    tol = bound[0] + len(rows) * si.U * float((scores - offset).abs().sum()) * P ** 0.5 / lam
    err = np.abs(phi.numpy()[0] - want).max()
    print(f"6 players: err {err:.3g}, tolerance {tol:.3g}")
    assert int(info) == 0 and err <= tol and abs(float(phi.sum()) - float(delta)) <= 4 * P * si.U * np.abs(want).sum()


def test_singular_gram_matrix_sets_info_and_ridge_solves_it():
    """Two paired coalitions for five players: A = z z^T + (1 - z)(1 - z)^T has rank 2 and 0 / 1 entries, so the factorisation is
    exact and meets a pivot of exactly 0: info > 0 and every phi NaN.  With a ridge the system is definite again."""
    from transmf_ad_amd import ops
    P, B = 5, 2
    coal = ops.shap_coalitions_torch(P, True, 3, 0, 2)
    scores, offset = si.scores_for(B, 2)
    A, rhs = ops.shap_gram_torch(coal, scores, offset, P)
    assert np.linalg.matrix_rank(A.numpy()) == 2
    delta = torch.tensor([0.5, -1.0], dtype=F64)
    phi, info = ops.shap_solve_torch(A, rhs, delta)
    assert 1 <= int(info) <= 3 and bool(phi.isnan().all())
    phi, info = ops.shap_solve_torch(A, rhs, delta, ridge=0.5)
    ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy(), 0.5)
    assert int(info) == 0 and bool((np.abs(phi.numpy() - ref).max(1) <= si.solve_bound(A.numpy(), 0.5, ref)[0]).all())
    for bad in (-1.0, float("nan"), float("inf"), "0"):
        with pytest.raises(ValueError):
            ops.shap_solve_torch(A, rhs, delta, ridge=bad)


def test_apply_twin_is_a_select():
    """Jobs and chunks of shap_apply_torch against an explicit loop over the voxels' players; the all-ones row is the volume,
    the zero row replaces every labelled voxel and no background; out= is written in place."""
    from transmf_ad_amd import ops
    size, R, p0, P = (4, 5, 6), 7, 7, 14
    vol, fill, base = si.volumes(size)
    lab = si.labels_for(size, R)
    z = si.coalition_bits(P, True, 5, 0, 4)
    z = np.concatenate([z, np.ones((1, P), bool), np.zeros((1, P), bool)])
    coal, N, B = si.pack(z), 6, vol.shape[0]
    got = ops.shap_apply_torch(vol, lab, coal, fill, R, p0, P, 0, B * N)
    has = (lab >= 1) & (lab <= R)
    for j in range(B * N):
        b, m = divmod(j, N)
        member = torch.from_numpy(z[m])[(p0 + lab.long() - 1).clamp(0, P - 1)]
        assert torch.equal(got[j, 0], torch.where(~has | member, vol[b, 0], fill[b])), j
    assert torch.equal(got[4], vol[0]) and torch.equal(got[5, 0][has], fill[0].expand(int(has.sum())))
    assert torch.equal(got[5, 0][~has], vol[0, 0][~has])
    buf = torch.zeros((3, 1) + size)
    out = ops.shap_apply_torch(vol, lab, coal, None, R, p0, P, N - 1, 3, base=base, out=buf)
    gone = has & ~torch.from_numpy(z[0])[(p0 + lab.long() - 1).clamp(0, P - 1)]         # job N of the chunk: sample 1, row 0
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out[1, 0][gone], base[1, 0][gone])
    assert torch.equal(out[1, 0][~gone], vol[1, 0][~gone]) and torch.equal(out[0], vol[0] * 0 + torch.where(has, fill[0] * 0 + base[0], vol[0]))
    for kw in (dict(R=0), dict(p0=8), dict(p0=-1), dict(j0=B * N), dict(K=0), dict(P=1)):
        args = dict(R=R, p0=p0, P=P, j0=0, K=1)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.shap_apply_torch(vol, lab, coal, fill, **args)


class RegionMeans(nn.Module):
    """logit 0 = sum_r w0[r] mean_r(mri) + sum_r w1[r] mean_r(pet), logit 1 = its negative: with score="logit", target=0 and
    fill 0 the game is additive and the share of region r of volume q is wq[r] * mean_r."""

    def __init__(self, atlas, R):
        super().__init__()
        onehot = torch.stack([(atlas == r + 1).reshape(-1) for r in range(R)]).double()
        self.register_buffer("pool", onehot / onehot.sum(1, keepdim=True))
        g = torch.Generator().manual_seed(1)
        self.w0 = nn.Parameter(torch.randn(R, generator=g, dtype=F64))
        self.w1 = nn.Parameter(torch.randn(R, generator=g, dtype=F64))
        self.bn = nn.BatchNorm1d(2).double()             # identity in eval mode at its initial statistics, up to eps

    def means(self, x):
        return x.reshape(x.shape[0], -1).double() @ self.pool.t()

    def forward(self, mri, pet):
        s = (self.means(mri) * self.w0).sum(1) + (self.means(pet) * self.w1).sum(1)
        return torch.stack([s, -s], 1)


def _toy():
    size, R = (6, 6, 6), 8
    atlas = si.block_atlas(size, 2)
    atlas[0, 0, :3] = 0                                   # some background
    g = torch.Generator().manual_seed(4)
    mri, pet = (torch.rand((2, 1) + size, generator=g, dtype=F64) + 0.5 for _ in range(2))
    return RegionMeans(atlas, R).eval(), mri, pet, atlas, R


def test_region_shap_torch_returns_the_known_shares():
    """The additive toy model: values = w * region mean (y is exact to a few ulp, the fit amplifies that by at most cond_2(M) <
    1e4: held at 1e-9 of the largest share), sum(values) = delta, r2 = 1, ok(); volume() puts the shares on the voxels; top and
    table agree with values; the caller's tensors, the parameters' grads, the buffers, the train flag and torch's generator are
    untouched."""
    import transmf_ad_amd as T
    net, mri, pet, atlas, R = _toy()
    keep = {k: v.clone() for k, v in net.state_dict().items()}
    vols = (mri.clone(), pet.clone())
    rng = torch.get_rng_state()
    sh = T.region_shap_torch(net, mri, pet, atlas=atlas, samples=128, seed=5, score="logit", target=0, chunk=7)
    assert torch.equal(torch.get_rng_state(), rng) and torch.equal(mri, vols[0]) and torch.equal(pet, vols[1])
    assert all(torch.equal(v, keep[k]) for k, v in net.state_dict().items()) and all(p.grad is None for p in net.parameters())
    assert not net.training and isinstance(sh, T.RegionShap)
    assert sh.R == R and sh.players == 2 * R and sh.volumes == (0, 1) and sh.joint and sh.samples == 128 and sh.seed == 5
    assert tuple(sh.phi.shape) == (2, 2 * R) and sh.phi.dtype == F64 and tuple(sh.scores.shape) == (2, 128)
    assert tuple(sh.coalitions.shape) == (128, 1) and sh.ok()
    want = [net.means(mri) * net.w0.detach(), net.means(pet) * net.w1.detach()]
    scale = float(torch.cat(want, 1).abs().max())
    for q in (0, 1):
        assert float((sh.values(q) - want[q]).abs().max()) <= 1e-9 * scale, q
    assert torch.equal(sh.values(), sh.values(0)) and torch.equal(sh.phi[:, R:].to(sh.logits.dtype), sh.values(1))
    total = sh.values(0).sum(1) + sh.values(1).sum(1)
    assert float((total.double() - sh.delta).abs().max()) <= 4 * 2 * R * si.U * float(sh.phi.abs().sum(1).max())
    assert torch.allclose(sh.delta, (sh.base_score - sh.empty_score).double(), rtol=0, atol=0)
    assert float((sh.r2() - 1).abs().max()) <= 1e-9
    z, _pad = si.unpack(sh.coalitions, 2 * R)
    assert torch.equal(sh.counts, torch.from_numpy(z.sum(0).astype(np.int32)))
    vmap = sh.volume(1)
    assert tuple(vmap.shape) == (2, 6, 6, 6) and bool((vmap[:, atlas == 0] == 0).all())
    assert torch.equal(vmap[:, atlas == 3], sh.values(1)[:, 2:3].expand(2, int((atlas == 3).sum())))
    idx, val = sh.top(3, 1)
    assert torch.equal(val, sh.values(1).gather(1, idx - 1)) and bool((val[:, :-1] >= val[:, 1:]).all())
    rows = sh.table({2: "two"})
    assert len(rows) == 2 * 2 * R and rows[1]["name"] == "two" and rows[R + 2]["volume"] == 1
    assert rows[R + 2]["value"] == float(sh.values(1)[0, 2])
    with pytest.raises(KeyError):
        T.region_shap_torch(net, mri, pet, atlas=atlas, samples=64, volumes=0, score="logit", target=0).values(1)


def test_separate_games_equal_single_volume_calls_and_baselines_run():
    import transmf_ad_amd as T
    net, mri, pet, atlas, R = _toy()
    kw = dict(atlas=atlas, samples=64, seed=9, score="logit", target=0, chunk=16)
    both = T.region_shap_torch(net, mri, pet, joint=False, **kw)
    assert both.players == 2 * R and not both.joint
    for q in (0, 1):
        one = T.region_shap_torch(net, mri, pet, volumes=q, **kw)
        assert one.players == R and torch.equal(one.values(), both.values(q)) and torch.equal(one.scores, both.of(q).scores)
        assert torch.equal(one.delta, both.of(q).delta) and torch.equal(one.phi, both.phi[:, q * R:(q + 1) * R])
    want = net.means(pet) * net.w1.detach()
    assert float((both.values(1) - want).abs().max()) <= 1e-9 * float(want.abs().max())
    # fill f: the share of region r becomes w (mean_r - f); a baseline tensor: w (mean_r(vol) - mean_r(baseline))
    f = T.region_shap_torch(net, mri, pet, volumes=1, fill=0.25, **kw)
    assert float((f.values() - net.w1.detach() * (net.means(pet) - 0.25)).abs().max()) <= 1e-9 * float(want.abs().max())
    b = T.region_shap_torch(net, mri, pet, volumes=1, baseline=mri, **kw)
    assert float((b.values() - net.w1.detach() * (net.means(pet) - net.means(mri))).abs().max()) <= 1e-9 * float(want.abs().max())
    assert T.region_shap_torch(net, mri, pet, volumes=0, baseline="blur", fill="mean", **kw).ok()
    unpaired = T.region_shap_torch(net, mri, pet, paired=False, atlas=atlas, samples=65, score="logit", target=0)
    assert unpaired.ok() and float((unpaired.values(1) - want).abs().max()) <= 1e-9 * float(want.abs().max())


def test_too_few_coalitions_and_argument_errors():
    import transmf_ad_amd as T
    net, mri, pet, atlas, R = _toy()
    few = T.region_shap_torch(net, mri, pet, atlas=atlas, samples=2, score="logit", target=0)
    assert not few.ok() and bool(few.values(0).isnan().all()) and bool(few.phi.isnan().all())
    assert T.region_shap_torch(net, mri, pet, atlas=atlas, samples=2, ridge=1.0, score="logit", target=0).ok()
    big = torch.arange(6 * 6 * 6, dtype=torch.int32).view(6, 6, 6) * 5            # 1075 labels: more players than the limit
    for kw, exc in ((dict(samples=1), ValueError), (dict(samples=7), ValueError), (dict(samples=8.0), ValueError),
                    (dict(atlas=atlas.double()), ValueError), (dict(atlas=atlas[:5]), ValueError), (dict(atlas=atlas * 0), ValueError),
                    (dict(atlas=big), ValueError), (dict(seed=-1), ValueError), (dict(ridge=-0.5), ValueError),
                    (dict(ridge=float("nan")), ValueError), (dict(score="loss"), ValueError), (dict(volumes=2), ValueError),
                    (dict(volumes=(0, 0)), ValueError), (dict(baseline="mean"), ValueError), (dict(baseline=mri[:1]), ValueError),
                    (dict(fill="median"), ValueError), (dict(chunk=0), ValueError), (dict(output=1), ValueError)):
        args = dict(atlas=atlas, samples=8)
        args.update(kw)
        with pytest.raises(exc):
            T.region_shap_torch(net, mri, pet, **args)
    with pytest.raises(ValueError, match="eval"):
        T.region_shap_torch(net.train(), mri, pet, atlas=atlas, samples=8)
    assert net.training
    with pytest.raises(TypeError):
        T.region_shap_torch(lambda a, b: a, mri, pet, atlas=atlas, samples=8)
    assert T.region_shap_torch(net.eval(), mri, pet, atlas=atlas, samples=7, paired=False, ridge=1.0).ok()
