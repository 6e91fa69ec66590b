"""Region Shapley values on the device: the kernels of csrc/shap.hip on their own (through _lib.call with raw pointers) against
the host Philox model, the torch twin of the select (bit for bit), the integer Gram matrix and the fp64 references of
tests/_shap_inputs.py; their refusals; the routing of the ops wrappers; region_shap against the model's own forward on batches
the test builds itself with shap_apply_torch, against region_shap_torch, with and without encoder reuse.

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs
included) must be unchanged, every output element written."""
import numpy as np
import pytest
import torch

import _shap_inputs as si
from test_gpu_bn_reduce import Arena, _call, _query, _st
from test_gpu_model import DEV
from test_gpu_rise import _bits_follow_the_batch, _calls, _package_model, _score

pytestmark = pytest.mark.gpu
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
ROWS = 73                                   # rows of the host model per (P, paired): m0 = 7 plus 66


def _i32(words):
    return torch.from_numpy(np.asarray(words).astype(np.uint32).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through raw pointers
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", si.PLAYERS)
def test_coalitions_kernel_equals_the_philox_model(P):
    """Byte for byte for N in 1, 2, 33, 66, paired and not, m0 = 0 and 7 (an odd m0 cuts a pair in two), two seeds with a
    non-zero high word.  A word of 32 members is the arena's fill pattern, so the arena only guards the surroundings here and
    every case also runs into a buffer of zeros: a word that was not written cannot equal the model in both."""
    Wd = si.words_of(P)
    cases = [(N, paired, m0) for N in si.COALITION_COUNTS for paired in (1, 0) for m0 in (0, 7)]
    outs = {f"c{i}": ((N, Wd), I32) for i, (N, _p, _m) in enumerate(cases)}
    ins = {"thr": _i32(si.size_table(P))} if P > 2 else {}
    ar = Arena(ins, outs, tail=4096)
    zeros = [torch.zeros((N, Wd), device=DEV, dtype=I32) for N, _p, _m in cases]
    for i, (N, paired, m0) in enumerate(cases):
        for dst in (ar.ptr(f"c{i}"), zeros[i].data_ptr()):
            _call("tmf_shap_coalitions", dst, ar.ptr("thr") if P > 2 else None, P, paired, si.SEEDS[paired], m0, N, _st())
    got = ar.fetch(workspace=tuple(outs))
    for i, (N, paired, m0) in enumerate(cases):
        want = si.coalitions(P, bool(paired), si.SEEDS[paired], 0, ROWS)[m0:m0 + N]
        assert torch.equal(got[f"c{i}"], want) and torch.equal(zeros[i].cpu(), want), (N, paired, m0)


APPLY_SIZES = {"scalar": (5, 6, 7), "vector": (4, 6, 8)}


@pytest.mark.parametrize("R", (1, 33, 70))
@pytest.mark.parametrize("kind", ("scalar", "vector"))
def test_apply_kernel_equals_the_twin(kind, R):
    """torch.equal with shap_apply_torch for p0 = 0 and p0 = R of P = 2 R players, with fill and with base, labels that hold 0,
    R + 1 and -1, B = 3: a chunk that straddles samples (j0 = N - 1, K = 3) and the chunk K = N + 1 that holds the zero row and
    more rows than the workgroups that share a tile stage in LDS at a time (71 rows against 8 workgroups of 8).  (5, 6, 7): one element per
    lane; (4, 6, 8): 16 bytes per lane (the arena's slots are 256-byte aligned) and once more through an output one element
    off, which forces the scalar path."""
    from transmf_ad_amd import ops
    size = APPLY_SIZES[kind]
    vol, fill, base = si.volumes(size)
    lab = si.labels_for(size, R)
    P, B, V = max(2 * R, 2), vol.shape[0], size[0] * size[1] * size[2]
    p0s = (0, R) if P >= 2 * R and R > 1 else (0, 1)
    coal = torch.cat([si.coalitions(P, True, si.SEEDS[0], 0, 70), torch.zeros((1, si.words_of(P)), dtype=I32)])
    N = coal.shape[0]
    chunks = [(N - 1, 3), (N, N), (0, N)]               # straddling; sample 1 whole: K = 70 + 1 with the zero row; sample 0 whole
    outs = {}
    for p0 in p0s:
        for i, (_j0, K) in enumerate(chunks):
            outs[f"fill{p0}_{i}"], outs[f"base{p0}_{i}"] = ((K, 1) + size, F32), ((K, 1) + size, F32)
    if kind == "vector":
        outs["off"] = ((chunks[0][1] * V + 1,), F32)
    ar = Arena(dict(vol=vol, lab=lab, coal=coal, fill=fill, base=base), outs, tail=4096)
    for p0 in p0s:
        for i, (j0, K) in enumerate(chunks):
            geo = (B, *size, R, p0, P, N, j0, K)
            _call("tmf_shap_apply", ar.ptr("vol"), ar.ptr("lab"), ar.ptr("coal"), ar.ptr("fill"), None, ar.ptr(f"fill{p0}_{i}"), *geo, _st())
            _call("tmf_shap_apply", ar.ptr("vol"), ar.ptr("lab"), ar.ptr("coal"), None, ar.ptr("base"), ar.ptr(f"base{p0}_{i}"), *geo, _st())
    written = None
    if kind == "vector":
        j0, K = chunks[0]
        _call("tmf_shap_apply", ar.ptr("vol"), ar.ptr("lab"), ar.ptr("coal"), ar.ptr("fill"), None, ar.ptr("off") + 4, B, *size, R,
              p0s[1], P, N, j0, K, _st())
        written = {"off": torch.ones(K * V + 1, dtype=torch.bool)}
        written["off"][0] = False
    got = ar.fetch(written=written)
    for p0 in p0s:
        for i, (j0, K) in enumerate(chunks):
            want = ops.shap_apply_torch(vol, lab, coal, fill, R, p0, P, j0, K)
            assert torch.equal(got[f"fill{p0}_{i}"], want), (p0, j0, K)
            assert torch.equal(got[f"base{p0}_{i}"], ops.shap_apply_torch(vol, lab, coal, None, R, p0, P, j0, K, base=base)), (p0, j0, K)
            if i == 0 and kind == "vector" and p0 == p0s[1]:
                assert torch.equal(got["off"][1:].view(want.shape), want)
    assert not torch.equal(got[f"fill{p0s[0]}_2"], got[f"fill{p0s[1]}_2"])                 # p0 matters
    zero_row = got[f"fill{p0s[0]}_1"][N - 1, 0]                                            # sample 1 under the empty coalition
    has = (lab >= 1) & (lab <= R)
    assert torch.equal(zero_row[has], fill[1].expand(int(has.sum()))) and torch.equal(zero_row[~has], vol[1, 0][~has])


@pytest.mark.parametrize("P", si.PLAYERS)
def test_gram_kernel(P):
    """A equals the integer reference exactly; rhs within N 2^-53 sum_m |y_m| of the ascending fp64 chain of the host (it IS
    that chain: the error is printed); two calls give the same bits.  N = 260 crosses the 128 coalitions a workgroup
    transposes at a time."""
    counts = si.GRAM_COUNTS + (260,)
    z_all = si.unpack(si.coalitions(P, True, si.SEEDS[0], 0, ROWS), P)[0]
    z_all = np.concatenate([z_all] * 4)[:max(counts)]
    if P <= 65:
        cases = [(N, B) for N in counts for B in si.GRAM_BATCHES if N != 260 or B == 3]
    else:                                   # (P, P) outputs of megabytes: every N and every B once
        cases = [(1, 1), (31, 3), (33, 9), (100, 3), (260, 3)]
    ins, outs = {}, {}
    for N in counts:
        ins[f"coal{N}"] = si.pack(z_all[:N])
    for N, B in cases:
        s, off = si.scores_for(B, N)
        ins[f"s{N}_{B}"], ins[f"o{N}_{B}"] = s, off
        for rep in "ab":
            outs[f"A{N}_{B}{rep}"], outs[f"r{N}_{B}{rep}"] = ((P, P), I32), ((B, P), F64)
    ar = Arena(ins, outs, tail=4096)
    for N, B in cases:
        for rep in "ab":
            _call("tmf_shap_gram", ar.ptr(f"coal{N}"), ar.ptr(f"s{N}_{B}"), ar.ptr(f"o{N}_{B}"), ar.ptr(f"A{N}_{B}{rep}"),
                  ar.ptr(f"r{N}_{B}{rep}"), B, P, N, _st())
    got = ar.fetch()
    worst = 0.0
    for N, B in cases:
        A, rhs, tol = si.gram_reference(z_all[:N], *si.scores_for(B, N))
        assert np.array_equal(got[f"A{N}_{B}a"].numpy(), A), (N, B)
        err = np.abs(got[f"r{N}_{B}a"].numpy() - rhs).max(1)
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all()), (N, B, (err / tol).max())
        assert torch.equal(got[f"A{N}_{B}a"], got[f"A{N}_{B}b"]) and torch.equal(got[f"r{N}_{B}a"], got[f"r{N}_{B}b"])
    print(f"P = {P}: worst rhs err / bound {worst:.3g}")


def _solve(A, rhs, delta, ridge, twice=False, nan=False):
    """tmf_shap_solve on host tensors -> {phi, info} host tensors (and phi2, info2 of a second call).  nan: phi may come back
    NaN, which is also the arena's fill pattern - it is then a buffer of zeros outside the arena."""
    B, P = rhs.shape
    nbytes = _query("tmf_shap_solve_workspace", B, P)
    outs = {"info": ((1,), I32), "ws": ((nbytes,), U8)}
    if not nan:
        outs["phi"] = ((B, P), F64)
    if twice:
        outs.update(phi2=((B, P), F64), info2=((1,), I32))
    ar = Arena(dict(A=A, rhs=rhs, delta=delta), outs, tail=4096)
    loose = torch.zeros((B, P), device=DEV, dtype=F64)
    for tag in ("", "2")[:2 if twice else 1]:
        _call("tmf_shap_solve", ar.ptr("A"), ar.ptr("rhs"), ar.ptr("delta"), ridge, loose.data_ptr() if nan else ar.ptr("phi" + tag),
              ar.ptr("info" + tag), ar.ptr("ws"), nbytes, B, P, _st())
    got = ar.fetch(workspace=("ws",))
    if nan:
        got["phi"] = loose.cpu()
    return got


@pytest.mark.parametrize("P,B", [(P, B) for P in si.SOLVE_PLAYERS for B in (1, 3)] + [(1024, 1)])
def test_solve_kernel_against_the_kkt_system(P, B):
    """phi against the numpy float64 solution of the KKT system of the same A, rhs and delta, within the header's bound
    16 P 2^-53 cond_2(M) max|phi| (cond_2 computed here); with a ridge; two calls give the same bits.  P = 1024 runs once."""
    A, rhs, delta = si.fit_case(P, B)
    got = _solve(A, rhs, delta, 0.0, twice=True)
    ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy())
    bound, cond = si.solve_bound(A.numpy(), 0.0, ref)
    err = np.abs(got["phi"].numpy() - ref).max(1)
    print(f"P = {P}, B = {B}: cond_2 {cond:.3g}, err / bound {(err / bound).max():.3g}")
    assert int(got["info"]) == 0 and bool((err <= bound).all()), (err / bound).max()
    assert torch.equal(got["phi"], got["phi2"]) and int(got["info2"]) == 0
    gap = np.abs(got["phi"].numpy().sum(1) - delta.numpy())
    assert bool((gap <= 4 * P * si.U * np.abs(got["phi"].numpy()).sum(1)).all())
    if P != 1024:
        got = _solve(A, rhs, delta, 0.25)
        ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy(), 0.25)
        err = np.abs(got["phi"].numpy() - ref).max(1)
        assert int(got["info"]) == 0 and bool((err <= si.solve_bound(A.numpy(), 0.25, ref)[0]).all())


def test_solve_kernel_singular_matrix_and_ridge():
    """Two paired coalitions for five players, and for the last seven of 40 players whose first 33 each have a coalition of their
    own (33 unit pivots: the failure lies in the second panel): the entries are 0 / 1, the factorisation is exact and meets a
    pivot of 0; info is its 1-based index as torch.linalg.cholesky_ex reports it and every phi is NaN; a ridge solves it."""
    from transmf_ad_amd import ops
    for P in (5, 40):
        z = si.coalition_bits(P, True, 3, 0, 2)
        if P == 40:
            z = np.zeros((35, 40), bool)
            z[:33, :33] = np.eye(33, dtype=bool)
            z[33:, 33:] = si.coalition_bits(7, True, 3, 0, 2)
        scores, offset = si.scores_for(2, z.shape[0])
        A, rhs = ops.shap_gram_torch(si.pack(z), scores, offset, P)
        delta = torch.tensor([0.5, -1.0], dtype=F64)
        _phi, want_info = ops.shap_solve_torch(A, rhs, delta)
        got = _solve(A, rhs, delta, 0.0, nan=True)
        assert int(want_info) >= (1 if P == 5 else 34) and int(got["info"]) == int(want_info), (P, int(got["info"]), int(want_info))
        assert bool(got["phi"].isnan().all())
        got = _solve(A, rhs, delta, 0.5)
        ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy(), 0.5)
        assert int(got["info"]) == 0
        assert bool((np.abs(got["phi"].numpy() - ref).max(1) <= si.solve_bound(A.numpy(), 0.5, ref)[0]).all())


# ---------------------------------------------------------------------------------------------------------------------
# refusals: bad arguments on real buffers full of a sentinel - a negative code, and every buffer unchanged
# ---------------------------------------------------------------------------------------------------------------------

def _sentinels():
    f = torch.full((4 * 512 + 64,), 7.0, device=DEV)
    o = torch.full((8 * 512 + 64,), 7.0, device=DEV)
    i = torch.full((4096,), 1, device=DEV, dtype=I32)
    d = torch.full((4096,), 7.0, device=DEV, dtype=F64)
    return f, o, i, d


def _unchanged(f, o, i, d):
    torch.cuda.synchronize()
    return bool((f == 7.0).all()) and bool((o == 7.0).all()) and bool((i == 1).all()) and bool((d == 7.0).all())


def test_coalitions_entry_refuses_before_any_launch():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    bufs = _sentinels()
    c, t = bufs[2].data_ptr(), bufs[2].data_ptr() + 8192
    call = lambda coal=c, thr=t, P=5, paired=1, m0=0, N=4: lib.tmf_shap_coalitions(coal, thr, P, paired, 1, m0, N, None)
    for kw in (dict(coal=None), dict(thr=None), dict(P=1), dict(P=1025), dict(paired=2), dict(paired=-1), dict(N=0), dict(m0=-1),
               dict(m0=2 ** 31 - 2, N=4), dict(coal=c + 2), dict(thr=t + 1)):
        assert call(**kw) < 0, kw
    assert lib.tmf_shap_coalitions(None, None, 2, 1, 1, 0, 2, None) == _lib.E_NULL
    assert b"tmf_shap_coalitions" in lib.tmf_last_error_string() and _unchanged(*bufs)


def test_apply_entry_refuses_before_any_launch():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    bufs = _sentinels()
    p, q, l = bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()
    c = l + 4 * 512
    call = lambda vol=p, lab=l, coal=c, fill=p, base=None, out=q, B=2, g=(8, 8, 8), R=3, p0=2, P=5, N=4, j0=0, K=1: \
        lib.tmf_shap_apply(vol, lab, coal, fill, base, out, B, *g, R, p0, P, N, j0, K, None)
    for kw in (dict(vol=None), dict(lab=None), dict(coal=None), dict(out=None), dict(fill=None), dict(B=0), dict(B=65537), dict(N=0),
               dict(g=(8, 0, 8)), dict(g=(2048, 2048, 512)), dict(R=0), dict(p0=-1), dict(p0=3), dict(P=1), dict(P=1025),
               dict(j0=-1), dict(K=0), dict(j0=8), dict(j0=6, K=3), dict(K=65537), dict(vol=p + 2), dict(out=q + 1), dict(lab=l + 2),
               dict(coal=c + 1), dict(fill=None, base=p + 2), dict(out=p), dict(out=p + 4 * 512), dict(vol=q + 4, out=q),
               dict(B=65536, N=32768)):
        assert call(**kw) < 0, kw
    assert b"tmf_shap_apply" in lib.tmf_last_error_string() and _unchanged(*bufs)


def test_gram_entry_refuses_before_any_launch():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    bufs = _sentinels()
    s, c, r = bufs[0].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr()
    a = c + 4096
    call = lambda coal=c, sc=s, off=s + 256, A=a, rhs=r, B=2, P=5, N=4: lib.tmf_shap_gram(coal, sc, off, A, rhs, B, P, N, None)
    for kw in (dict(coal=None), dict(sc=None), dict(off=None), dict(A=None), dict(rhs=None), dict(B=0), dict(B=65537), dict(P=1),
               dict(P=1025), dict(N=0), dict(B=65536, N=32768), dict(coal=c + 2), dict(sc=s + 1), dict(off=s + 2), dict(A=a + 2),
               dict(rhs=r + 4)):
        assert call(**kw) < 0, kw
    assert b"tmf_shap_gram" in lib.tmf_last_error_string() and _unchanged(*bufs)


def test_solve_entry_refuses_before_any_launch():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    bufs = _sentinels()
    a, r = bufs[2].data_ptr(), bufs[3].data_ptr()
    d, phi, ws, info = r + 1024, r + 2048, r + 8192, a + 8192
    need = lib.tmf_shap_solve_workspace(2, 5)
    assert need == (2 * 32 * 32 + 3 * 32) * 8 and need <= 4096 * 8 - 8192 and lib.tmf_shap_solve_workspace(2, 33) > need
    assert lib.tmf_shap_solve_workspace(0, 5) == lib.tmf_shap_solve_workspace(2, 1) == lib.tmf_shap_solve_workspace(2, 1025) == 0
    call = lambda A=a, rhs=r, delta=d, ridge=0.0, phi=phi, info=info, ws=ws, nbytes=need, B=2, P=5: \
        lib.tmf_shap_solve(A, rhs, delta, ridge, phi, info, ws, nbytes, B, P, None)
    for kw in (dict(A=None), dict(rhs=None), dict(delta=None), dict(phi=None), dict(info=None), dict(ws=None), dict(B=0),
               dict(B=65537), dict(P=1), dict(P=1025), dict(ridge=-1.0), dict(ridge=float("nan")), dict(ridge=float("inf")),
               dict(A=a + 2), dict(info=info + 1), dict(rhs=r + 4), dict(delta=d + 4), dict(phi=phi + 4), dict(ws=ws + 8),
               dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**kw) < 0, kw
    assert call(nbytes=need - 1) == _lib.E_WORKSPACE
    assert b"tmf_shap_solve" in lib.tmf_last_error_string() and _unchanged(*bufs)


# ---------------------------------------------------------------------------------------------------------------------
# the ops wrappers
# ---------------------------------------------------------------------------------------------------------------------

def test_ops_wrappers_route(monkeypatch):
    """Contiguous float32 HIP tensors take the kernels, anything else the torch formulas: the same values."""
    from transmf_ad_amd import ops
    size, R, P, N = (4, 6, 8), 33, 66, 34
    vol, fill, base = si.volumes(size)
    lab = si.labels_for(size, R)
    want = si.coalitions(P, True, si.SEEDS[0], 0, N)
    coal, names = _calls(monkeypatch, lambda: ops.shap_coalitions(P, True, si.SEEDS[0], 0, N, DEV))
    assert names == ["tmf_shap_size_table", "tmf_shap_coalitions"] and torch.equal(coal.cpu(), want)
    host, names = _calls(monkeypatch, lambda: ops.shap_coalitions(P, True, si.SEEDS[0], 0, N, "cpu"))
    assert names == [] and torch.equal(host, want)
    v, f, b, l = vol.to(DEV), fill.to(DEV), base.to(DEV), lab.to(DEV)
    assert ops.shap_ok(v, l, coal, f) and not ops.shap_ok(vol, coal) and not ops.shap_ok(v.half(), coal)
    j0, K = N - 1, 3
    ref = ops.shap_apply_torch(vol, lab, want, fill, R, 33, P, j0, K)
    got, names = _calls(monkeypatch, lambda: ops.shap_apply(v, l, coal, f, R, 33, P, j0, K))
    assert names == ["tmf_shap_apply"] and torch.equal(got.cpu(), ref)
    buf = torch.empty((K + 2, 1) + size, device=DEV)
    got, names = _calls(monkeypatch, lambda: ops.shap_apply(v, l, coal, None, R, 33, P, j0, K, base=b, out=buf[:K]))
    assert names == ["tmf_shap_apply"] and got.data_ptr() == buf.data_ptr()
    assert torch.equal(got.cpu(), ops.shap_apply_torch(vol, lab, want, None, R, 33, P, j0, K, base=base))
    assert torch.equal(ops.shap_apply_torch(v, l, coal, f, R, 33, P, j0, K).cpu(), ref)              # the twin on the device
    got, names = _calls(monkeypatch, lambda: ops.shap_apply(v.double(), l, coal, f.double(), R, 33, P, j0, K))
    assert names == [] and got.dtype == F64 and torch.equal(got.cpu(), ref.double())
    got, names = _calls(monkeypatch, lambda: ops.shap_apply(v, l.long(), coal, f, R, 33, P, j0, K))
    assert names == [] and torch.equal(got.cpu(), ref)
    wide = torch.zeros((3, 1) + size[:2] + (2 * size[2],), device=DEV)
    wide[..., ::2] = v
    got, names = _calls(monkeypatch, lambda: ops.shap_apply(wide[..., ::2], l, coal, f, R, 33, P, j0, K))
    assert names == [] and torch.equal(got.cpu(), ref)
    s, off = si.scores_for(3, N)
    z = si.unpack(want, P)[0]
    A, rhs, tol = si.gram_reference(z, s, off)
    (gA, gr), names = _calls(monkeypatch, lambda: ops.shap_gram(coal, s.to(DEV), off.to(DEV), P))
    assert names == ["tmf_shap_gram"] and np.array_equal(gA.cpu().numpy(), A) and bool((np.abs(gr.cpu().numpy() - rhs).max(1) <= tol).all())
    (tA, tr), names = _calls(monkeypatch, lambda: ops.shap_gram(coal, s.to(DEV).double(), off.to(DEV).double(), P))
    assert names == [] and np.array_equal(tA.cpu().numpy(), A) and bool((np.abs(tr.cpu().numpy() - rhs).max(1) <= tol).all())
    A, rhs, delta = si.fit_case(33, 3)
    ref = si.kkt(A.numpy(), rhs.numpy(), delta.numpy())
    bound = si.solve_bound(A.numpy(), 0.0, ref)[0]
    (phi, info), names = _calls(monkeypatch, lambda: ops.shap_solve(A.to(DEV), rhs.to(DEV), delta.to(DEV)))
    assert names == ["tmf_shap_solve"] and int(info) == 0 and bool((np.abs(phi.cpu().numpy() - ref).max(1) <= bound).all())
    (phi, info), names = _calls(monkeypatch, lambda: ops.shap_solve(A.to(DEV).long(), rhs.to(DEV), delta.to(DEV)))
    assert names == [] and int(info) == 0 and bool((np.abs(phi.cpu().numpy() - ref).max(1) <= bound).all())
    (phi, info), names = _calls(monkeypatch, lambda: ops.shap_solve(A, rhs, delta))
    assert names == [] and phi.device.type == "cpu"


# ---------------------------------------------------------------------------------------------------------------------
# region_shap against the model's own forward and against region_shap_torch
# ---------------------------------------------------------------------------------------------------------------------

def _loop(net, vols, which, rows, atlas, R, P, target, chunk):
    """The user's loop through the model's own forward: shap_apply_torch (fill 0) on the volumes `which`, in chunks of `chunk`
    jobs -> scores (B, rows)."""
    from transmf_ad_amd import ops
    B, N = vols[0].shape[0], rows.shape[0]
    zero = torch.zeros(B, device=DEV)
    outs = []
    with torch.no_grad():
        for j0 in range(0, B * N, chunk):
            K = min(chunk, B * N - j0)
            at = torch.arange(j0, j0 + K, device=DEV) // N
            batch = [v.index_select(0, at) for v in vols]
            for q, i in enumerate(which):
                batch[i] = ops.shap_apply_torch(vols[i], atlas, rows, zero, R, q * R, P, j0, K)
            out = net(*batch)
            out = out[0] if isinstance(out, tuple) else out
            outs.append(_score(out, target.index_select(0, at)))
    return torch.cat(outs).view(B, N)


@pytest.mark.parametrize("name", ("cnn_tiny", "ad_tiny"))
def test_region_shap_is_the_models_own_forward_and_the_twins_fit(name, monkeypatch):
    """A 3 x 3 x 3-block atlas (R = 27, P = 54 jointly), samples = 256, chunk = 8: chunks straddle samples and the zero row sits
    in a partial chunk.  scores and empty_score equal, bit for bit, the model's own forward on volumes the twin writes; phi
    matches region_shap_torch within the solve bound plus the propagated difference of the right-hand sides,
    2 sqrt(P) / lambda_min(M) * (sum_m |scores - scores_twin| + N 2^-53 sum_m |y_m|) + |delta - delta_twin|; sum(phi) = delta;
    one apply launch per chunk and volume, one gram and one solve call, no host read through info; reuse=True and reuse=False
    agree (or the kept encoder's bits follow the batch size); the model and torch's generators are unchanged."""
    import transmf_ad_amd as T
    from transmf_ad_amd import ops
    net, vols, size = _package_model(name)
    atlas = si.block_atlas(size, 3).to(DEV)
    B, N, R, P, chunk, seed = vols[0].shape[0], 256, 27, 54, 8, si.SEEDS[1]
    nchunks = -(-B * (N + 1) // chunk)
    assert (N + 1) % chunk and B * (N + 1) % chunk
    keep = {k: v.clone() for k, v in net.state_dict().items()}
    rng, rng_host = torch.cuda.get_rng_state(0), torch.get_rng_state()
    sh, names = _calls(monkeypatch, lambda: T.region_shap(net, *vols, atlas=atlas, samples=N, seed=seed, chunk=chunk))
    assert names.count("tmf_shap_coalitions") == 1 and names.count("tmf_shap_apply") == 2 * nchunks
    assert names.count("tmf_shap_gram") == 1 and names.count("tmf_shap_solve") == 1
    assert sh.R == R and sh.players == P and sh.volumes == (0, 1) and sh.joint and sh.ok()
    coal = si.coalitions(P, True, seed, 0, N)
    assert torch.equal(sh.coalitions.cpu(), coal)
    rows = torch.cat([sh.coalitions, torch.zeros((1, 2), device=DEV, dtype=I32)])
    target = sh.logits.argmax(1)
    assert torch.equal(sh.target, target) and torch.equal(sh.base_score, _score(sh.logits, target))
    want = _loop(net, vols, (0, 1), rows, atlas, R, P, target, chunk)
    assert torch.equal(sh.scores, want[:, :N]) and torch.equal(sh.empty_score, want[:, N])
    assert float((sh.scores - sh.base_score.view(B, 1)).abs().max()) > 0
    tw = T.region_shap_torch(net, *vols, atlas=atlas, samples=N, seed=seed, chunk=chunk)
    assert tw.ok() and torch.equal(tw.coalitions.cpu(), coal)
    z = si.unpack(coal, P)[0].astype(np.int64)
    A = z.T @ z
    assert np.array_equal(sh.counts.cpu().numpy(), np.diag(A))
    ref = tw.phi.cpu().numpy()
    bound, cond = si.solve_bound(A, 0.0, ref)
    y = (sh.scores.double() - sh.empty_score.double().view(B, 1)).cpu().numpy()
    dy = (sh.scores.double() - tw.scores.double()).abs().sum(1).cpu().numpy()
    lam = np.linalg.eigvalsh(A.astype(np.float64))[0]
    tol = bound + 2 * P ** 0.5 / lam * (dy + N * si.U * np.abs(y).sum(1)) + (sh.delta - tw.delta).abs().cpu().numpy()
    err = np.abs(sh.phi.cpu().numpy() - ref).max(1)
    print(f"{name}: cond_2 {cond:.3g}, max |scores - twin's| {dy.max():.3g}, phi err / tolerance {(err / tol).max():.3g}, r2 {sh.r2().tolist()}")
    assert bool((err <= tol).all()), (err / tol).tolist()
    phi = sh.phi.cpu().numpy()
    assert bool((np.abs(phi.sum(1) - sh.delta.cpu().numpy()) <= 4 * P * si.U * np.abs(phi).sum(1)).all())
    total = (sh.values(0).double().sum(1) + sh.values(1).double().sum(1)).cpu().numpy()
    assert bool((np.abs(total - sh.delta.cpu().numpy()) <= (P + 1) * 2.0 ** -24 * np.abs(phi).sum(1)).all())
    assert torch.equal(sh.delta, sh.base_score.double() - sh.empty_score.double())
    assert tuple(sh.values(1).shape) == (B, R) and sh.values(1).dtype == sh.logits.dtype
    vmap = sh.volume(1)
    assert tuple(vmap.shape) == (B,) + size and torch.equal(vmap[:, atlas == 5], sh.values(1)[:, 4:5].expand(B, int((atlas == 5).sum())))
    one = [T.region_shap(net, *vols, atlas=atlas, samples=N, seed=seed, chunk=chunk, volumes=0, joint=False, reuse=r) for r in (False, True)]
    assert one[0].players == R and torch.equal(one[0].coalitions.cpu(), si.coalitions(R, True, seed, 0, N))
    same = torch.equal(one[0].scores, one[1].scores) and torch.equal(one[0].phi, one[1].phi)
    print(f"{name}: max |scores(reuse=True) - scores(reuse=False)| = {float((one[0].scores - one[1].scores).abs().max()):.3e}")
    assert same or _bits_follow_the_batch(net.pet_cnn, vols[1], N + 1, chunk)
    assert all(torch.equal(v, keep[k]) for k, v in net.state_dict().items()) and all(p.grad is None for p in net.parameters())
    assert torch.equal(torch.cuda.get_rng_state(0), rng) and torch.equal(torch.get_rng_state(), rng_host)
