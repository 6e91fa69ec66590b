"""CPU-only checks of RISE (transmf_ad_amd/rise.py, the torch twins of ops.py, the host side of csrc/rise.hip): the binding, the
geometry, the nodes and shifts against the host Philox model of tests/_rise_inputs.py, the float32 mask formula against a
scalar numpy restatement (bit for bit) and against float64 (the header's bound), jobs and chunks of rise_apply_torch, the
bound of rise_accumulate_torch, the refusals of the entries with pointers that are never dereferenced, every ValueError of the
public function and the planted evidence it must find."""
import ctypes

import numpy as np
import pytest
import torch

import _rise_inputs as ri

F32, F64 = torch.float32, torch.float64
SMALL = ri.GEOMETRIES[:4]                # the scalar restatement walks voxel by voxel


def test_symbols_exports_and_geometry():
    import transmf_ad_amd
    from transmf_ad_amd import _lib, ops
    from transmf_ad_amd.build import FILE_FLAGS, SOURCES
    C, P = ctypes, _lib.PROTOTYPES
    assert P["tmf_rise_geometry"] == (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 2)
    assert P["tmf_rise_masks"] == (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_float, C.c_ulonglong, C.c_int, C.c_int, C.c_void_p])
    assert P["tmf_rise_apply"] == (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 10 + [C.c_void_p])
    assert P["tmf_rise_accumulate"] == (C.c_int, [C.c_void_p] * 4 + [C.c_float] + [C.c_int] * 10 + [C.c_void_p])
    assert "rise.hip" in SOURCES and FILE_FLAGS["rise.hip"] == ["-ffp-contract=off"]
    for name in ("rise", "rise_torch", "Rise"):
        assert name in transmf_ad_amd.__all__ and callable(getattr(transmf_ad_amd, name))
    for name in ("rise_geometry", "rise_masks", "rise_masks_torch", "rise_apply", "rise_apply_torch", "rise_accumulate",
                 "rise_accumulate_torch", "rise_ok"):
        assert callable(getattr(ops, name)), name
    lib = _lib.load()
    for size, cells in ri.GEOMETRIES + [ri.STRIDING, ((96, 96, 96), (8, 8, 8)), ((7, 1, 3), (7, 1, 1))]:
        cell, nodes = (C.c_int * 3)(), (C.c_int * 3)()
        G = lib.tmf_rise_geometry(*size, *cells, cell, nodes)
        assert (tuple(cell), tuple(nodes), G) == ri.geometry(size, cells) == ops.rise_geometry(size, cells), (size, cells)
        assert all((c - 1) * s < S <= c * s for c, s, S in zip(tuple(cell), cells, size))           # c = ceil(S / s)
    assert ops.rise_geometry((96, 96, 96), 8) == ((12, 12, 12), (10, 10, 10), 1000)
    for size, cells in (((8, 8, 8), (0, 1, 1)), ((8, 8, 8), (1, 9, 1)), ((8, 8, 8), (1, 1, -2))):
        assert lib.tmf_rise_geometry(*size, *cells, cell, nodes) == _lib.E_ARG
        with pytest.raises(ValueError):
            ops.rise_geometry(size, cells)
    assert lib.tmf_rise_geometry(0, 8, 8, 1, 1, 1, cell, nodes) == _lib.E_SHAPE
    assert lib.tmf_rise_geometry(2048, 1024, 1024, 1, 1, 1, cell, nodes) == _lib.E_SHAPE
    assert lib.tmf_rise_geometry(1 << 30, 1, 1, 1 << 30, 1, 1, cell, nodes) == _lib.E_SHAPE           # the node grid
    assert lib.tmf_rise_geometry(8, 8, 8, 1, 1, 1, None, nodes) == lib.tmf_rise_geometry(8, 8, 8, 1, 1, 1, cell, None) == _lib.E_NULL


def test_entries_refuse_before_any_launch():
    """Every refusal of include/tmf_hip.h with pointers that are never dereferenced: the checks run ahead of the launches."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    V, ND, SH, F, BS, O, SC = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000
    geo = (8, 8, 8, 2, 2, 2)

    def masks(nodes=ND, shifts=SH, geo=geo, p=0.5, seed=1, m0=0, N=4):
        return lib.tmf_rise_masks(nodes, shifts, *geo, p, seed, m0, N, None)

    def apply(vol=V, nodes=ND, shifts=SH, fill=F, base=None, out=O, B=2, geo=geo, N=4, j0=0, K=1):
        return lib.tmf_rise_apply(vol, nodes, shifts, fill, base, out, B, *geo, N, j0, K, None)

    def acc(scores=SC, nodes=ND, shifts=SH, sal=O, scale=1.0, B=2, geo=geo, N=4, m_first=0, m_step=1):
        return lib.tmf_rise_accumulate(scores, nodes, shifts, sal, scale, B, *geo, N, m_first, m_step, None)

    assert masks(nodes=None) == masks(shifts=None) == _lib.E_NULL
    assert apply(vol=None) == apply(nodes=None) == apply(shifts=None) == apply(out=None) == apply(fill=None) == _lib.E_NULL
    assert acc(scores=None) == acc(nodes=None) == acc(shifts=None) == acc(sal=None) == _lib.E_NULL
    for g in ((0, 8, 8, 2, 2, 2), (8, -1, 8, 2, 2, 2), (2048, 1024, 1024, 2, 2, 2)):
        assert masks(geo=g) == apply(geo=g) == acc(geo=g) == _lib.E_SHAPE, g
    for g in ((8, 8, 8, 0, 2, 2), (8, 8, 8, 2, 9, 2), (8, 8, 8, 2, 2, -1)):
        assert masks(geo=g) == apply(geo=g) == acc(geo=g) == _lib.E_ARG, g
    for p in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert masks(p=p) == _lib.E_ARG, p
    for m0, N in ((0, 0), (0, -1), (-1, 4), (2 ** 31 - 4, 4), (1, 2 ** 31 - 1)):
        assert masks(m0=m0, N=N) == _lib.E_ARG, (m0, N)
    assert apply(N=0) == acc(N=0) == _lib.E_ARG
    for B in (0, -1, 65537):
        assert apply(B=B) == acc(B=B) == _lib.E_SHAPE, B
    assert apply(B=65536, N=32768) == acc(B=65536, N=32768) == _lib.E_SHAPE                             # B * N = 2^31
    for j0, K in ((0, 0), (0, -1), (-1, 1), (8, 1), (6, 3), (0, 65537)):
        assert apply(j0=j0, K=K, N=4 if K < 100 else 1 << 20) == _lib.E_ARG, (j0, K)
    for m_first, m_step in ((0, 0), (0, -1), (-1, 1), (4, 1), (5, 2)):
        assert acc(m_first=m_first, m_step=m_step) == _lib.E_ARG, (m_first, m_step)
    assert masks(shifts=SH + 2) == apply(vol=V + 2) == apply(shifts=SH + 1) == apply(fill=F + 2) == apply(out=O + 3) == _lib.E_ALIGN
    assert apply(fill=None, base=BS + 1) == acc(scores=SC + 2) == acc(shifts=SH + 2) == acc(sal=O + 1) == _lib.E_ALIGN
    n = 512 * 4
    for out, K in ((V, 1), (V + 4, 1), (V + 2 * n - 4, 1), (V - n + 4, 1), (V - 3 * n + 4, 3)):
        assert apply(out=out, K=K) == _lib.E_ARG, hex(out)
    assert b"tmf_rise_apply" in lib.tmf_last_error_string()


@pytest.mark.parametrize("geom", ri.GEOMETRIES, ids=ri.geom_id)
def test_nodes_and_shifts_are_a_function_of_seed_and_mask(geom):
    """rise_masks_torch equals the host Philox model byte for byte; 0 <= t < c; masks m0 .. m0+N-1 drawn in two calls equal one
    call; another seed, another p, another mask: other bytes."""
    from transmf_ad_amd import ops
    size, cells = geom
    cell, nn, _G = ri.geometry(size, cells)
    for seed in ri.SEEDS:
        nodes, shifts = ops.rise_masks_torch(size, cells, ri.P, seed, 0, ri.MASKS)
        want_n, want_s = ri.masks_model(size, cells, ri.P, seed, 0, ri.MASKS)
        assert nodes.dtype == torch.uint8 and shifts.dtype == torch.int32 and tuple(nodes.shape) == (ri.MASKS,) + nn
        assert torch.equal(nodes, want_n) and torch.equal(shifts, want_s), seed
        assert bool((shifts >= 0).all()) and bool((shifts < torch.tensor(cell)).all()) and int(nodes.max()) <= 1
        a, b = ops.rise_masks_torch(size, cells, ri.P, seed, 0, 4), ops.rise_masks_torch(size, cells, ri.P, seed, 4, ri.MASKS - 4)
        assert torch.equal(torch.cat([a[0], b[0]]), nodes) and torch.equal(torch.cat([a[1], b[1]]), shifts)
    other = ops.rise_masks_torch(size, cells, ri.P, ri.SEEDS[0], 0, ri.MASKS)[0]
    assert not torch.equal(other, nodes) and not torch.equal(nodes[0], nodes[1])
    low = ops.rise_masks_torch(size, cells, 0.1, ri.SEEDS[2], 0, ri.MASKS)[0]
    assert int(low.sum()) < int(nodes.sum()) and bool((low <= nodes).all())              # the same words under a lower threshold


def test_node_rate_and_value_errors_of_the_mask_wrappers():
    from transmf_ad_amd import ops
    nodes, _s = ops.rise_masks_torch((16, 16, 16), 6, 0.3, 9, 0, 200)
    rate, sigma = float(nodes.float().mean()), (0.3 * 0.7 / nodes.numel()) ** 0.5
    assert abs(rate - 0.3) < 4 * sigma
    for kw in (dict(p=0.0), dict(p=1.0), dict(p="0.5"), dict(seed=-1), dict(seed=1 << 64), dict(N=0), dict(m0=-1), dict(cells=(1, 2)),
               dict(cells=17), dict(cells=0)):
        args = dict(size=(16, 16, 16), cells=4, p=0.5, seed=0, m0=0, N=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.rise_masks_torch(**args)


@pytest.mark.parametrize("geom", SMALL, ids=ri.geom_id)
def test_mask_formula_bits_and_bound(geom):
    """The float32 twin formula equals the scalar numpy restatement bit for bit, lies within 16 * 2^-24 of the float64 twin and
    inside [0, 1 + 2^-22]; with cell 1 it is the node itself."""
    from transmf_ad_amd import ops
    size, cells = geom
    nodes, shifts = ri.masks_model(size, cells, ri.P, ri.SEEDS[1], 0, 4)
    M32 = ops.rise_mask_values(nodes, shifts, size, cells)
    M64 = ops.rise_mask_values(nodes, shifts, size, cells, F64)
    assert M32.dtype == F32 and M64.dtype == F64 and tuple(M32.shape) == (4,) + size
    for m in range(4):
        want = ri.mask_scalar32(nodes[m].numpy(), shifts[m].numpy(), size, cells)
        assert np.array_equal(M32[m].numpy(), want), m
    err = float((M32.double() - M64).abs().max())
    print(f"{ri.geom_id(geom)}: max |M32 - M64| = {err * 2 ** 24:.3f} * 2^-24")
    assert err <= ri.MASK_BOUND and float(M32.min()) >= 0 and float(M32.max()) <= ri.MASK_MAX
    assert float(M64.min()) >= 0 and float(M64.max()) <= 1
    if max(ri.geometry(size, cells)[0]) == 1:
        assert bool((shifts == 0).all()) and torch.equal(M32, nodes[:, :size[0], :size[1], :size[2]].float())
    assert ops.rise_mask_values(nodes, shifts, size, cells, torch.bfloat16).dtype == torch.bfloat16


@pytest.mark.parametrize("geom", ri.GEOMETRIES[:5], ids=ri.geom_id)
def test_apply_twin_jobs_and_chunks(geom):
    """Job j = b*N + m across a chunk that straddles samples; fill 0 equals M * vol bit for bit; fill and base follow
    f + M * (vol - f); chunks cut anywhere give the rows of the whole."""
    from transmf_ad_amd import ops
    size, cells = geom
    vol, fill, base = ri.volumes(size)
    B, N = vol.shape[0], ri.MASKS
    nodes, shifts = ri.masks_model(size, cells, ri.P, ri.SEEDS[0], 0, N)
    M = ops.rise_mask_values(nodes, shifts, size, cells)
    zero = torch.zeros(B)
    whole = ops.rise_apply_torch(vol, nodes, shifts, zero, size, cells, 0, B * N)
    for j in range(B * N):
        assert torch.equal(whole[j, 0], M[j % N] * vol[j // N, 0]), j
    for j0, K in ri.chunkings(B, N):
        assert torch.equal(ops.rise_apply_torch(vol, nodes, shifts, zero, size, cells, j0, K), whole[j0:j0 + K])
        got = ops.rise_apply_torch(vol, nodes, shifts, fill, size, cells, j0, K)
        gotb = ops.rise_apply(vol, nodes, shifts, None, size, cells, j0, K, base=base)           # CPU tensors: the twin
        for k in range(K):
            b, m = divmod(j0 + k, N)
            assert torch.equal(got[k, 0], fill[b] + M[m] * (vol[b, 0] - fill[b]))
            assert torch.equal(gotb[k, 0], base[b, 0] + M[m] * (vol[b, 0] - base[b, 0]))
    buf = torch.empty((4, 1) + size)
    assert ops.rise_apply_torch(vol, nodes, shifts, fill, size, cells, 2, 4, out=buf).data_ptr() == buf.data_ptr()
    d = ops.rise_apply_torch(vol.double(), nodes, shifts, fill.double(), size, cells, 0, 2)
    assert d.dtype == F64 and float((d - ops.rise_apply_torch(vol, nodes, shifts, fill, size, cells, 0, 2)).abs().max()) < 1e-5
    for j0, K in ((0, 0), (-1, 1), (B * N, 1), (B * N - 1, 2)):
        with pytest.raises(ValueError):
            ops.rise_apply_torch(vol, nodes, shifts, fill, size, cells, j0, K)
    with pytest.raises(ValueError):
        ops.rise_apply_torch(vol, nodes, shifts, fill[:2], size, cells, 0, 1)
    with pytest.raises(ValueError):
        ops.rise_apply_torch(vol, nodes[:, 1:], shifts, fill, size, cells, 0, 1)


@pytest.mark.parametrize("geom", ri.GEOMETRIES[:5], ids=ri.geom_id)
def test_accumulate_twin_bound_halves_and_coverage(geom):
    """The float32 twin within the header's bound of the float64 twin; even plus odd halves sum to the whole within it; the
    coverage (scores of ones) lies between 0 and N."""
    from transmf_ad_amd import ops
    size, cells = geom
    B, N = 3, ri.MASKS
    nodes, shifts = ri.masks_model(size, cells, ri.P, ri.SEEDS[2], 0, N)
    s = ri.scores_for(B, N)
    scale = 1.0 / (N * ri.P)
    ref = ops.rise_accumulate_torch(s.double(), nodes, shifts, size, cells, scale)
    got = ops.rise_accumulate(s, nodes, shifts, size, cells, scale)                               # CPU tensors: the twin
    M64 = ops.rise_mask_values(nodes, shifts, size, cells, F64)
    assert ref.dtype == F64 and torch.allclose(ref, scale * torch.einsum("bn,ndhw->bdhw", s.double(), M64), rtol=0, atol=1e-13)
    err, tol = ri.row_errors(got, ref), ri.map_tolerance(s, scale, range(N))
    print(f"{ri.geom_id(geom)}: err / tol {(err / tol).tolist()}")
    assert got.dtype == F32 and tuple(got.shape) == (B,) + size and bool((err <= tol).all())
    even = ops.rise_accumulate_torch(s, nodes, shifts, size, cells, scale, 0, 2)
    odd = ops.rise_accumulate_torch(s, nodes, shifts, size, cells, scale, 1, 2)
    tol2 = ri.map_tolerance(s, scale, range(0, N, 2)) + ri.map_tolerance(s, scale, range(1, N, 2))
    assert bool((ri.row_errors(even.double() + odd.double(), ref) <= tol2).all())
    assert bool((ri.row_errors(even, ops.rise_accumulate_torch(s.double(), nodes, shifts, size, cells, scale, 0, 2))
                 <= ri.map_tolerance(s, scale, range(0, N, 2))).all())
    cover = ops.rise_accumulate_torch(torch.ones((1, N)), nodes, shifts, size, cells)
    assert float(cover.min()) >= 0 and float(cover.max()) <= N * ri.MASK_MAX
    assert bool((ri.row_errors(cover, M64.sum(0, keepdim=True)) <= ri.map_tolerance(torch.ones((1, N)), 1.0, range(N))).all())
    assert bool((ri.row_errors(ops.rise_accumulate_torch(s, nodes, shifts, size, cells, scale, chunk=3), ref) <= tol).all())
    for m_first, m_step in ((0, 0), (-1, 1), (N, 1)):
        with pytest.raises(ValueError):
            ops.rise_accumulate_torch(s, nodes, shifts, size, cells, scale, m_first, m_step)
    with pytest.raises(ValueError):
        ops.rise_accumulate_torch(s[:, 1:], nodes, shifts, size, cells, scale)


class Cube(torch.nn.Module):
    """The planted evidence: two classes whose logits are +- the mean of the volume over a fixed 5 x 5 x 5 cube."""
    LO, HI = (3, 6, 9), (8, 11, 14)

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(1.0))
        self.register_buffer("calls", torch.zeros(()))

    def inside(self, size):
        m = torch.zeros(size, dtype=torch.bool)
        m[self.LO[0]:self.HI[0], self.LO[1]:self.HI[1], self.LO[2]:self.HI[2]] = True
        return m

    def forward(self, x):
        s = self.gain * x[:, 0, self.LO[0]:self.HI[0], self.LO[1]:self.HI[1], self.LO[2]:self.HI[2]].mean((1, 2, 3))
        return torch.stack([s, -s], 1)


def cube_volumes(seed, B=2, size=(16, 16, 16), dtype=F32):
    g = torch.Generator().manual_seed(seed & 0x7FFFFFFF)
    return torch.rand((B, 1) + size, generator=g, dtype=dtype) + 0.5


@pytest.mark.parametrize("seed", ri.SEEDS)
def test_rise_finds_the_planted_cube(seed):
    """rise_torch on (16, 16, 16), cells 4, p 0.5, N = 256, volumes uniform in [0.5, 1.5]: the map's mean inside the cube
    exceeds its mean outside by at least one standard deviation of the outside voxels.  The model, the caller's tensors and
    torch's generator stay untouched."""
    from transmf_ad_amd import rise_torch
    net = Cube().eval()
    x = cube_volumes(seed)
    keep, rng = x.clone(), torch.get_rng_state()
    r = rise_torch(net, x, masks=256, cells=4, p=0.5, seed=seed, score="logit", target=0)
    assert torch.equal(x, keep) and torch.equal(torch.get_rng_state(), rng) and net.gain.grad is None and float(net.calls) == 0
    sal, inside = r.map(0), net.inside((16, 16, 16))
    assert tuple(sal.shape) == (2, 16, 16, 16) and tuple(r.scores(0).shape) == (2, 256) and r.masks == 256
    assert r.cells == (4, 4, 4) and r.cell == (4, 4, 4) and r.p == 0.5 and r.seed == seed and r.volumes == (0,)
    for b in range(2):
        margin = float((sal[b][inside].mean() - sal[b][~inside].mean()) / sal[b][~inside].std())
        print(f"seed {seed:#x} sample {b}: inside - outside = {margin:.2f} standard deviations of the outside voxels")
        assert margin >= 1.0


def test_rise_torch_options_and_errors():
    """scores are the model's own forward on rise_apply_torch batches under the same chunking; halves, coverage, baseline,
    joint, volumes; float64; every ValueError."""
    from transmf_ad_amd import Rise, gaussian_smooth_torch, ops, rise, rise_torch, smooth

    class Two(torch.nn.Module):
        def forward(self, x, y):
            s = (x[:, 0, 2:6, 2:6, 2:6].mean((1, 2, 3)) - y[:, 0, 4:8, 4:8, 4:8].mean((1, 2, 3)))
            return torch.stack([s, -s, 0 * s], 1), s

    net = Two().eval()
    g = torch.Generator().manual_seed(4)
    x, y = torch.rand((2, 1, 8, 8, 10), generator=g), torch.rand((2, 1, 8, 8, 10), generator=g)
    size, cells, N = (8, 8, 10), (2, 3, 4), 10
    r = rise_torch(net, x, y, masks=N, cells=cells, seed=5, chunk=7, halves=True, fill=0.25)
    assert isinstance(r, Rise) and r.volumes == (0, 1) and r.cell == (4, 3, 3) and r.coverage is None
    nodes, shifts = ops.rise_masks_torch(size, cells, 0.5, 5, 0, N)
    assert torch.equal(r.nodes, nodes) and torch.equal(r.mask(3), ops.rise_mask_values(nodes, shifts, size, cells)[3])
    fill = torch.full((2,), 0.25)
    for i, vols in ((0, (x, y)), (1, (x, y))):
        want = []
        for j0 in range(0, 2 * N, 7):
            K = min(7, 2 * N - j0)
            rows = torch.arange(j0, j0 + K) // N
            batch = [v.index_select(0, rows) for v in vols]
            batch[i] = ops.rise_apply_torch(vols[i], nodes, shifts, fill, size, cells, j0, K)
            want.append(torch.softmax(net(*batch)[0], 1).gather(1, r.target.index_select(0, rows).view(-1, 1))[:, 0])
        assert torch.equal(r.scores(i), torch.cat(want).view(2, N)), i
        assert torch.equal(r.map(i), ops.rise_accumulate_torch(r.scores(i), nodes, shifts, size, cells, 1.0 / (N * 0.5)))
        even, odd = r.halves(i)
        assert torch.equal(even, ops.rise_accumulate_torch(r.scores(i), nodes, shifts, size, cells, 1.0 / (5 * 0.5), 0, 2))
        assert torch.equal(odd, ops.rise_accumulate_torch(r.scores(i), nodes, shifts, size, cells, 1.0 / (5 * 0.5), 1, 2))
        sh = r.split_half(i)
        assert tuple(sh.shape) == (2,) and bool((sh.abs() <= 1 + 1e-6).all())
    with pytest.raises(KeyError):
        r.map(2)
    c = rise_torch(net, x, y, masks=N, cells=cells, seed=5, normalize="coverage", volumes=1, baseline="blur", score="logit", output=0)
    cover = ops.rise_accumulate_torch(torch.ones((1, N)), nodes, shifts, size, cells)[0]
    assert c.volumes == (1,) and torch.equal(c.coverage, cover) and float(cover.min()) >= 0 and float(cover.max()) <= N * ri.MASK_MAX
    blur = gaussian_smooth_torch(y, sigma=smooth.BLUR_SIGMA)
    b = rise_torch(net, x, y, masks=N, cells=cells, seed=5, normalize="coverage", volumes=(1,), baseline=blur, score="logit")
    assert torch.equal(b.scores(), c.scores()) and torch.equal(b.map(), c.map())
    total = ops.rise_accumulate_torch(c.scores(), nodes, shifts, size, cells)
    assert torch.equal(c.map(), torch.where(cover > 0, total / cover, torch.zeros(())))
    with pytest.raises(ValueError, match="halves"):
        c.halves()
    j = rise_torch(net, x, y, masks=N, cells=cells, seed=5, joint=True, output=0)
    assert torch.equal(j.map(0), j.map(1)) and torch.equal(j.map(), j.map(0)) and not torch.equal(j.scores(), r.scores(0))
    assert torch.equal(rise(net, x, y, masks=N, cells=cells, seed=5, joint=True).map(), j.map())          # CPU tensors: the twins
    d = rise_torch(net.double(), x.double(), y.double(), masks=N, cells=cells, seed=5, fill=0.25)
    assert d.map(0).dtype == F64 and float((d.map(0) - r.map(0)).abs().max()) < 1e-5
    ok = dict(masks=4, cells=2)
    for kw in (dict(cells=0), dict(cells=9), dict(cells=(2, 2)), dict(cells=2.0), dict(p=0.0), dict(p=1.0), dict(p=None),
               dict(masks=0), dict(masks=1, halves=True), dict(masks=2.5), dict(normalize="mean"), dict(baseline="gauss"),
               dict(baseline=torch.zeros(3)), dict(fill="median"), dict(fill=torch.zeros(3)), dict(score="margin"),
               dict(volumes=2), dict(volumes=(0, 0)), dict(volumes=()), dict(chunk=0), dict(seed=-1), dict(output=2), dict(target=5)):
        with pytest.raises(ValueError):
            rise_torch(net, x, y, **dict(ok, **kw))
    with pytest.raises(ValueError, match="eval"):
        rise_torch(Two().train(), x, y, **ok)
    with pytest.raises(ValueError, match="eval"):
        rise(Two().train(), x, y, **ok)
